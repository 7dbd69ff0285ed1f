// draco_amd HIP/CDNA4 kernels — MI355X (gfx950) native.
//
// Every coding / aggregation / optimizer hot spot of the framework runs through the
// kernels in this file (SURVEY.md §2.5 K1-K12 inventory; reference semantics cited per
// kernel).  All of them are HBM-bandwidth-bound elementwise/reduction kernels over the
// flat gradient space (d up to ~10^7 fp32 per model replica), so the design rules are
// the memory ones from the CDNA4 guide: 256-thread blocks (4 waves of 64), float4
// (16 B/lane) vectorized access, grid-stride loops capped at ~2048 blocks, wave-level
// __shfl reductions (wave = 64 lanes on CDNA4, not 32).  The exceptions are the three
// column-sort kernels (k_col_trimmed_mean: median / trimmed mean; k_col_mean_around:
// mean around median / Phocas; k_seg_mean_around: Multi-Krum / Bulyan over per-segment
// row selections), which sort each column in registers and are VALU-heavy.  k_collude
// (colluding ALIE / inner-product adversaries) keeps a column in registers as they do,
// four columns per lane, without the sort; k_clip_step (centered clipping) does the
// same and carries per-row distance accumulators on top.
//
// Build: hipcc --offload-arch=gfx950 (tools/build_ext.py); loaded as torch extension
// draco_amd._hip_ops.  No CUDA path, no hipify — HIP-native source.

#include <torch/extension.h>
#include <c10/hip/HIPException.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#define WAVE 64
#define NTHREADS 256

// --------------------------------------------------------------------------- shared helpers
static inline int n_blocks(long work, int per_block) {
  long b = (work + per_block - 1) / per_block;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

#define CHECK_IN(t) \
  TORCH_CHECK(t.is_cuda(), #t " must be on GPU"); \
  TORCH_CHECK(t.is_contiguous(), #t " must be contiguous")

// index / segment-bound tensors: the kernels read them as 64-bit
#define CHECK_IDX(t) \
  CHECK_IN(t); \
  TORCH_CHECK(t.scalar_type() == torch::kInt64, #t " must be int64")

// Every launch of this file: NTHREADS-thread blocks on the current stream, followed by
// the launch-error check (a hipGetLastError on the host, no synchronisation), so a
// launch the runtime refuses raises instead of leaving the output as it was.
template <typename... Params, typename... Args>
static inline void launch(void (*kernel)(Params...), dim3 grid, size_t lds_bytes,
                          Args... args) {
  hipLaunchKernelGGL(kernel, grid, dim3(NTHREADS), lds_bytes,
                     c10::hip::getCurrentHIPStream().stream(), args...);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// The kernels that keep a column of P rows in registers are compiled for the padded
// sizes below; f gets the smallest one >= P as a std::integral_constant, so that it is
// a compile-time constant inside a generic lambda.
template <typename F>
static inline void for_padded(long P, F &&f) {
  if (P <= 4) f(std::integral_constant<int, 4>{});
  else if (P <= 8) f(std::integral_constant<int, 8>{});
  else if (P <= 12) f(std::integral_constant<int, 12>{});
  else if (P <= 16) f(std::integral_constant<int, 16>{});
  else if (P <= 24) f(std::integral_constant<int, 24>{});
  else if (P <= 32) f(std::integral_constant<int, 32>{});
  else if (P <= 48) f(std::integral_constant<int, 48>{});
  else f(std::integral_constant<int, 64>{});
}

// The optional nan-guard flag of the optimizer steps: an empty tensor means no guard.
static inline const bool *guard_ptr(const torch::Tensor &guard) {
  if (guard.numel() == 0) return nullptr;
  TORCH_CHECK(guard.is_cuda() && guard.scalar_type() == torch::kBool, "guard must be a GPU bool");
  return guard.data_ptr<bool>();
}

// x of the vote statistics: (rows, d), with d % 4 == 0 where the kernel reads float4
static inline void check_rows(const char *op, const torch::Tensor &x, bool vec4) {
  CHECK_IN(x);
  TORCH_CHECK(x.dim() == 2, op, ": x must be 2D");
  TORCH_CHECK(!vec4 || x.size(1) % 4 == 0, op, ": row length must be a multiple of 4");
}

// ... and the row pairs (a_idx[k], b_idx[k]) of the pairwise ones
static inline void check_pairs(const char *op, const torch::Tensor &x, const torch::Tensor &a_idx,
                               const torch::Tensor &b_idx, bool vec4) {
  check_rows(op, x, vec4);
  CHECK_IDX(a_idx); CHECK_IDX(b_idx);
  TORCH_CHECK(a_idx.numel() == b_idx.numel(), op, ": index lengths differ");
}

// seg holds the L+1 bounds of L segments; returns L
static inline long segment_count(const char *op, const torch::Tensor &seg) {
  CHECK_IDX(seg);
  TORCH_CHECK(seg.dim() == 1 && seg.numel() >= 1, op, ": seg must be 1D with L+1 >= 1 bounds");
  return seg.numel() - 1;
}

// The segment kernels stage the bounds in dynamic LDS, and `per_segment` more bytes
// per segment behind them: L, and the LDS request checked against what a block may take.
struct SegmentLds { int L; size_t bytes; };
static inline SegmentLds segment_lds(const char *op, const torch::Tensor &seg,
                                     size_t per_segment) {
  long L = segment_count(op, seg);
  size_t bytes = (size_t)(L + 1) * sizeof(long) + (size_t)L * per_segment;
  TORCH_CHECK(bytes <= 64 * 1024, op, ": ", L, " segments take ", bytes,
              " bytes of LDS, a block may take 65536");
  return {(int)L, bytes};
}

// Device side of the same: stage the bounds (the caller's __syncthreads() follows) ...
__device__ __forceinline__ void stage_segments(long *s_seg, const long *__restrict__ seg, int L) {
  for (int i = threadIdx.x; i <= L; i += blockDim.x) s_seg[i] = seg[i];
}

// ... whether column i lies in any segment (false for every i when L = 0) ...
__device__ __forceinline__ bool in_segments(const long *s_seg, int L, long i) {
  return i >= s_seg[0] && i < s_seg[L];
}

// ... and, for such a column, the segment l with seg[l] <= i < seg[l+1] (binary search;
// empty segments are skipped over)
__device__ __forceinline__ int find_segment(const long *s_seg, int L, long i) {
  int lo = 0, hi = L - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (s_seg[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// 64-lane __shfl_down trees: lane 0 ends up with the wave's result
struct SumOp { __device__ float operator()(float a, float b) const { return a + b; } };
struct MaxOp { __device__ float operator()(float a, float b) const { return fmaxf(a, b); } };

template <typename Op>
__device__ __forceinline__ float wave_reduce(float v, Op op) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) v = op(v, __shfl_down(v, off, WAVE));
  return v;
}
__device__ __forceinline__ float wave_reduce_sum(float v) { return wave_reduce(v, SumOp{}); }
__device__ __forceinline__ float wave_reduce_max(float v) { return wave_reduce(v, MaxOp{}); }

// Block step on top: the NTHREADS / WAVE wave results go through LDS and thread 0 folds
// them onto `init` in ascending wave order.  The return value is the block's result in
// thread 0 only.
template <typename Op>
__device__ __forceinline__ float block_reduce(float wave_result, float init, Op op) {
  __shared__ float part[NTHREADS / WAVE];
  if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = wave_result;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int wv = 0; wv < NTHREADS / WAVE; ++wv) init = op(init, part[wv]);
  return init;
}

// Column i of the P rows of x into s[0..n): NaN -> +inf (the vote statistics' rule),
// rows P..n-1 are +inf padding.  n is the caller's compile-time padded size, passed as
// an argument on purpose: the loop then unrolls only once it is inlined, together with
// the kernel's own loops, and the kernels compile to what they were with the loop
// written out in them.  With n a template parameter the loop unrolls before inlining,
// the loads' loop-invariant address arithmetic is hoisted in another order, and
// k_col_mean_around measured 0.4-2.5 % slower at P < n
// (profiles/kernel_bw_shared_helpers.txt).  After unrolling s[] is indexed by
// compile-time constants only.
__device__ __forceinline__ void load_column(float *s, int n, const float *x, int P, long stride,
                                            long i) {
#pragma unroll
  for (int p = 0; p < n; ++p) {
    float v = INFINITY;
    if (p < P) {
      v = x[p * stride + i];
      v = (v != v) ? INFINITY : v;
    }
    s[p] = v;
  }
}

// --------------------------------------------------------------------------- SGD
// Fused flat SGD + momentum/nesterov/weight-decay (reference semantics:
// optim/sgd_modified.py:53-89 including the first-step dampening quirk).
// One launch for the whole parameter space vs the reference's per-tensor loop.
template <bool MOM, bool NESTEROV>
__global__ void k_sgd(float4 *__restrict__ p, const float4 *__restrict__ g,
                      float4 *__restrict__ buf, long n4, float lr, float momentum,
                      float grad_scale /* 1-dampening, or 1 on first step */, float wd,
                      const bool *__restrict__ guard /* device flag: 0 -> skip update */) {
  if (guard != nullptr && !*guard) return;  // nan-guard: whole update is a no-op
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = gridDim.x * (long)blockDim.x;
  for (; i < n4; i += stride) {
    float4 pv = p[i];
    float4 gv = g[i];
    float dp[4] = {gv.x, gv.y, gv.z, gv.w};
    float pp[4] = {pv.x, pv.y, pv.z, pv.w};
    if (wd != 0.f) {
#pragma unroll
      for (int c = 0; c < 4; ++c) dp[c] = fmaf(wd, pp[c], dp[c]);
    }
    if (MOM) {
      float4 bv = buf[i];
      float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        bb[c] = fmaf(momentum, bb[c], grad_scale * dp[c]);
        dp[c] = NESTEROV ? fmaf(momentum, bb[c], dp[c]) : bb[c];
      }
      buf[i] = make_float4(bb[0], bb[1], bb[2], bb[3]);
#pragma unroll
      for (int c = 0; c < 4; ++c) pp[c] = fmaf(-lr, dp[c], pp[c]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) pp[c] = fmaf(-lr, dp[c], pp[c]);
    }
    p[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
  }
}

void fused_sgd_step(torch::Tensor param, torch::Tensor grad, torch::Tensor buf,
                    double lr, double momentum, double dampening, double weight_decay,
                    bool nesterov, bool first_step, torch::Tensor guard) {
  CHECK_IN(param); CHECK_IN(grad);
  TORCH_CHECK(param.numel() % 4 == 0, "flat param length must be a multiple of 4");
  TORCH_CHECK(grad.numel() == param.numel(), "fused_sgd_step: grad must have param's length");
  long n4 = param.numel() / 4;
  int blocks = n_blocks(n4, NTHREADS);
  bool mom = momentum != 0.0;
  float gscale = first_step ? 1.f : (1.f - (float)dampening);
  auto pp = (float4 *)param.data_ptr<float>();
  auto gg = (const float4 *)grad.data_ptr<float>();
  float4 *bb = nullptr;
  const bool *gd = guard_ptr(guard);
  if (mom) {
    CHECK_IN(buf);
    TORCH_CHECK(buf.numel() == param.numel(), "fused_sgd_step: buf must have param's length");
    bb = (float4 *)buf.data_ptr<float>();
  }
  auto kernel = mom && nesterov ? k_sgd<true, true> : mom ? k_sgd<true, false> : k_sgd<false, false>;
  launch(kernel, dim3(blocks), 0, pp, gg, bb, n4, (float)lr, (float)momentum, gscale,
         (float)weight_decay, gd);
}

// --------------------------------------------------------------------------- Adam
// Fused flat Adam/AMSGrad (reference: optim/adam_modified.py:32-93).
template <bool AMS>
__global__ void k_adam(float4 *__restrict__ p, const float4 *__restrict__ g,
                       float4 *__restrict__ m, float4 *__restrict__ v,
                       float4 *__restrict__ vmax, long n4, float lr_t, float beta1,
                       float beta2, float omb1 /* 1-beta1 */, float omb2 /* 1-beta2 */,
                       float eps, float wd,
                       const bool *__restrict__ guard) {
  if (guard != nullptr && !*guard) return;  // nan-guard: whole update is a no-op
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = gridDim.x * (long)blockDim.x;
  for (; i < n4; i += stride) {
    float4 pv = p[i], gv = g[i], mv = m[i], vv = v[i];
    float pp[4] = {pv.x, pv.y, pv.z, pv.w};
    float dg[4] = {gv.x, gv.y, gv.z, gv.w};
    float mm[4] = {mv.x, mv.y, mv.z, mv.w};
    float ss[4] = {vv.x, vv.y, vv.z, vv.w};
    float dn[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (wd != 0.f) dg[c] = fmaf(wd, pp[c], dg[c]);
      mm[c] = fmaf(beta1, mm[c], omb1 * dg[c]);
      ss[c] = fmaf(beta2, ss[c], omb2 * dg[c] * dg[c]);
      dn[c] = ss[c];
    }
    if (AMS) {
      float4 xv = vmax[i];
      float xx[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) { xx[c] = fmaxf(xx[c], ss[c]); dn[c] = xx[c]; }
      vmax[i] = make_float4(xx[0], xx[1], xx[2], xx[3]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      pp[c] -= lr_t * mm[c] / (sqrtf(dn[c]) + eps);
    m[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
    v[i] = make_float4(ss[0], ss[1], ss[2], ss[3]);
    p[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
  }
}

void fused_adam_step(torch::Tensor param, torch::Tensor grad, torch::Tensor exp_avg,
                     torch::Tensor exp_avg_sq, torch::Tensor max_exp_avg_sq, long step,
                     double lr, double beta1, double beta2, double eps,
                     double weight_decay, bool amsgrad, torch::Tensor guard) {
  CHECK_IN(param); CHECK_IN(grad); CHECK_IN(exp_avg); CHECK_IN(exp_avg_sq);
  TORCH_CHECK(param.numel() % 4 == 0, "flat param length must be a multiple of 4");
  TORCH_CHECK(grad.numel() == param.numel() && exp_avg.numel() == param.numel() &&
                  exp_avg_sq.numel() == param.numel(),
              "fused_adam_step: grad and state must have param's length");
  long n4 = param.numel() / 4;
  int blocks = n_blocks(n4, NTHREADS);
  double bc1 = 1.0 - pow(beta1, (double)step);
  double bc2 = 1.0 - pow(beta2, (double)step);
  float lr_t = (float)(lr * sqrt(bc2) / bc1);
  // 1-beta is formed in double: in fp32, 1.f - 0.999f cancels to 1.3e-5 relative
  // error, which lands undiminished in exp_avg_sq (the fallback uses the double too)
  float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  auto pp = (float4 *)param.data_ptr<float>();
  auto gg = (const float4 *)grad.data_ptr<float>();
  auto mm = (float4 *)exp_avg.data_ptr<float>();
  auto vv = (float4 *)exp_avg_sq.data_ptr<float>();
  float4 *xx = nullptr;
  const bool *gd = guard_ptr(guard);
  if (amsgrad) {
    CHECK_IN(max_exp_avg_sq);
    TORCH_CHECK(max_exp_avg_sq.numel() == param.numel(),
                "fused_adam_step: max_exp_avg_sq must have param's length");
    xx = (float4 *)max_exp_avg_sq.data_ptr<float>();
  }
  launch(amsgrad ? k_adam<true> : k_adam<false>, dim3(blocks), 0, pp, gg, mm, vv, xx, n4, lr_t,
         (float)beta1, (float)beta2, omb1, omb2, (float)eps, (float)weight_decay, gd);
}

// --------------------------------------------------------------------------- inject
// Adversary injection y = a*y + b covers every reference err_simulation mode
// (model_ops/utils.py:6-23): rev_grad (a=-100,b=0), rev_grad cyclic (a=-99,b=0),
// constant (a=0,b=-100), constant cyclic (a=1,b=-100).
__global__ void k_axpb(float4 *__restrict__ y, long n4, float a, float b) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = gridDim.x * (long)blockDim.x;
  for (; i < n4; i += stride) {
    float4 v = y[i];
    y[i] = make_float4(fmaf(a, v.x, b), fmaf(a, v.y, b), fmaf(a, v.z, b), fmaf(a, v.w, b));
  }
}

void inject(torch::Tensor grad, std::string mode, bool cyclic) {
  CHECK_IN(grad);
  const float ADV = -100.f;
  float a, b;
  if (mode == "rev_grad") { a = cyclic ? (1.f + ADV) : ADV; b = 0.f; }
  else if (mode == "constant") { a = cyclic ? 1.f : 0.f; b = ADV; }
  else TORCH_CHECK(false, "inject: unknown mode ", mode);
  TORCH_CHECK(grad.numel() % 4 == 0, "inject: length must be a multiple of 4");
  long n4 = grad.numel() / 4;
  launch(k_axpb, dim3(n_blocks(n4, NTHREADS)), 0, (float4 *)grad.data_ptr<float>(), n4, a, b);
}

// --------------------------------------------------------------------------- vote
// Majority-vote equality test (reference: np.array_equal per member,
// rep_master.py:154-168).  out[pair] preset to 1; any mismatching element anywhere in
// the shard stores 0 (benign race — no reduction needed, one pass at full bandwidth).
__global__ void k_rows_equal(const float4 *__restrict__ x, const long *__restrict__ ai,
                             const long *__restrict__ bi, unsigned char *__restrict__ out,
                             long d4, long stride4, float atol) {
  int pair = blockIdx.y;
  const float4 *ra = x + ai[pair] * stride4;
  const float4 *rb = x + bi[pair] * stride4;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = gridDim.x * (long)blockDim.x;
  bool neq = false;
  for (; i < d4; i += stride) {
    float4 a = ra[i], b = rb[i];
    neq |= !(fabsf(a.x - b.x) <= atol) | !(fabsf(a.y - b.y) <= atol) |
           !(fabsf(a.z - b.z) <= atol) | !(fabsf(a.w - b.w) <= atol);
  }
  // one store per wave suffices when any lane saw a mismatch (benign race on out)
  if (__any(neq) && (threadIdx.x & (WAVE - 1)) == 0) out[pair] = 0;
}

torch::Tensor rows_equal(torch::Tensor x, torch::Tensor a_idx, torch::Tensor b_idx,
                         double atol) {
  check_pairs("rows_equal", x, a_idx, b_idx, true);
  long k = a_idx.numel();
  long d = x.size(1);
  auto out = torch::ones({k}, torch::dtype(torch::kUInt8).device(x.device()));
  if (d == 0 || k == 0) return out;
  dim3 grid(n_blocks(d / 4, NTHREADS), (unsigned)k);
  launch(k_rows_equal, grid, 0, (const float4 *)x.data_ptr<float>(), a_idx.data_ptr<long>(),
         b_idx.data_ptr<long>(), out.data_ptr<unsigned char>(), d / 4, d / 4, (float)atol);
  return out;
}

// Tolerance-vote statistics: per-pair max|a-b| and per-row max|x| over the shard.
// (MIOpen conv backward is not bitwise-reproducible on this stack, so the GPU vote is
// tolerance-based: equal iff max|a-b| <= atol + rtol*max(rowmax_a, rowmax_b) — the
// thresholds are combined host-side after a cross-rank MAX allreduce.)
__device__ inline void atomic_max_f32(float *addr, float val) {
  // valid for non-negative floats: IEEE ordering matches int ordering
  atomicMax((int *)addr, __float_as_int(val));
}

// Non-finite rule of the four vote statistics: |v| with NaN canonicalised to +inf, so
// any NaN/+-Inf element (Inf - Inf included) makes its cell exactly +inf.  fmaxf
// alone DROPS a NaN operand, which would let a NaN-sending member compare equal to
// everyone.  +inf (not NaN) because the statistic goes through a cross-rank MAX
// allreduce next, and it is the largest value under the float-as-int atomicMax.
__device__ inline float abs_nan_inf(float v) {
  float a = fabsf(v);
  return (a != a) ? INFINITY : a;
}

template <bool PAIR>
__global__ void k_absmax(const float4 *__restrict__ x, const long *__restrict__ ai,
                         const long *__restrict__ bi, float *__restrict__ out, long d4,
                         long stride4) {
  int row = blockIdx.y;
  const float4 *ra = x + (PAIR ? ai[row] : (long)row) * stride4;
  const float4 *rb = PAIR ? (x + bi[row] * stride4) : nullptr;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = gridDim.x * (long)blockDim.x;
  // |v| as its bit pattern orders like the float for every non-NaN value, and a NaN
  // pattern sorts ABOVE +inf: the integer max keeps a NaN that fmaxf would drop, and
  // one min against +inf's pattern then applies the non-finite rule per thread
  int mi = 0;
  for (; i < d4; i += stride) {
    float4 a = ra[i];
    if (PAIR) {
      float4 b = rb[i];
      a = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
    }
    mi = max(mi, max(max(__float_as_int(a.x) & 0x7fffffff, __float_as_int(a.y) & 0x7fffffff),
                     max(__float_as_int(a.z) & 0x7fffffff, __float_as_int(a.w) & 0x7fffffff)));
  }
  float mx = __int_as_float(min(mi, 0x7f800000));
  // mx >= +0 and never NaN, so folding onto 0 changes nothing
  float tot = block_reduce(wave_reduce_max(mx), 0.f, MaxOp{});
  if (threadIdx.x == 0) atomic_max_f32(&out[row], tot);
}

torch::Tensor pair_maxdiff(torch::Tensor x, torch::Tensor a_idx, torch::Tensor b_idx) {
  check_pairs("pair_maxdiff", x, a_idx, b_idx, true);
  long k = a_idx.numel(), d = x.size(1);
  auto out = torch::zeros({k}, torch::dtype(torch::kFloat32).device(x.device()));
  if (d == 0 || k == 0) return out;
  dim3 grid(n_blocks(d / 4 / 8, NTHREADS), (unsigned)k);
  launch(k_absmax<true>, grid, 0, (const float4 *)x.data_ptr<float>(), a_idx.data_ptr<long>(),
         b_idx.data_ptr<long>(), out.data_ptr<float>(), d / 4, d / 4);
  return out;
}

torch::Tensor row_absmax(torch::Tensor x) {
  check_rows("row_absmax", x, true);
  long m = x.size(0), d = x.size(1);
  auto out = torch::zeros({m}, torch::dtype(torch::kFloat32).device(x.device()));
  if (d == 0 || m == 0) return out;
  dim3 grid(n_blocks(d / 4 / 8, NTHREADS), (unsigned)m);
  launch(k_absmax<false>, grid, 0, (const float4 *)x.data_ptr<float>(), nullptr, nullptr,
         out.data_ptr<float>(), d / 4, d / 4);
  return out;
}

// Per-SEGMENT tolerance-vote statistics: the segment-granular vote bounds a
// within-tolerance adversary to rtol*segmax per parameter tensor instead of
// rtol*rowmax over the whole gradient (~10x tighter for late small layers).
// Same layout as k_seg_sqdist: segment bounds in LDS (stage_segments), find_segment
// per element.  The grid-stride loop makes a thread's CONSECUTIVE elements gstride
// apart, i.e. almost always in DIFFERENT segments — so a per-thread running maximum
// flushed on segment change degenerates to one GLOBAL atomic per element (measured
// 4-7 GB/s).  Instead each block accumulates into an LDS per-segment array (LDS
// atomics: conflict-serialised but ~3 orders cheaper than L2) and flushes ONCE per
// (block, segment).
template <bool PAIR>
__global__ void k_seg_absmax(const float *__restrict__ x, const long *__restrict__ ai,
                             const long *__restrict__ bi, const long *__restrict__ seg,
                             int L, float *__restrict__ out /* (rows, L) */, long d,
                             long stride) {
  extern __shared__ char smem[];
  long *s_seg = (long *)smem;
  int *s_max = (int *)(smem + (L + 1) * sizeof(long));  // float bits (non-negative)
  stage_segments(s_seg, seg, L);
  for (int i = threadIdx.x; i < L; i += blockDim.x) s_max[i] = 0;
  __syncthreads();
  int r = blockIdx.y;
  const float *ra = x + (PAIR ? ai[r] : (long)r) * stride;
  const float *rb = PAIR ? (x + bi[r] * stride) : nullptr;
  long gstride = gridDim.x * (long)blockDim.x;
  // base-indexed loop: the trip condition is uniform per block, so every lane is
  // active at each __shfl/__all (a wave whose 64 lanes share a segment — the
  // common case — pre-reduces in registers and issues ONE LDS atomic)
  for (long base = blockIdx.x * (long)blockDim.x; base < d; base += gstride) {
    long i = base + threadIdx.x;
    bool valid = (i < d) && in_segments(s_seg, L, i);
    int lo = 0;
    float v = 0.f;
    if (valid) {
      lo = find_segment(s_seg, L, i);
      v = abs_nan_inf(PAIR ? (ra[i] - rb[i]) : ra[i]);  // feeds both paths below
    }
    int lo0 = __shfl(lo, 0, WAVE);
    if (__all(valid && lo == lo0)) {
      v = wave_reduce_max(v);
      if ((threadIdx.x & (WAVE - 1)) == 0) atomicMax(&s_max[lo0], __float_as_int(v));
    } else if (valid) {
      atomicMax(&s_max[lo], __float_as_int(v));
    }
  }
  __syncthreads();
  for (int l = threadIdx.x; l < L; l += blockDim.x) {
    float m = __int_as_float(s_max[l]);
    if (m > 0.f) atomic_max_f32(&out[r * L + l], m);  // +inf passes; NaN never gets here
  }
}

torch::Tensor segment_absmax(torch::Tensor x, torch::Tensor seg) {
  check_rows("segment_absmax", x, false);
  SegmentLds sl = segment_lds("segment_absmax", seg, sizeof(int));
  long m = x.size(0), d = x.size(1);
  auto out = torch::zeros({m, sl.L}, torch::dtype(torch::kFloat32).device(x.device()));
  if (d == 0 || m == 0) return out;
  dim3 grid(n_blocks(d / 8, NTHREADS), (unsigned)m);
  launch(k_seg_absmax<false>, grid, sl.bytes, x.data_ptr<float>(), nullptr, nullptr,
         seg.data_ptr<long>(), sl.L, out.data_ptr<float>(), d, d);
  return out;
}

torch::Tensor segment_pair_maxdiff(torch::Tensor x, torch::Tensor a_idx,
                                   torch::Tensor b_idx, torch::Tensor seg) {
  check_pairs("segment_pair_maxdiff", x, a_idx, b_idx, false);
  SegmentLds sl = segment_lds("segment_pair_maxdiff", seg, sizeof(int));
  long k = a_idx.numel(), d = x.size(1);
  auto out = torch::zeros({k, sl.L}, torch::dtype(torch::kFloat32).device(x.device()));
  if (d == 0 || k == 0) return out;
  dim3 grid(n_blocks(d / 8, NTHREADS), (unsigned)k);
  launch(k_seg_absmax<true>, grid, sl.bytes, x.data_ptr<float>(), a_idx.data_ptr<long>(),
         b_idx.data_ptr<long>(), seg.data_ptr<long>(), sl.L, out.data_ptr<float>(), d, d);
  return out;
}

// --------------------------------------------------------------------------- combine
// Generic weighted row combination out[j] = sum_i w[i] * x[rows[i]][j].
// Serves: mean of group winners (K8), sum_rows, cyclic encode per-plane and the final
// decode recombination Re(v @ R) (K1/K5) — the n<=2*64 coefficients live in L2 and are
// re-read per thread (negligible vs the d-wide streams).
__global__ void k_combine(const float4 *__restrict__ x, const long *__restrict__ rows,
                          const float *__restrict__ w, int m, float4 *__restrict__ out,
                          long d4, long stride4) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = gridDim.x * (long)blockDim.x;
  for (; i < d4; i += stride) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < m; ++r) {
      float4 v = x[rows[r] * stride4 + i];
      float wr = w[r];
      acc[0] = fmaf(wr, v.x, acc[0]);
      acc[1] = fmaf(wr, v.y, acc[1]);
      acc[2] = fmaf(wr, v.z, acc[2]);
      acc[3] = fmaf(wr, v.w, acc[3]);
    }
    out[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
}

static void launch_combine(torch::Tensor x, torch::Tensor rows, torch::Tensor w,
                           torch::Tensor out, long stride_elems, long col_off = 0) {
  long d = out.numel();
  TORCH_CHECK(d % 4 == 0 && stride_elems % 4 == 0 && col_off % 4 == 0,
              "combine: 16-byte alignment required");
  TORCH_CHECK(w.numel() == rows.numel(), "combine: one weight per row index required");
  TORCH_CHECK(x.dim() == 2 && d <= x.size(1), "combine: out is longer than a row of x");
  launch(k_combine, dim3(n_blocks(d / 4, NTHREADS)), 0,
         (const float4 *)(x.data_ptr<float>() + col_off), rows.data_ptr<long>(),
         w.data_ptr<float>(), (int)rows.numel(), (float4 *)out.data_ptr<float>(), d / 4,
         stride_elems / 4);
}

// Bucketed cyclic encode (per-layer overlap): combine only the [col_off,
// col_off + out.numel()) column range of the source rows into `out` (the matching
// slice of the encoded plane).  Same arithmetic per element as the full-row
// combine, so bucketed and whole-row encodes are bit-identical.
void combine_rows_slice(torch::Tensor x, torch::Tensor rows, torch::Tensor w,
                        torch::Tensor out, long col_off) {
  CHECK_IN(x); CHECK_IDX(rows); CHECK_IN(w); CHECK_IN(out);
  TORCH_CHECK(col_off + out.numel() <= x.size(1), "combine slice out of range");
  launch_combine(x, rows, w, out, x.size(1), col_off);
}

void mean_rows(torch::Tensor x, torch::Tensor idx, torch::Tensor out) {
  CHECK_IN(x); CHECK_IDX(idx); CHECK_IN(out);
  auto w = torch::full({idx.numel()}, 1.0 / (double)idx.numel(),
                       torch::dtype(torch::kFloat32).device(x.device()));
  launch_combine(x, idx, w, out, x.size(1));
}

void sum_rows(torch::Tensor x, torch::Tensor out) {
  CHECK_IN(x); CHECK_IN(out);
  auto idx = torch::arange(x.size(0), torch::dtype(torch::kInt64).device(x.device()));
  auto w = torch::ones({x.size(0)}, torch::dtype(torch::kFloat32).device(x.device()));
  launch_combine(x, idx, w, out, x.size(1));
}

// Cyclic encode (K1, cyclic_worker.py:172-176): one read of the (2s+1, d) sub-batch
// gradients produces BOTH complex planes (re/im written in the same pass).
__global__ void k_encode2(const float4 *__restrict__ g, const float *__restrict__ wre,
                          const float *__restrict__ wim, int m, float4 *__restrict__ outre,
                          float4 *__restrict__ outim, long d4, long stride4) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = gridDim.x * (long)blockDim.x;
  for (; i < d4; i += stride) {
    float re[4] = {0, 0, 0, 0}, im[4] = {0, 0, 0, 0};
    for (int r = 0; r < m; ++r) {
      float4 v = g[r * stride4 + i];
      float a = wre[r], b = wim[r];
      re[0] = fmaf(a, v.x, re[0]); im[0] = fmaf(b, v.x, im[0]);
      re[1] = fmaf(a, v.y, re[1]); im[1] = fmaf(b, v.y, im[1]);
      re[2] = fmaf(a, v.z, re[2]); im[2] = fmaf(b, v.z, im[2]);
      re[3] = fmaf(a, v.w, re[3]); im[3] = fmaf(b, v.w, im[3]);
    }
    outre[i] = make_float4(re[0], re[1], re[2], re[3]);
    outim[i] = make_float4(im[0], im[1], im[2], im[3]);
  }
}

void cyclic_encode(torch::Tensor grads, torch::Tensor w_re, torch::Tensor w_im,
                   torch::Tensor out) {
  CHECK_IN(grads); CHECK_IN(w_re); CHECK_IN(w_im); CHECK_IN(out);
  TORCH_CHECK(grads.dim() == 2 && out.dim() == 2 && out.size(0) == 2,
              "cyclic_encode: grads must be (k, d') and out (2, d)");
  long d = out.size(1);
  long stride = grads.size(1);
  TORCH_CHECK(d % 4 == 0 && stride % 4 == 0,
              "cyclic_encode: row lengths must be multiples of 4");
  TORCH_CHECK(stride >= d, "cyclic_encode: grads rows are shorter than out rows");
  TORCH_CHECK(w_re.numel() == grads.size(0) && w_im.numel() == grads.size(0),
              "cyclic_encode: w_re and w_im need one weight per grads row");
  launch(k_encode2, dim3(n_blocks(d / 4, NTHREADS)), 0,
         (const float4 *)grads.data_ptr<float>(), w_re.data_ptr<float>(),
         w_im.data_ptr<float>(), (int)grads.size(0), (float4 *)out.data_ptr<float>(),
         (float4 *)out.data_ptr<float>() + d / 4, d / 4, stride / 4);
}

void cyclic_recombine(torch::Tensor r_planes, torch::Tensor v_re, torch::Tensor v_im,
                      torch::Tensor out) {
  CHECK_IN(r_planes); CHECK_IN(out);
  TORCH_CHECK(r_planes.dim() == 3 && r_planes.size(1) == 2,
              "cyclic_recombine: r_planes must be (n, 2, d)");
  TORCH_CHECK(v_re.numel() == r_planes.size(0) && v_im.numel() == r_planes.size(0),
              "cyclic_recombine: v_re and v_im need one weight per worker");
  // rows (2i, 2i+1) are worker i's (re, im) planes; Re(v @ R) = sum vre*re - vim*im
  long n = r_planes.size(0);
  auto dev = r_planes.device();
  auto rows = torch::arange(2 * n, torch::dtype(torch::kInt64).device(dev));
  auto w = torch::stack({v_re, -v_im}, 1).reshape({2 * n}).contiguous().to(dev);
  launch_combine(r_planes.view({2 * n, -1}), rows, w, out, r_planes.size(2));
}

// --------------------------------------------------------------------------- project
// K3 (cyclic_master.py:154): partial projection proj[i] = sum_d R[i,d] * z[d] over the
// local shard.  One block row per (worker, plane); wave_reduce_sum, then block_reduce
// across the block's 4 waves, one atomicAdd per block.
__global__ void k_project(const float4 *__restrict__ r, const float4 *__restrict__ z,
                          float *__restrict__ out, long d4, long stride4) {
  int row = blockIdx.y;
  const float4 *rr = r + row * stride4;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = gridDim.x * (long)blockDim.x;
  float acc = 0.f;
  for (; i < d4; i += stride) {
    float4 a = rr[i], b = z[i];
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    acc = fmaf(a.w, b.w, acc);
  }
  float tot = block_reduce(wave_reduce_sum(acc), 0.f, SumOp{});
  if (threadIdx.x == 0) atomicAdd(&out[row], tot);
}

torch::Tensor cyclic_project(torch::Tensor rows, torch::Tensor z) {
  CHECK_IN(rows); CHECK_IN(z);
  TORCH_CHECK(rows.dim() == 2, "cyclic_project: rows must be 2D");
  long m = rows.size(0);
  long d = rows.size(1);
  TORCH_CHECK(d % 4 == 0, "cyclic_project: row length must be a multiple of 4");
  TORCH_CHECK(z.numel() == d, "cyclic_project: z must have the rows' length");
  auto out = torch::zeros({m}, torch::dtype(torch::kFloat32).device(rows.device()));
  if (d == 0 || m == 0) return out;
  dim3 grid(n_blocks(d / 4 / 8, NTHREADS), (unsigned)m);
  launch(k_project, grid, 0, (const float4 *)rows.data_ptr<float>(),
         (const float4 *)z.data_ptr<float>(), out.data_ptr<float>(), d / 4, d / 4);
  return out;
}

void combine_rows(torch::Tensor x, torch::Tensor rows, torch::Tensor w, torch::Tensor out) {
  CHECK_IN(x); CHECK_IDX(rows); CHECK_IN(w); CHECK_IN(out);
  launch_combine(x, rows, w, out, x.size(1));
}

// --------------------------------------------------------------------------- geomed
// K6 (baseline_master.py:271-276 / hdmedians): per-(worker, layer-segment) partial
// squared distances for the sharded Weiszfeld iteration.  Segment bounds live in LDS
// (stage_segments), find_segment per element.  Same LDS-accumulate pattern as
// k_seg_absmax (see comment there): grid-stride means per-element segment changes, so
// per-thread flush-on-change would cost one GLOBAL atomic per element.  Blocks
// accumulate per-segment partial sums in LDS and flush once per (block, segment).
__global__ void k_seg_sqdist(const float *__restrict__ x, const float *__restrict__ z,
                             const long *__restrict__ seg, int L,
                             float *__restrict__ out /* (P, L) */, long d, long stride) {
  extern __shared__ char smem[];
  long *s_seg = (long *)smem;
  float *s_acc = (float *)(smem + (L + 1) * sizeof(long));
  stage_segments(s_seg, seg, L);
  for (int i = threadIdx.x; i < L; i += blockDim.x) s_acc[i] = 0.f;
  __syncthreads();
  int p = blockIdx.y;
  const float *row = x + p * stride;
  long gstride = gridDim.x * (long)blockDim.x;
  for (long base = blockIdx.x * (long)blockDim.x; base < d; base += gstride) {
    long i = base + threadIdx.x;
    bool valid = (i < d) && in_segments(s_seg, L, i);
    int lo = 0;
    float c = 0.f;
    if (valid) {
      lo = find_segment(s_seg, L, i);
      float dlt = row[i] - z[i];
      c = dlt * dlt;
    }
    int lo0 = __shfl(lo, 0, WAVE);
    if (__all(valid && lo == lo0)) {  // whole wave in one segment: one LDS atomic
      c = wave_reduce_sum(c);
      if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(&s_acc[lo0], c);
    } else if (valid) {
      atomicAdd(&s_acc[lo], c);
    }
  }
  __syncthreads();
  for (int l = threadIdx.x; l < L; l += blockDim.x)
    if (s_acc[l] != 0.f) atomicAdd(&out[p * L + l], s_acc[l]);
}

torch::Tensor segment_sqdist(torch::Tensor x, torch::Tensor z, torch::Tensor seg) {
  CHECK_IN(x); CHECK_IN(z);
  TORCH_CHECK(x.dim() == 2 && z.numel() == x.size(1),
              "segment_sqdist: z must have the length of a row of x");
  SegmentLds sl = segment_lds("segment_sqdist", seg, sizeof(float));
  long P = x.size(0), d = x.size(1);
  auto out = torch::zeros({P, sl.L}, torch::dtype(torch::kFloat32).device(x.device()));
  if (d == 0 || P == 0) return out;
  dim3 grid(n_blocks(d / 4, NTHREADS), (unsigned)P);
  launch(k_seg_sqdist, grid, sl.bytes, x.data_ptr<float>(), z.data_ptr<float>(),
         seg.data_ptr<long>(), sl.L, out.data_ptr<float>(), d, d);
  return out;
}

// Weiszfeld update z[j] = sum_p w[p, seg(j)] * x[p, j] (weights pre-normalised).
__global__ void k_seg_wmean(const float *__restrict__ x, const float *__restrict__ w,
                            const long *__restrict__ seg, int L, int P,
                            float *__restrict__ out, long d, long stride) {
  extern __shared__ long s_seg[];
  stage_segments(s_seg, seg, L);
  __syncthreads();
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long gstride = gridDim.x * (long)blockDim.x;
  for (; i < d; i += gstride) {
    if (!in_segments(s_seg, L, i)) continue;  // outside all segments: out is
    // left untouched, matching the CPU fallback (callers zero-init the buffer;
    // the [d, d_pad) padding tail must stay zero)
    int lo = find_segment(s_seg, L, i);
    float acc = 0.f;
    for (int p = 0; p < P; ++p) acc = fmaf(w[p * L + lo], x[p * stride + i], acc);
    out[i] = acc;
  }
}

void segment_weighted_mean(torch::Tensor x, torch::Tensor w, torch::Tensor seg,
                           torch::Tensor out) {
  CHECK_IN(x); CHECK_IN(w); CHECK_IN(out);
  TORCH_CHECK(x.dim() == 2, "segment_weighted_mean: x must be 2D");
  SegmentLds sl = segment_lds("segment_weighted_mean", seg, 0);
  long P = x.size(0), d = x.size(1);
  TORCH_CHECK(w.numel() == P * sl.L, "segment_weighted_mean: w must be (P, L)");
  TORCH_CHECK(out.numel() >= d, "segment_weighted_mean: out is shorter than a row of x");
  if (d == 0) return;
  launch(k_seg_wmean, dim3(n_blocks(d, NTHREADS)), sl.bytes, x.data_ptr<float>(),
         w.data_ptr<float>(), seg.data_ptr<long>(), sl.L, (int)P, out.data_ptr<float>(), d, d);
}

// --------------------------------------------------------------------------- krum
// K7 (baseline_master.py:278-296): per-segment Gram matrices for the pairwise
// distance matrix.  Host pre-splits segments into <=CHUNK-element descriptors; a block
// stages its chunk (P x CHUNK) through LDS and accumulates all P*P pair dots.
#define GRAM_CHUNK 256
#define GRAM_LD (GRAM_CHUNK + 1)  // +1 float: row stride odd mod 64 banks, so
                                  // lanes reading consecutive rows hit distinct
                                  // banks (stride 256/512 put EVERY lane on one
                                  // bank: measured 64-way conflict, ~50 GB/s)
__global__ void k_seg_gram(const float *__restrict__ x, const long *__restrict__ desc,
                           /* desc: (nchunks, 3) = (seg, start, len) */
                           int P, float *__restrict__ out /* (L, P, P) */, long stride) {
  __shared__ float tile[32][GRAM_LD];  // [P][chunk], padded leading dim
  int c = blockIdx.x;
  long segid = desc[c * 3 + 0];
  long start = desc[c * 3 + 1];
  long len = desc[c * 3 + 2];
  // cooperative load: threads sweep (p, e)
  for (long t = threadIdx.x; t < (long)P * len; t += blockDim.x) {
    int p = (int)(t / len);
    long e = t % len;
    tile[p][e] = x[p * stride + start + e];
  }
  __syncthreads();
  float *base = out + segid * P * P;
  for (int pair = threadIdx.x; pair < P * P; pair += blockDim.x) {
    int a = pair / P, b = pair % P;
    if (b < a) continue;  // symmetric: fill upper, mirror below
    // 4 independent accumulator chains: the naive single-chain form is a
    // len-deep dependent FMA+LDS sequence (latency-bound, measured ~60 GB/s)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    long e = 0;
    for (; e + 3 < len; e += 4) {
      a0 = fmaf(tile[a][e], tile[b][e], a0);
      a1 = fmaf(tile[a][e + 1], tile[b][e + 1], a1);
      a2 = fmaf(tile[a][e + 2], tile[b][e + 2], a2);
      a3 = fmaf(tile[a][e + 3], tile[b][e + 3], a3);
    }
    float acc = (a0 + a1) + (a2 + a3);
    for (; e < len; ++e) acc = fmaf(tile[a][e], tile[b][e], acc);
    atomicAdd(&base[a * P + b], acc);
    if (a != b) atomicAdd(&base[b * P + a], acc);
  }
}

torch::Tensor segment_gram(torch::Tensor x, torch::Tensor seg) {
  check_rows("segment_gram", x, false);
  long L = segment_count("segment_gram", seg);
  long P = x.size(0), d = x.size(1);
  TORCH_CHECK(P <= 32, "segment_gram kernel supports P <= 32");
  auto out = torch::zeros({L, P, P}, torch::dtype(torch::kFloat32).device(x.device()));
  // host-side chunk descriptors
  auto seg_c = seg.to(torch::kCPU);
  auto sp = seg_c.data_ptr<long>();
  std::vector<long> desc;
  for (int l = 0; l < L; ++l) {
    for (long s0 = sp[l]; s0 < sp[l + 1]; s0 += GRAM_CHUNK) {
      desc.push_back(l);
      desc.push_back(s0);
      desc.push_back(std::min((long)GRAM_CHUNK, sp[l + 1] - s0));
    }
  }
  if (desc.empty()) return out;
  auto desc_t = torch::from_blob(desc.data(), {(long)desc.size()}, torch::kInt64)
                    .clone().to(x.device());
  launch(k_seg_gram, dim3((unsigned)(desc.size() / 3)), 0, x.data_ptr<float>(),
         desc_t.data_ptr<long>(), (int)P, out.data_ptr<float>(), d);
  return out;
}

// --------------------------------------------------------------------------- trimmed mean
// Coordinate-wise median / beta-trimmed mean (Yin et al., arXiv:1803.01498): per
// column j, sort the P worker values (NaN -> +inf first, the vote statistics' rule)
// and average ranks [lo, hi) — added one at a time in ascending order, so the result
// is bit-identical to the CPU fallback.  Median: lo=(P-1)/2, hi=P/2+1.
//
// The first of the three kernels that sort (k_col_mean_around and k_seg_mean_around
// share its sort).  Each lane owns whole columns (consecutive lanes on consecutive
// columns: every row read is one coalesced 256 B wave access) and sorts in REGISTERS:
// the array s[] is only ever indexed by compile-time constants (a fully unrolled
// sorting network over the padded size N, chosen by for_padded), because a
// runtime-indexed per-thread array goes to scratch.  load_column's +inf padding rows
// sort to the top and never enter [lo, hi) since hi <= P.  fminf/fmaxf never see a NaN, so
// each compare-exchange is an exact permutation of its two inputs.
//
// The network is Batcher's merge exchange (Knuth 5.2.2 Algorithm M), built at compile
// time: it sorts ANY N (not just powers of two) with ascending comparators only —
// N=24 takes 127 compare-exchanges where a bitonic network padded to 32 takes 240,
// and the min/max pairs are the kernel's VALU cost (at 24 rows x 11.2M the bitonic
// form was VALU-bound: 593 us against combine_rows' 197 us for the same bytes).
template <int N>
struct MergeExchange {
  static constexpr int kMax = N * 6 * 7 / 4 + 1;  // N t(t+1)/4 bound, t = log2(64)
  int a[kMax], b[kMax];
  int n;
  constexpr MergeExchange() : a{}, b{}, n(0) {
    int t = 0;
    while ((1 << t) < N) ++t;
    for (int p = t > 0 ? 1 << (t - 1) : 0; p > 0; p >>= 1) {
      int q = 1 << (t - 1), r = 0, d = p;
      while (true) {
        for (int i = 0; i + d < N; ++i)
          if ((i & p) == r) { a[n] = i; b[n] = i + d; ++n; }
        if (q == p) break;
        d = q - p; q >>= 1; r = p;
      }
    }
  }
};
template <int N> constexpr MergeExchange<N> kMergeExchange{};

template <int A, int B, int N>
__device__ __forceinline__ int cmp_exchange(float (&s)[N]) {
  float mn = fminf(s[A], s[B]), mx = fmaxf(s[A], s[B]);
  s[A] = mn;
  s[B] = mx;
  return 0;
}

template <int N, int... Is>
__device__ __forceinline__ void sort_columns(float (&s)[N], std::integer_sequence<int, Is...>) {
  // comparator indices are template arguments: constants by construction
  int order[] = {0, cmp_exchange<kMergeExchange<N>.a[Is], kMergeExchange<N>.b[Is]>(s)...};
  (void)order;
}

template <int N>
__global__ void __launch_bounds__(NTHREADS)
k_col_trimmed_mean(const float *__restrict__ x, int P, int lo, int hi, float cnt,
                   float *__restrict__ out, long d, long stride) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long gstride = gridDim.x * (long)blockDim.x;
  for (; i < d; i += gstride) {
    float s[N];
    load_column(s, N, x, P, stride, i);
    sort_columns(s, std::make_integer_sequence<int, kMergeExchange<N>.n>{});
    // -0.0f + v == v bit for bit (v = -0.0f included), so the first kept rank needs
    // no case of its own
    float acc = -0.f;
#pragma unroll
    for (int r = 0; r < N; ++r)
      if (r >= lo && r < hi) acc += s[r];
    out[i] = acc / cnt;
  }
}

void column_trimmed_mean(torch::Tensor x, long lo, long hi, torch::Tensor out) {
  CHECK_IN(x); CHECK_IN(out);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 && out.scalar_type() == torch::kFloat32,
              "column_trimmed_mean: x and out must be fp32");
  TORCH_CHECK(x.dim() == 2, "column_trimmed_mean: x must be 2D");
  long P = x.size(0), d = x.size(1);
  TORCH_CHECK(P >= 1 && P <= 64, "column_trimmed_mean kernel supports 1 <= P <= 64, got ", P);
  TORCH_CHECK(0 <= lo && lo < hi && hi <= P,
              "column_trimmed_mean: need 0 <= lo < hi <= P, got lo=", lo, " hi=", hi, " P=", P);
  TORCH_CHECK(out.numel() == d, "column_trimmed_mean: out must have the length of a row of x");
  TORCH_CHECK(d % 4 == 0, "column_trimmed_mean: row length must be a multiple of 4");
  if (d == 0) return;
  dim3 grid(n_blocks(d, NTHREADS));
  const float *xp = x.data_ptr<float>();
  float *op = out.data_ptr<float>();
  float cnt = (float)(hi - lo);
  for_padded(P, [&](auto n) {
    launch(k_col_trimmed_mean<decltype(n)::value>, grid, 0, xp, (int)P, (int)lo, (int)hi, cnt,
           op, d, d);
  });
}

// --------------------------------------------------------------------------- mean around
// Mean around median ("MeaMed", Xie et al., arXiv:1802.10116) and Phocas
// (arXiv:1805.09682): per column, the mean of the `keep` values nearest to a robust
// centre c — the median (clo=(P-1)/2, chi=P/2+1) or the b-trimmed mean (clo=b,
// chi=P-b), b = P - keep.  Same layout, padding and register sort as
// k_col_trimmed_mean; c is that kernel's arithmetic on ranks [clo, chi).
//
// The `keep` nearest values of a sorted column are a contiguous window s[w, w+keep).
// Its start is a count, not a search:  w = #{ j < b : (c - s[j]) > (s[j+keep] - c) }
// (the predicate is monotone in j; a tie keeps the lower value, a NaN compares false).
// s[j + keep] has a run-time offset, and a run-time-indexed per-thread array goes to
// scratch, so t[j] = s[j + keep] is built by a barrel shifter: stage q moves every
// element down by 1<<q if bit q of keep is set — compile-time indices, wave-uniform
// conditions, registers only.  The window is then summed ascending with a per-lane
// select between acc and acc + s[r] (never "+ 0", which would turn a -0 result into
// +0), so the result is bit-identical to the CPU fallback.
// Steps 2-4 on a sorted column (centre, window start, window mean), shared by
// k_col_mean_around and k_seg_mean_around; P is the number of real rows in s[0..N).
template <int N>
__device__ __forceinline__ float mean_around_sorted(const float (&s)[N], int P, int keep, int clo,
                                                    int chi, float ccnt, float kcnt) {
  const int b = P - keep;
  float c = -0.f;
#pragma unroll
  for (int r = 0; r < N; ++r)
    if (r >= clo && r < chi) c += s[r];
  c = c / ccnt;
  // t[j] = s[j + keep] (+inf past the end: never compared, since j + keep < P for j < b)
  float t[N];
#pragma unroll
  for (int r = 0; r < N; ++r) t[r] = s[r];
#pragma unroll
  for (int q = 0; (1 << q) <= N; ++q) {
    if (keep & (1 << q)) {
#pragma unroll
      for (int r = 0; r < N; ++r) t[r] = (r + (1 << q) < N) ? t[r + (1 << q)] : INFINITY;
    }
  }
  int w = 0;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j < b) w += ((c - s[j]) > (t[j] - c)) ? 1 : 0;
  const int wend = w + keep;
  float acc = -0.f;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    float nxt = acc + s[r];
    acc = (r >= w && r < wend) ? nxt : acc;
  }
  return acc / kcnt;
}

template <int N>
__global__ void __launch_bounds__(NTHREADS)
k_col_mean_around(const float *__restrict__ x, int P, int keep, int clo, int chi,
                  float ccnt, float kcnt, float *__restrict__ out, long d, long stride) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long gstride = gridDim.x * (long)blockDim.x;
  for (; i < d; i += gstride) {
    float s[N];
    load_column(s, N, x, P, stride, i);
    sort_columns(s, std::make_integer_sequence<int, kMergeExchange<N>.n>{});
    out[i] = mean_around_sorted(s, P, keep, clo, chi, ccnt, kcnt);
  }
}

void column_mean_around(torch::Tensor x, long keep, long clo, long chi, torch::Tensor out) {
  CHECK_IN(x); CHECK_IN(out);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 && out.scalar_type() == torch::kFloat32,
              "column_mean_around: x and out must be fp32");
  TORCH_CHECK(x.dim() == 2, "column_mean_around: x must be 2D");
  long P = x.size(0), d = x.size(1);
  TORCH_CHECK(P >= 1 && P <= 64, "column_mean_around kernel supports 1 <= P <= 64, got ", P);
  TORCH_CHECK(1 <= keep && keep <= P,
              "column_mean_around: need 1 <= keep <= P, got keep=", keep, " P=", P);
  TORCH_CHECK(0 <= clo && clo < chi && chi <= P,
              "column_mean_around: need 0 <= clo < chi <= P, got clo=", clo, " chi=", chi,
              " P=", P);
  TORCH_CHECK(out.numel() == d, "column_mean_around: out must have the length of a row of x");
  TORCH_CHECK(d % 4 == 0, "column_mean_around: row length must be a multiple of 4");
  if (d == 0) return;
  dim3 grid(n_blocks(d, NTHREADS));
  const float *xp = x.data_ptr<float>();
  float *op = out.data_ptr<float>();
  float ccnt = (float)(chi - clo), kcnt = (float)keep;
  for_padded(P, [&](auto n) {
    launch(k_col_mean_around<decltype(n)::value>, grid, 0, xp, (int)P, (int)keep, (int)clo,
           (int)chi, ccnt, kcnt, op, d, d);
  });
}

// --------------------------------------------------------------------------- segment mean around
// Multi-Krum / Bulyan decode (arXiv:1703.02757 §4, arXiv:1802.07927): the Krum
// selection keeps T of the P rows PER SEGMENT (parameter tensor), and column j of
// segment l is k_col_mean_around's arithmetic over the T values x[sel[l][k]][j] —
// Multi-Krum: keep = T (plain mean); Bulyan: median centre, keep = T - 2f.
//
// Same layout as k_col_mean_around (one column per lane, grid cap, +inf padding to N,
// register sort, mean_around_sorted); new is where the rows come from.  Per column the
// segment is found by find_segment over the bounds staged in LDS ((L+1) longs, checked
// against the LDS limit by segment_lds on the host).  The (L, T) index table is
// NOT staged: L*T*8 bytes has no bound the host could promise (160 tensors x 64 rows is
// 80 KiB, which would also cost occupancy), it is a few KiB that every block re-reads,
// so it stays cache-resident and is read from global memory.  The register array s[] is
// still indexed by compile-time k only; the table is what is read at a run-time address.
// Every lane reads the table at its own segment's row (the lanes of a wave inside one
// segment read one address: a broadcast), so a wave that straddles a boundary simply
// gathers different rows per lane.  An unselected row is never read: a NaN there cannot
// reach the output (0/1 weights in k_seg_wmean could not promise that, fmaf(0, NaN, acc)
// is NaN).
//
// The gather loop has NO branch on k < T: a load behind a (wave-uniform) branch is
// waited for before the next branch, which chains the T row reads one latency after the
// other.  Padding slots k >= T re-read table entry T-1 — in bounds, the line already in
// cache — and are replaced by +inf in a select, so the N index loads and then the N row
// loads are in flight together.  Measured at d = 11.2M, 62 segments (stand-alone timing
// of both forms, equal outputs): T=22 611 -> 454 us, T=13 367 -> 240 us, T=33 (15
// padding slots) 1396 -> 1112 us.
//
// Every index read from the table is clamped into [0, P): bad sel contents give a
// wrong row, never an out-of-bounds read (the fallback clamps the same way).  The table
// address itself is in bounds for any seg contents, since the search result is in
// [0, L) and the slot in [0, T).  Columns outside [seg[0], seg[L]) get +0.0, so every
// element of out is written.
template <int N>
__device__ __forceinline__ void gather_column(float (&s)[N], const float *__restrict__ x,
                                              const long *__restrict__ row, int T, int P,
                                              long stride, long i) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    long r = row[k < T ? k : T - 1];
    r = r < 0 ? 0 : (r >= P ? (long)P - 1 : r);
    float v = x[r * stride + i];
    s[k] = (k < T && v == v) ? v : INFINITY;
  }
}

template <int N>
__global__ void __launch_bounds__(NTHREADS)
k_seg_mean_around(const float *__restrict__ x, const long *__restrict__ sel,
                  const long *__restrict__ seg, int L, int T, int P, int keep, int clo,
                  int chi, float ccnt, float kcnt, float *__restrict__ out, long d,
                  long stride) {
  extern __shared__ long s_seg[];
  stage_segments(s_seg, seg, L);
  __syncthreads();
  long gstride = gridDim.x * (long)blockDim.x;
  // base-indexed loop with a per-lane `valid` instead of `continue`: the sort stays in
  // one block of straight-line code that every lane of the wave runs (a lane outside
  // the segments sorts +inf and stores 0).  The form with an early `continue` per lane
  // compiles to a similar instruction mix but measured 711 us against 454 us at T=22
  // (266 against 240 us at T=13).
  for (long base = blockIdx.x * (long)blockDim.x; base < d; base += gstride) {
    long i = base + threadIdx.x;
    bool valid = (i < d) && in_segments(s_seg, L, i);
    int lo = 0;
    if (valid) lo = find_segment(s_seg, L, i);
    float s[N];
    if (valid) {
      gather_column(s, x, sel + (long)lo * T, T, P, stride, i);
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) s[k] = INFINITY;  // result unused
    }
    sort_columns(s, std::make_integer_sequence<int, kMergeExchange<N>.n>{});
    float r = mean_around_sorted(s, T, keep, clo, chi, ccnt, kcnt);
    if (i < d) out[i] = valid ? r : 0.f;
  }
}

void segment_mean_around(torch::Tensor x, torch::Tensor sel, torch::Tensor seg, long keep,
                         long clo, long chi, torch::Tensor out) {
  CHECK_IN(x); CHECK_IDX(sel); CHECK_IN(out);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 && out.scalar_type() == torch::kFloat32,
              "segment_mean_around: x and out must be fp32");
  TORCH_CHECK(x.dim() == 2, "segment_mean_around: x must be 2D");
  TORCH_CHECK(sel.dim() == 2, "segment_mean_around: sel must be 2D (L, T)");
  SegmentLds sl = segment_lds("segment_mean_around", seg, 0);
  long P = x.size(0), d = x.size(1), T = sel.size(1);
  long L = sl.L;
  TORCH_CHECK(sel.size(0) == L, "segment_mean_around: sel must have one row per segment, got ",
              sel.size(0), " rows for L=", L);
  TORCH_CHECK(T >= 1 && T <= 64, "segment_mean_around kernel supports 1 <= T <= 64, got ", T);
  TORCH_CHECK(T <= P, "segment_mean_around: need T <= P, got T=", T, " P=", P);
  TORCH_CHECK(1 <= keep && keep <= T,
              "segment_mean_around: need 1 <= keep <= T, got keep=", keep, " T=", T);
  TORCH_CHECK(0 <= clo && clo < chi && chi <= T,
              "segment_mean_around: need 0 <= clo < chi <= T, got clo=", clo, " chi=", chi,
              " T=", T);
  TORCH_CHECK(out.numel() == d, "segment_mean_around: out must have the length of a row of x");
  TORCH_CHECK(d % 4 == 0, "segment_mean_around: row length must be a multiple of 4");
  if (d == 0) return;
  dim3 grid(n_blocks(d, NTHREADS));
  const float *xp = x.data_ptr<float>();
  const long *sp = sel.data_ptr<long>();
  const long *gp = seg.data_ptr<long>();
  float *op = out.data_ptr<float>();
  float ccnt = (float)(chi - clo), kcnt = (float)keep;
  for_padded(T, [&](auto n) {
    launch(k_seg_mean_around<decltype(n)::value>, grid, sl.bytes, xp, sp, gp, sl.L, (int)T,
           (int)P, (int)keep, (int)clo, (int)chi, ccnt, kcnt, op, d, d);
  });
}

// --------------------------------------------------------------------------- collusion
// Colluding adversaries that see the honest gradients: ALIE ("A Little Is Enough",
// Baruch et al., arXiv:1902.06156: mu - z*sigma) and inner-product manipulation (Xie
// et al., arXiv:1903.03936: -eps*mu).  In place on the (P, d) block every rank holds
// after the all_to_all: per column, mu and the population sigma of the HONEST rows
// (those whose bit is clear in `mask`), and every row whose bit is set is overwritten
// with a*mu + b*sigma.  Honest rows are only read, Byzantine rows only written.
//
// Same padding as the column-sort kernels (honest values in registers indexed by
// compile-time constants only, N the smallest padded size >= P), but each lane owns
// FOUR adjacent columns and moves them as one 16-byte access (rows are 16-byte aligned:
// d % 4 == 0): at one column per lane and 4 B per access this kernel, with no sort at
// all, ran no faster than k_col_trimmed_mean (profiles/kernel_bw_collude.txt).  `mask`
// is wave-uniform, so the row tests are scalar branches: a Byzantine row costs no load,
// an honest row no store.  Two-pass variance (mu first, then the sum of (x - mu)^2,
// rows in ascending order): the one-pass E[x^2] - mu^2 form cancels and can go negative
// under the root.  SIGMA=false (b == 0, IPM) skips the second pass and the root.
typedef float col4 __attribute__((ext_vector_type(4)));

template <int N, bool SIGMA>
__global__ void __launch_bounds__(NTHREADS)
k_collude(float *x, int P, unsigned long long mask, float cnt, float a, float b, long d4,
          long stride) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long gstride = gridDim.x * (long)blockDim.x;
  for (; i < d4; i += gstride) {
    col4 s[N];
    col4 sum = 0.f;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      s[p] = 0.f;
      if (p < P && !((mask >> p) & 1ull)) {
        s[p] = *reinterpret_cast<const col4 *>(x + p * stride + 4 * i);
        sum += s[p];
      }
    }
    col4 mu = sum / cnt;
    col4 v = a * mu;
    if (SIGMA) {
      col4 ss = 0.f;
#pragma unroll
      for (int p = 0; p < N; ++p)
        if (p < P && !((mask >> p) & 1ull)) {
          col4 dev = s[p] - mu;
          ss += dev * dev;
        }
      ss = ss / cnt;
      v.x += b * sqrtf(ss.x);
      v.y += b * sqrtf(ss.y);
      v.z += b * sqrtf(ss.z);
      v.w += b * sqrtf(ss.w);
    }
#pragma unroll
    for (int p = 0; p < N; ++p)
      if (p < P && ((mask >> p) & 1ull)) *reinterpret_cast<col4 *>(x + p * stride + 4 * i) = v;
  }
}

void collude(torch::Tensor x, std::vector<int64_t> rows, double a, double b) {
  CHECK_IN(x);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32, "collude: x must be fp32");
  TORCH_CHECK(x.dim() == 2, "collude: x must be 2D");
  long P = x.size(0), d = x.size(1);
  TORCH_CHECK(P >= 2 && P <= 64, "collude kernel supports 2 <= P <= 64, got ", P);
  TORCH_CHECK(d % 4 == 0, "collude: row length must be a multiple of 4");
  unsigned long long mask = 0;
  for (int64_t r : rows) {
    TORCH_CHECK(0 <= r && r < P, "collude: row ", r, " outside [0, ", P, ")");
    unsigned long long bit = 1ull << r;
    TORCH_CHECK(!(mask & bit), "collude: row ", r, " listed twice");
    mask |= bit;
  }
  long h = P - (long)rows.size();
  TORCH_CHECK(h >= 1, "collude: all ", P, " rows are Byzantine, need at least one honest row");
  if (rows.empty() || d == 0) return;
  float *xp = x.data_ptr<float>();
  TORCH_CHECK((uintptr_t)xp % 16 == 0, "collude: x must be 16-byte aligned");
  long d4 = d / 4;
  dim3 grid(n_blocks(d4, NTHREADS));
  float cnt = (float)h, af = (float)a, bf = (float)b;
  for_padded(P, [&](auto n) {
    constexpr int N = decltype(n)::value;
    if (bf != 0.f)
      launch(k_collude<N, true>, grid, 0, xp, (int)P, mask, cnt, af, bf, d4, d);
    else
      launch(k_collude<N, false>, grid, 0, xp, (int)P, mask, cnt, af, bf, d4, d);
  });
}

// --------------------------------------------------------------------------- centered clipping
// One iteration of centered clipping (Karimireddy, He, Jaggi, arXiv:2012.10333) on the
// (P, n) block: per column v += sum over rows with w[p] != 0 of w[p] * (x[p] - v), rows
// in ascending order, and (DIST) d2[p] = sum over columns of (x[p] - v_new)^2 for EVERY
// row, which are the distances the caller turns into the next iteration's weights.  The
// column is read once and serves both halves from registers.
//
// Padding as in k_collude (N the smallest padded size >= P, compile-time indices only)
// and its wide layout: each lane owns CW adjacent columns.  CW = 4 (16-byte accesses)
// up to N = 32; N = 48 / 64 take CW = 2, because the N distance accumulators each lane
// carries across its grid-stride trips come on top of the N * CW column registers
// (profiles/kernel_bw_centered_clip.txt has the register counts).  `w` is wave-uniform:
// the row tests are scalar branches, a row with w[p] == 0 is never read by the update
// (not at all when !DIST), so a NaN there cannot reach v.  With every weight zero v is
// not written.
//
// The distances use no float atomics and a fixed order: lane accumulators over the
// lane's trips, xor-butterfly over the wave, the block's waves in ascending order
// through LDS, one row of the (gridDim, P) workspace per block, and k_clip_finish sums
// each workspace column in a fixed order.  The grid depends on n alone, so two runs on
// the same input agree bit for bit.
template <int CW> struct ColVec;
template <> struct ColVec<4> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct ColVec<2> { typedef float type __attribute__((ext_vector_type(2))); };

__device__ inline float col_sumsq(col4 d) {
  return d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
}
__device__ inline float col_sumsq(ColVec<2>::type d) { return d.x * d.x + d.y * d.y; }

template <int N, int CW, bool DIST>
__global__ void __launch_bounds__(NTHREADS)
k_clip_step(const float *__restrict__ x, float *__restrict__ v, const float *__restrict__ w,
            float *__restrict__ ws, int P, long nv, long stride) {
  typedef typename ColVec<CW>::type colv;
  __shared__ float part[NTHREADS / WAVE][N];
  float wr[N];
  bool any = false;
#pragma unroll
  for (int p = 0; p < N; ++p) {
    wr[p] = p < P ? w[p] : 0.f;
    any = any || wr[p] != 0.f;
  }
  float acc[N];
#pragma unroll
  for (int p = 0; p < N; ++p) acc[p] = 0.f;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long gstride = gridDim.x * (long)blockDim.x;
  for (; i < nv; i += gstride) {
    colv vv = *reinterpret_cast<const colv *>(v + CW * i);
    colv s[N];
    colv delta = 0.f;
    // loads first, with no use inside the row branches, so that they stay in flight
    // together (a use per branch waits for each load in turn)
#pragma unroll
    for (int p = 0; p < N; ++p) {
      s[p] = 0.f;
      if (p < P && (DIST || wr[p] != 0.f))
        s[p] = *reinterpret_cast<const colv *>(x + p * stride + CW * i);
    }
#pragma unroll
    for (int p = 0; p < N; ++p)
      if (wr[p] != 0.f) delta += wr[p] * (s[p] - vv);  // wr[p] == 0 for p >= P
    if (any) {
      vv += delta;
      *reinterpret_cast<colv *>(v + CW * i) = vv;
    }
    if (DIST) {
#pragma unroll
      for (int p = 0; p < N; ++p)
        if (p < P) acc[p] += col_sumsq(s[p] - vv);
    }
  }
  if (DIST) {
    int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      if (p < P) {
        float a = acc[p];
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, WAVE);
        if (lane == 0) part[wave][p] = a;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < P) {
      float a = part[0][threadIdx.x];
#pragma unroll
      for (int k = 1; k < NTHREADS / WAVE; ++k) a += part[k][threadIdx.x];
      ws[blockIdx.x * (long)P + threadIdx.x] = a;
    }
  }
}

// d2[p] = sum over the nb workspace rows of ws[b][p]: one block per p, thread t adds
// rows t, t + 256, ... in ascending order, then a fixed LDS tree over the 256 partials.
__global__ void __launch_bounds__(NTHREADS)
k_clip_finish(const float *__restrict__ ws, float *__restrict__ d2, int nb, int P) {
  __shared__ float red[NTHREADS];
  int p = blockIdx.x;
  float a = 0.f;
  for (int b = threadIdx.x; b < nb; b += NTHREADS) a += ws[b * (long)P + p];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = NTHREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) d2[p] = red[0];
}

c10::optional<torch::Tensor> clip_step(torch::Tensor x, torch::Tensor v, torch::Tensor w,
                                       bool dist) {
  CHECK_IN(x);
  CHECK_IN(v);
  CHECK_IN(w);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 && v.scalar_type() == torch::kFloat32 &&
                  w.scalar_type() == torch::kFloat32,
              "clip_step: x, v and w must be fp32");
  TORCH_CHECK(x.dim() == 2, "clip_step: x must be 2D");
  long P = x.size(0), n = x.size(1);
  TORCH_CHECK(P >= 1 && P <= 64, "clip_step kernel supports 1 <= P <= 64, got ", P);
  TORCH_CHECK(n % 4 == 0, "clip_step: row length must be a multiple of 4");
  TORCH_CHECK(v.dim() == 1 && v.size(0) == n, "clip_step: v must have shape (", n, ",)");
  TORCH_CHECK(w.dim() == 1 && w.size(0) == P, "clip_step: w must have shape (", P, ",)");
  TORCH_CHECK(v.device() == x.device() && w.device() == x.device(),
              "clip_step: v and w must be on x's device");
  c10::optional<torch::Tensor> out;
  if (dist) out = torch::zeros({P}, x.options());
  if (n == 0) return out;
  const float *xp = x.data_ptr<float>();
  float *vp = v.data_ptr<float>();
  TORCH_CHECK((uintptr_t)xp % 16 == 0 && (uintptr_t)vp % 16 == 0,
              "clip_step: x and v must be 16-byte aligned");
  const float *wp = w.data_ptr<float>();
  for_padded(P, [&](auto n_pad) {
    constexpr int N = decltype(n_pad)::value;
    constexpr int CW = N <= 32 ? 4 : 2;  // columns per lane, see k_clip_step's comment
    long nv = n / CW;
    int nb = n_blocks(nv, NTHREADS);
    if (dist) {
      torch::Tensor ws = torch::empty({(long)nb, P}, x.options());
      launch(k_clip_step<N, CW, true>, dim3(nb), 0, xp, vp, wp, ws.data_ptr<float>(), (int)P,
             nv, n);
      launch(k_clip_finish, dim3((int)P), 0, ws.data_ptr<float>(), out->data_ptr<float>(), nb,
             (int)P);
    } else {
      launch(k_clip_step<N, CW, false>, dim3(nb), 0, xp, vp, wp, nullptr, (int)P, nv, n);
    }
  });
  return out;
}

// --------------------------------------------------------------------------- worker momentum
// Worker-side momentum ("Learning from History for Byzantine Robust Optimization",
// arXiv:2012.10333): a logical worker sends m = beta*m + (1-beta)*g instead of g.  One
// pass over a payload row (or a bucket's slice of it) and the same span of the worker's
// state row: 8 B read + 8 B written per element, bandwidth-bound like k_sgd.  Per
// element and branch-free: a non-finite g (NaN, +-Inf) leaves m as it was and is sent
// as it is, so one overflowing step does not poison the state for the rest of the run.
// FIRST (the worker's first step): m = g bit for bit (0 where g is non-finite), g is
// sent unchanged, so m is never read and g never written.  Definition:
// fallback.worker_momentum_.
template <bool FIRST>
__global__ void __launch_bounds__(NTHREADS)
k_worker_momentum(float4 *__restrict__ g, float4 *__restrict__ m, long n4, float beta,
                  float omb /* 1-beta, formed in double on the host */) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = gridDim.x * (long)blockDim.x;
  for (; i < n4; i += stride) {
    float4 gv = g[i];
    float gg[4] = {gv.x, gv.y, gv.z, gv.w};
    float mm[4];
    if (FIRST) {
#pragma unroll
      for (int c = 0; c < 4; ++c) mm[c] = fabsf(gg[c]) < INFINITY ? gg[c] : 0.f;
      m[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
    } else {
      float4 mv = m[i];
      float old[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        bool fin = fabsf(gg[c]) < INFINITY;  // false for NaN and +-Inf
        float upd = fmaf(beta, old[c], omb * gg[c]);
        mm[c] = fin ? upd : old[c];
        gg[c] = fin ? upd : gg[c];
      }
      m[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
      g[i] = make_float4(gg[0], gg[1], gg[2], gg[3]);
    }
  }
}

void worker_momentum(torch::Tensor g, torch::Tensor m, double beta, bool first) {
  CHECK_IN(g);
  CHECK_IN(m);
  TORCH_CHECK(g.scalar_type() == torch::kFloat32 && m.scalar_type() == torch::kFloat32,
              "worker_momentum: g and m must be fp32");
  TORCH_CHECK(g.device() == m.device(), "worker_momentum: m must be on g's device");
  TORCH_CHECK(m.numel() == g.numel(), "worker_momentum: m must have g's length, got ",
              m.numel(), " and ", g.numel());
  TORCH_CHECK(g.numel() % 4 == 0, "worker_momentum: length must be a multiple of 4");
  TORCH_CHECK(beta >= 0.0 && beta < 1.0, "worker_momentum: beta must be in [0, 1), got ", beta);
  if (g.numel() == 0) return;
  float *gp = g.data_ptr<float>();
  float *mp = m.data_ptr<float>();
  TORCH_CHECK((uintptr_t)gp % 16 == 0 && (uintptr_t)mp % 16 == 0,
              "worker_momentum: g and m must be 16-byte aligned");
  long n4 = g.numel() / 4;
  int blocks = n_blocks(n4, NTHREADS);
  // 1-beta in double, then cast: 1.f - 0.99f is off by 2e-6 relative (see fused_adam_step)
  float omb = (float)(1.0 - beta);
  launch(first ? k_worker_momentum<true> : k_worker_momentum<false>, dim3(blocks), 0,
         (float4 *)gp, (float4 *)mp, n4, (float)beta, omb);
}

// --------------------------------------------------------------------------- module
void register_bn_ops(pybind11::module &m);  // bn_kernels.hip: fused BatchNorm+add+ReLU

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  register_bn_ops(m);
  m.def("fused_sgd_step", &fused_sgd_step);
  m.def("fused_adam_step", &fused_adam_step);
  m.def("inject", &inject);
  m.def("rows_equal", &rows_equal);
  m.def("pair_maxdiff", &pair_maxdiff);
  m.def("row_absmax", &row_absmax);
  m.def("mean_rows", &mean_rows);
  m.def("sum_rows", &sum_rows);
  m.def("cyclic_encode", &cyclic_encode);
  m.def("cyclic_project", &cyclic_project);
  m.def("combine_rows", &combine_rows);
  m.def("combine_rows_slice", &combine_rows_slice);
  m.def("cyclic_recombine", &cyclic_recombine);
  m.def("segment_absmax", &segment_absmax);
  m.def("segment_pair_maxdiff", &segment_pair_maxdiff);
  m.def("segment_sqdist", &segment_sqdist);
  m.def("segment_weighted_mean", &segment_weighted_mean);
  m.def("segment_gram", &segment_gram);
  m.def("column_trimmed_mean", &column_trimmed_mean);
  m.def("column_mean_around", &column_mean_around);
  m.def("segment_mean_around", &segment_mean_around);
  m.def("collude", &collude);
  m.def("clip_step", &clip_step);
  m.def("worker_momentum", &worker_momentum);
}
