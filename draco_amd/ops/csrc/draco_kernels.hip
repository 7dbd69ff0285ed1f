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
// same and carries per-row distance accumulators on top.  k_mix_rows (nearest-neighbour
// mixing, Y = W X in place) is the one kernel on the matrix unit (fp32 MFMA).
// k_sign_pack / k_sign_majority (signSGD with majority vote) are the bit kernels: wave
// ballots pack two sign bits per element, bit-sliced counters vote on 64 elements at once.
// k_mx8_pack / k_mx8_unpack (the MXFP8 block-scaled wire) convert with the gfx950 scaled
// FP8 instructions; the block scale is reduced across eight lanes by DPP.  k_mx8_col is
// the column sort on that wire: it reads the packed records, four columns per lane.
// k_mx8_seg_gram / k_mx8_seg_mean_around are Multi-Krum's and Bulyan's two steps on it: the
// Gram decodes a lane's MX block in registers and multiplies on the matrix unit.
// k_mx8_clip_step / k_mx8_weiszfeld are the iterative rules' passes (centered clipping, the
// geometric median) on it: codes packed in registers, each row decoded twice per pass.
// k_mx4_pack / k_mx4_unpack (the MXFP4 4-bit wire) use the scaled FP4 converts; a block is
// one quad of lanes, and the stochastic rounding is integer VALU work on a stateless hash.
// k_scatter_grads (the gradient sink) writes one backward's gradient tensors into the flat
// payload row in one pass; its tensor table travels by value in the kernel arguments.
//
// Build: hipcc --offload-arch=gfx950 (tools/build_ext.py); loaded as torch extension
// draco_amd._hip_ops.  No CUDA path, no hipify — HIP-native source.

#include <torch/extension.h>
#include <c10/hip/HIPException.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

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

// --------------------------------------------------------------------------- row mixing
// Y = W X in place on the (P, n) block, W a dense (P, P) fp32 matrix on device and rows
// in `skip` left out of the sum: y[i, c] = sum over k not in skip of w[i, k] * x[k, c].
// It is the heavy half of nearest-neighbour mixing (Allouah et al., "Fixing by Mixing",
// arXiv:2302.01772: every row becomes the mean of its P-f nearest rows) and the one
// kernel of this file on the matrix unit: at P = 32 a column costs 1024 FMAs for 256
// bytes moved, and a one-column-per-lane vector kernel would fetch a W operand for every
// one of them.  v_mfma_f32_32x32x2f32 keeps W, zero-padded to 32 x 32, in 16 registers
// per lane for the whole kernel.  No LDS, no second (P, n) buffer.
//
// A wave owns MIX_COLS = 128 consecutive columns per trip.  Lane (h = lane / 32,
// q = lane % 32) loads, for s = 0..15, the 16 bytes of row k = 2s + h at columns
// 4q..4q+3 (a half-wave reads 512 contiguous bytes of one row).  The instruction takes
// B[k = 2s + h][j = q] from lane (h, q): component t of those loads, across the lanes,
// is the B operand of column tile t, whose 32 columns are 4j + t.  Which columns form a
// tile is the kernel's choice, the instruction does not care.  A[i = q][k = 2s + h] =
// w[i, k] comes from the same lane numbering.  4 tiles x 16 steps accumulate into four
// 16-register tiles; register v of lane (h, q) holds row i = 8 (v / 4) + 4 h + v % 4 of
// column j = q, so the four tiles' registers v are that row's columns 4q..4q+3 again:
// one 16-byte store per (lane, v), 16 per lane, rows >= P not stored.
//
// Rows k >= P and rows in `skip` are never loaded; their B values AND their A values
// are zero (0 * 0, never 0 * NaN), so neither a NaN in a skipped row of x nor whatever w
// holds in that column reaches an output.  Steps whose two rows are both >= P are left
// out (P is wave-uniform).  Every store of a lane depends, through the accumulators, on
// every load of the wave's columns, and waves own disjoint columns, so in place is safe.
// Fixed order, no atomics: two runs agree bit for bit.
#define MIX_COLS 128
// the kernel's only fp32 arithmetic is the matrix instruction; the packed VALU forms
// (v_pk_add/mul/fma_f32) are switched off for it so that it stays that way
#if defined(__HIP_DEVICE_COMPILE__)
#define NO_PACKED_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define NO_PACKED_FP32
#endif
typedef float acc16 __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mix_rows(float *x, const float *__restrict__ w, int P, unsigned long long skip, long n) {
  const int lane = threadIdx.x % WAVE, h = lane / 32, q = lane % 32;
  float a[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    int k = 2 * s + h;
    a[s] = 0.f;
    if (q < P && k < P && !((skip >> k) & 1ull)) a[s] = w[q * P + k];
  }
  long chunks = (n + MIX_COLS - 1) / MIX_COLS;
  long c = blockIdx.x * (long)(NTHREADS / WAVE) + threadIdx.x / WAVE;
  long cstride = gridDim.x * (long)(NTHREADS / WAVE);
  for (; c < chunks; c += cstride) {  // wave-uniform trip count
    long col = c * MIX_COLS + 4 * q;
    bool in = col < n;  // n % 4 == 0: a float4 is inside or outside as a whole
    // rows h and 4h of the lane's columns: the row loaded in step s and the row stored
    // from register v lie a wave-uniform number of rows further on
    const float *xl = x + h * n + col;
    float *xs = x + 4 * h * n + col;
    col4 b[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      int k = 2 * s + h;
      b[s] = 0.f;
      if (in && k < P && !((skip >> k) & 1ull))
        b[s] = *reinterpret_cast<const col4 *>(xl + 2 * s * n);
    }
    acc16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (2 * s < P) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s][t], acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      int i = 8 * (v / 4) + 4 * h + v % 4;
      if (in && i < P) {
        col4 y = {acc[0][v], acc[1][v], acc[2][v], acc[3][v]};
        *reinterpret_cast<col4 *>(xs + (8 * (v / 4) + v % 4) * n) = y;
      }
    }
  }
}

void mix_rows(torch::Tensor x, torch::Tensor w, std::vector<int64_t> skip) {
  check_rows("mix_rows", x, true);
  CHECK_IN(w);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 && w.scalar_type() == torch::kFloat32,
              "mix_rows: x and w must be fp32");
  long P = x.size(0), n = x.size(1);
  TORCH_CHECK(P <= 32, "mix_rows kernel supports P <= 32 (one 32x32 matrix tile), got ", P);
  TORCH_CHECK(w.dim() == 2 && w.size(0) == P && w.size(1) == P, "mix_rows: w must have shape (",
              P, ", ", P, ")");
  TORCH_CHECK(w.device() == x.device(), "mix_rows: w must be on x's device");
  unsigned long long mask = 0;
  for (int64_t r : skip) {
    TORCH_CHECK(0 <= r && r < P, "mix_rows: skip row ", r, " outside [0, ", P, ")");
    unsigned long long bit = 1ull << r;
    TORCH_CHECK(!(mask & bit), "mix_rows: skip row ", r, " listed twice");
    mask |= bit;
  }
  if (P == 0 || n == 0) return;
  float *xp = x.data_ptr<float>();
  TORCH_CHECK((uintptr_t)xp % 16 == 0, "mix_rows: x must be 16-byte aligned");
  long chunks = (n + MIX_COLS - 1) / MIX_COLS;
  launch(k_mix_rows, dim3(n_blocks(chunks, NTHREADS / WAVE)), 0, xp, w.data_ptr<float>(), (int)P,
         mask, n);
}

// --------------------------------------------------------------------------- sign majority
// signSGD with majority vote (Bernstein et al., arXiv:1810.05291): a worker sends the sign
// of every gradient coordinate, the server takes the per-coordinate majority.  The vote of
// a value g is +1 (g > 0), -1 (g < 0) or 0 (abstain: +0.0, -0.0, NaN); +-Inf and
// subnormals vote their sign.  It is read off the bit pattern, never a float compare (no
// flush of subnormals) and never the raw sign bit (-0.0 and NaN abstain).
//
// PACKED FORMAT (the one description; fallback.sign_pack produces the same bytes).  Two
// bits per element, a `neg` plane and a `pos` plane.  Elements [64 r, 64 r + 64) form
// record r: four int32 words, 16 bytes, at words 4r .. 4r+3 of the packed row,
//     word 0 = neg bits 0..31, word 1 = neg bits 32..63,
//     word 2 = pos bits 0..31, word 3 = pos bits 32..63,
// and element e = 4 l + c of the record (l = 0..15, c = 0..3) is bit 16 c + l of its
// plane.  The bit of an element depends on its index alone, and records are whole and in
// order, so the packing of a 64-aligned slice of a row is the matching slice of the packed
// row: the even all_to_all split of a packed row lands every rank's shard (a multiple of
// 64 elements) on it.  The 16 c + l order is what four wave ballots over a float4 per lane
// give without a transpose: bits 16 k .. 16 k + 15 of ballot c are lanes 16 k .. 16 k + 15,
// the 16 float4s of the wave's k-th record.  A row with both bits of an element set (no
// sign_pack output has one) counts once for each side: it cancels itself and abstains.
//
// k_sign_pack: one streaming pass, 4 B read and 0.25 B written per element, no LDS, no
// atomics.  A wave owns SIGN_TRIP chunks of 256 consecutive elements per trip; all its
// float4 loads are issued first, then per chunk eight ballots (neg, pos for c = 0..3)
// executed by every lane, and lanes 0..3 assemble and store the chunk's four records, one
// 16-byte store each (64 contiguous bytes).  n % 64 == 0: a lane's float4 and a record are
// inside or outside as a whole; an outside lane votes 0 and an outside record is not
// stored, which is all that n % 256 in {64, 128, 192} needs.
#define SIGN_TRIP 4

__device__ __forceinline__ void sign_votes(unsigned u, bool &neg, bool &pos) {
  unsigned a = u & 0x7fffffffu;
  bool votes = a != 0u && a <= 0x7f800000u;  // not +-0, not NaN
  neg = votes && (u >> 31);
  pos = votes && !(u >> 31);
}

// integer work only; the packed fp32 VALU forms stay off as for k_mix_rows
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_sign_pack(const uint4 *__restrict__ g, int4 *__restrict__ out, long n) {
  const int lane = threadIdx.x % WAVE;
  long chunks = (n + 255) / 256, nrec = n / 64;
  long c = (blockIdx.x * (long)(NTHREADS / WAVE) + threadIdx.x / WAVE) * SIGN_TRIP;
  long cstride = gridDim.x * (long)(NTHREADS / WAVE) * SIGN_TRIP;
  for (; c < chunks; c += cstride) {  // wave-uniform trip count: every lane ballots
    uint4 v[SIGN_TRIP];
#pragma unroll
    for (int j = 0; j < SIGN_TRIP; ++j) {
      long i4 = (c + j) * 64 + lane;  // the lane's float4
      v[j] = make_uint4(0u, 0u, 0u, 0u);
      if (i4 * 4 < n) v[j] = g[i4];
    }
#pragma unroll
    for (int j = 0; j < SIGN_TRIP; ++j) {
      unsigned u[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
      unsigned long long bn[4], bp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        bool neg, pos;
        sign_votes(u[k], neg, pos);
        bn[k] = __builtin_amdgcn_ballot_w64(neg);
        bp[k] = __builtin_amdgcn_ballot_w64(pos);
      }
      // lane k < 4: record k of the chunk is bits 16k .. 16k+15 of the eight ballots
      int sh = 16 * (lane & 3);
      unsigned w[4];
      w[0] = (unsigned)((bn[0] >> sh) & 0xffffu) | (unsigned)((bn[1] >> sh) & 0xffffu) << 16;
      w[1] = (unsigned)((bn[2] >> sh) & 0xffffu) | (unsigned)((bn[3] >> sh) & 0xffffu) << 16;
      w[2] = (unsigned)((bp[0] >> sh) & 0xffffu) | (unsigned)((bp[1] >> sh) & 0xffffu) << 16;
      w[3] = (unsigned)((bp[2] >> sh) & 0xffffu) | (unsigned)((bp[3] >> sh) & 0xffffu) << 16;
      long rec = (c + j) * 4 + lane;
      if (lane < 4 && rec < nrec) out[rec] = make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]);
    }
  }
}

// the checks shared by sign_pack and sign_majority: values (n,) fp32 and rows of n/16 int32
static inline void check_sign(const char *op, const torch::Tensor &vals, const torch::Tensor &bits,
                              long n) {
  CHECK_IN(vals);
  CHECK_IN(bits);
  TORCH_CHECK(vals.device() == bits.device(), op, ": tensors must be on one device");
  TORCH_CHECK(vals.scalar_type() == torch::kFloat32, op, ": values must be fp32");
  TORCH_CHECK(bits.scalar_type() == torch::kInt32, op, ": packed signs must be int32");
  TORCH_CHECK(vals.dim() == 1 && vals.numel() == n, op, ": values must be 1D of length ", n);
  TORCH_CHECK(n % 64 == 0, op, ": length must be a multiple of 64, got ", n);
}

void sign_pack(torch::Tensor g, torch::Tensor out) {
  long n = g.numel();
  check_sign("sign_pack", g, out, n);
  TORCH_CHECK(out.dim() == 1 && out.numel() == n / 16, "sign_pack: out must be 1D of length ",
              n / 16, ", got ", out.numel());
  if (n == 0) return;
  const float *gp = g.data_ptr<float>();
  int *op = out.data_ptr<int>();
  TORCH_CHECK((uintptr_t)gp % 16 == 0 && (uintptr_t)op % 16 == 0,
              "sign_pack: g and out must be 16-byte aligned");
  long chunks = (n + 255) / 256;
  int blocks = n_blocks((chunks + SIGN_TRIP - 1) / SIGN_TRIP, NTHREADS / WAVE);
  launch(k_sign_pack, dim3(blocks), 0, (const uint4 *)gp, (int4 *)op, n);
}

// k_sign_majority: out[j] = sign(#pos_j - #neg_j) over the P packed rows, in {-1, +0, +1},
// bit-sliced.  A lane owns one record (64 elements) per trip, a block 256 consecutive ones.
// Per row the lane reads its record with one 16-byte load (a wave reads 1 KB contiguous;
// four rows in flight) and adds the two 64-bit planes into two vertical counters of NB
// bit-planes each (NB = bits of P, at most 7: counts reach 64) with a ripple add: per plane
// an AND for the carry and an XOR, 64 elements at once.  A bit-sliced compare from the top
// plane down then gives the masks pos > neg and neg > pos.
//
// The store is coalesced through LDS: every lane parks its two masks (16 B), and in step
// s = 0..15 lane L fetches the masks of its wave's record 4 s + L / 16 (one 16-byte LDS
// read, four distinct addresses per wave) and writes that record's elements
// 4 (L % 16) .. + 3 as one float4, so a wave stores 1 KB of consecutive floats per step.  The
// trip count is uniform over the block (the two __syncthreads()).  Fixed order, no
// atomics: two runs agree bit for bit.  Ties, all-abstain columns and the zero pad tail
// give +0.0; the result is always finite.
template <int NB>
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_sign_majority(const int4 *__restrict__ packed, float4 *__restrict__ out, int P, long R) {
  typedef unsigned long long u64;
  __shared__ ulonglong2 s_mask[NTHREADS];
  const int tid = threadIdx.x, lane = tid % WAVE, wave0 = tid - lane;
  for (long base = blockIdx.x * (long)NTHREADS; base < R; base += gridDim.x * (long)NTHREADS) {
    long r = base + tid;
    bool in = r < R;
    u64 cn[NB], cp[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) cn[k] = cp[k] = 0ull;
    for (int p0 = 0; p0 < P; p0 += 4) {
      int4 w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = make_int4(0, 0, 0, 0);
        if (in && p0 + j < P) w[j] = packed[(long)(p0 + j) * R + r];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        u64 carry_n = (u64)(unsigned)w[j].x | (u64)(unsigned)w[j].y << 32;
        u64 carry_p = (u64)(unsigned)w[j].z | (u64)(unsigned)w[j].w << 32;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          u64 tn = cn[k] & carry_n, tp = cp[k] & carry_p;
          cn[k] ^= carry_n;
          cp[k] ^= carry_p;
          carry_n = tn;
          carry_p = tp;
        }
      }
    }
    u64 gt = 0ull, lt = 0ull, eq = ~0ull;
#pragma unroll
    for (int k = NB - 1; k >= 0; --k) {
      gt |= eq & cp[k] & ~cn[k];
      lt |= eq & cn[k] & ~cp[k];
      eq &= ~(cp[k] ^ cn[k]);
    }
    s_mask[tid] = make_ulonglong2(gt, lt);
    __syncthreads();
    const int l = lane % 16;
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      int src = 4 * s + lane / 16;
      long rec = base + wave0 + src;
      ulonglong2 m = s_mask[wave0 + src];
      unsigned f[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        unsigned g1 = (unsigned)(m.x >> (16 * c + l)) & 1u;
        unsigned l1 = (unsigned)(m.y >> (16 * c + l)) & 1u;
        f[c] = (g1 | l1) * 0x3f800000u | l1 << 31;  // gt and lt are disjoint
      }
      if (rec < R)
        out[rec * 16 + l] = make_float4(__uint_as_float(f[0]), __uint_as_float(f[1]),
                                        __uint_as_float(f[2]), __uint_as_float(f[3]));
    }
    __syncthreads();  // the next trip overwrites s_mask
  }
}

void sign_majority(torch::Tensor packed, torch::Tensor out) {
  long n = out.numel();
  check_sign("sign_majority", out, packed, n);
  TORCH_CHECK(packed.dim() == 2 && packed.size(1) == n / 16,
              "sign_majority: packed must be (P, ", n / 16, "), one row of n/16 words per worker");
  long P = packed.size(0), R = n / 64;
  TORCH_CHECK(P <= 64, "sign_majority kernel supports P <= 64 (7 counter planes), got ", P);
  if (n == 0 || P == 0) return;  // no launch; with no rows out is left as it is
  const int *pp = packed.data_ptr<int>();
  float *op = out.data_ptr<float>();
  TORCH_CHECK((uintptr_t)pp % 16 == 0 && (uintptr_t)op % 16 == 0,
              "sign_majority: packed and out must be 16-byte aligned");
  int nb = 1;
  while ((1L << nb) <= P) ++nb;  // counts 0..P need nb = bits of P planes
  auto run = [&](auto planes) {
    launch(k_sign_majority<decltype(planes)::value>, dim3(n_blocks(R, NTHREADS)), 0,
           (const int4 *)pp, (float4 *)op, (int)P, R);
  };
  switch (nb) {
    case 1: run(std::integral_constant<int, 1>{}); break;
    case 2: run(std::integral_constant<int, 2>{}); break;
    case 3: run(std::integral_constant<int, 3>{}); break;
    case 4: run(std::integral_constant<int, 4>{}); break;
    case 5: run(std::integral_constant<int, 5>{}); break;
    case 6: run(std::integral_constant<int, 6>{}); break;
    default: run(std::integral_constant<int, 7>{}); break;
  }
}

// --------------------------------------------------------------------------- mx8 wire
// An 8-bit block-scaled wire format for gradient rows: OCP Microscaling MXFP8, E4M3
// elements with one E8M0 scale per 32 elements.  Unlike the sign wire it keeps magnitudes:
// it decodes to an ordinary fp32 block, so every rule reads it unchanged.
//
// WIRE FORMAT (the one description; fallback.mx8_pack / mx8_unpack produce the same bytes).
// Element code: one byte, OCP FP8 E4M3 ("e4m3fn"): 1 sign, 4 exponent (bias 7), 3 mantissa
// bits; no infinities, 0x7F / 0xFF are NaN, the largest magnitude is 448 (0x7E),
// subnormals step by 2^-9.  Block: 32 consecutive elements of a row share a scale byte s,
// an E8M0 exponent meaning 2^(s-127); s = 0xFF is NaN for the whole block.
//   Encoding a block: amax = the largest |x| over its FINITE elements; e = the smallest
// integer with amax / 2^e <= 448, read off amax's bits: e = exponent(amax) - 8, plus 1 if the
// mantissa field exceeds 0x600000 (448 = 1.75 * 2^8); e is clamped to >= -117 (also taken
// when no element is finite or amax = 0) and s = e + 127, so an encoder emits s in
// [10, 247].  A finite element becomes the code nearest to x / 2^e, ties to the even code,
// with x's sign bit (-0.0 and values that round to zero keep it); by the choice of e nothing
// saturates.  NaN, +Inf and -Inf become the NaN code 0x7F with the element's sign bit and
// do not influence the scale.
//   Decoding: s = 0xFF gives NaN for the whole block; otherwise s is clamped to >= 10 and
// value = code value * 2^(s-127) in fp32, NaN codes giving NaN.  With the clamp every
// finite non-zero result is a normal fp32 number (2^-9 * 2^-117 = 2^-126), so flushing
// denormals changes nothing; an overflowing product (s >= 247 with large codes) is +-Inf.
// Every byte pattern decodes to an fp32 value, NaN or +-Inf.
//   Packed row: a row of n elements is packed against a chunk (the shard length) with
// n % chunk == 0 and chunk % 64 == 0, into n / chunk records of
// chunk_bytes = chunk + round_up(chunk / 32, 16) bytes: the chunk code bytes, the chunk / 32
// scale bytes, zero padding.  Records and scale runs start 16-byte aligned, a record
// depends on its chunk's elements alone, and the even all_to_all split of a packed row
// lands each rank's codes and scales on it.
//   Error: for finite x in a block of scale X = 2^e, |decode(encode(x)) - x| <=
// max(2^-4 |x|, 2^-10 X), and X < amax / 224.
//
// The gfx950 scaled converts (v_cvt_scalef32_pk_fp8_f32 / v_cvt_scalef32_pk_f32_fp8) do the
// element work.  Measured once on the MI355X with a stand-alone probe program that is not in
// the tree (the exact tests of tests/test_mx8_gpu.py are what stays), against the integer
// statement of the format, over every fp32 bit pattern that is in range for scales 10, 11,
// 60, 127, 200, 246, 247 and
// over every (code, scale) pair: the encode gives the format's byte for every finite input
// (nearest, ties to even, fp32 subnormal inputs honoured, FP8 subnormal outputs produced,
// sign of zero kept); for NaN it does not keep the sign bit (+NaN came out as 0xFF), so
// non-finite elements are patched with an integer select; the decode is exact for all 256
// codes at every scale 10..254, NaN codes and the overflow to +-Inf included.  The scale
// operand is the fp32 number 2^(s-127), always normal here.  Out-of-range inputs are never
// converted, so what the instruction does with them is not relied on.
//
// Both kernels walk "units": a unit is one wave-wide load of 256 consecutive elements of one
// record (a float4, or a dword of codes, per lane), MX8_TRIP units per wave per trip with
// all loads issued before any conversion.  chunk % 64 == 0: a lane's four elements and a
// 32-element block (eight adjacent lanes) are inside or outside the record as a whole.
#define MX8_TRIP 4
typedef short mx8_v2s __attribute__((ext_vector_type(2)));
typedef float mx8_v2f __attribute__((ext_vector_type(2)));

static inline long mx8_chunk_bytes(long chunk) { return chunk + (chunk / 32 + 15) / 16 * 16; }

// max over the eight lanes of a block, in every one of them: two quad permutes and a mirror
// of the 8-lane half row, on the VALU's data path (no LDS, no ds_bpermute)
__device__ __forceinline__ unsigned mx8_block_max(unsigned v) {
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));   // lane ^ 1
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));   // lane ^ 2
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));  // 7 - lane
  return v;
}

// k_mx8_pack: one streaming pass, 4 B read and ~1.03 B written per element, no LDS, no
// atomics.  Per unit: the finite amax of a lane's float4 (integer max of the magnitude
// bits), the block max by DPP, the scale byte from amax's exponent and mantissa fields, two
// scaled converts for the lane's dword of codes (a wave stores 256 contiguous bytes).  The
// eight scale bytes of a unit are collected from lanes 0, 8, .., 56 with v_readlane into two
// dwords, and lane 0 stores them as one 8-byte vector; an outside block contributes 0, which
// is the record's padding, and the unit that ends a record with an odd unit count also
// writes the 8 zero bytes that complete the padded scale run (round_up(chunk/32, 16)).
// The loop's trip count is wave-uniform: every lane runs the DPP and readlane steps.
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mx8_pack(const uint4 *__restrict__ g, unsigned char *__restrict__ out, long chunk, long cbytes,
           int upr, int units) {
  const int lane = threadIdx.x % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  long u0 = (blockIdx.x * (long)(NTHREADS / WAVE) + wave) * MX8_TRIP;
  long ustride = gridDim.x * (long)(NTHREADS / WAVE) * MX8_TRIP;
  for (; u0 < units; u0 += ustride) {
    // u0 < units fits an int (checked on the host): a 32-bit division, once per trip
    const int u = (int)u0;
    int r = u / upr, j = u - r * upr;  // record, unit of the record
    uint4 v[MX8_TRIP];
    long base[MX8_TRIP];  // byte offset of the unit's record; -1: no such unit
    int uj[MX8_TRIP];
#pragma unroll
    for (int t = 0; t < MX8_TRIP; ++t) {
      long o = (long)j * 256 + 4 * lane;  // the lane's first element in the record
      base[t] = u0 + t < units ? r * cbytes : -1;
      uj[t] = j;
      v[t] = make_uint4(0u, 0u, 0u, 0u);
      if (base[t] >= 0 && o < chunk) v[t] = g[(r * chunk + o) / 4];
      if (++j == upr) { j = 0; ++r; }
    }
#pragma unroll
    for (int t = 0; t < MX8_TRIP; ++t) {
      long o = (long)uj[t] * 256 + 4 * lane;
      bool in = base[t] >= 0 && o < chunk;
      unsigned x[4] = {v[t].x, v[t].y, v[t].z, v[t].w};
      unsigned amax = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned a = x[k] & 0x7fffffffu;
        amax = max(amax, a < 0x7f800000u ? a : 0u);
      }
      amax = mx8_block_max(amax);
      int s = (int)(amax >> 23) - 8 + ((amax & 0x7fffffu) > 0x600000u);
      s = max(s, 10);
      float scale = __uint_as_float((unsigned)s << 23);
      mx8_v2s w = {0, 0};
      w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, __uint_as_float(x[0]), __uint_as_float(x[1]),
                                                   scale, false);
      w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, __uint_as_float(x[2]), __uint_as_float(x[3]),
                                                   scale, true);
      unsigned codes = __builtin_bit_cast(unsigned, w);
#pragma unroll
      for (int k = 0; k < 4; ++k)  // NaN, +-Inf: the NaN code with the element's sign
        if ((x[k] & 0x7fffffffu) >= 0x7f800000u)
          codes = (codes & ~(0xffu << (8 * k))) | ((0x7fu | (x[k] >> 24 & 0x80u)) << (8 * k));
      if (in) *reinterpret_cast<unsigned *>(out + base[t] + o) = codes;
      int sb = in ? s : 0;
      unsigned lo = 0u, hi = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lo |= (unsigned)__builtin_amdgcn_readlane(sb, 8 * k) << (8 * k);
        hi |= (unsigned)__builtin_amdgcn_readlane(sb, 32 + 8 * k) << (8 * k);
      }
      if (lane == 0 && base[t] >= 0) {
        unsigned char *sp = out + base[t] + chunk + 8L * uj[t];
        *reinterpret_cast<uint2 *>(sp) = make_uint2(lo, hi);
        if (uj[t] == upr - 1 && (upr & 1)) *reinterpret_cast<uint2 *>(sp + 8) = make_uint2(0u, 0u);
      }
    }
  }
}

// k_mx8_unpack: 1 B read and 4 B written per element.  A unit is 256 codes of one packed
// row: a lane reads its dword of codes (256 contiguous bytes per wave) and its block's scale
// byte (one byte shared by eight lanes, a cached byte load), converts with two scaled
// converts and writes one float4 (1 KB contiguous per wave).  The rows are flattened into
// the unit index.  No cross-lane step, so an outside lane simply skips.
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mx8_unpack(const unsigned char *__restrict__ packed, float4 *__restrict__ out, long chunk,
             long cbytes, int upr, int units) {
  const int lane = threadIdx.x % WAVE;
  long u0 = (blockIdx.x * (long)(NTHREADS / WAVE) + threadIdx.x / WAVE) * MX8_TRIP;
  long ustride = gridDim.x * (long)(NTHREADS / WAVE) * MX8_TRIP;
  for (; u0 < units; u0 += ustride) {
    const int u = (int)u0;  // as in k_mx8_pack
    int r = u / upr, j = u - r * upr;
    unsigned codes[MX8_TRIP], sbyte[MX8_TRIP];
    long dst[MX8_TRIP];  // float4 index in out; -1: nothing to do
#pragma unroll
    for (int t = 0; t < MX8_TRIP; ++t) {
      long o = (long)j * 256 + 4 * lane;
      bool in = u0 + t < units && o < chunk;
      dst[t] = in ? (r * chunk + o) / 4 : -1;
      codes[t] = sbyte[t] = 0u;
      if (in) {
        const unsigned char *rec = packed + r * cbytes;
        codes[t] = *reinterpret_cast<const unsigned *>(rec + o);
        sbyte[t] = rec[chunk + o / 32];
      }
      if (++j == upr) { j = 0; ++r; }
    }
#pragma unroll
    for (int t = 0; t < MX8_TRIP; ++t) {
      float scale = __uint_as_float(max(sbyte[t], 10u) << 23);
      mx8_v2f a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(codes[t], scale, false);
      mx8_v2f b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(codes[t], scale, true);
      float4 y = make_float4(a.x, a.y, b.x, b.y);
      if (sbyte[t] == 0xffu) y.x = y.y = y.z = y.w = __uint_as_float(0x7fc00000u);
      if (dst[t] >= 0) out[dst[t]] = y;
    }
  }
}

// the checks shared by the pack and unpack ops of the block-scaled wires (mx8 and mx4):
// `records` records of `cbytes` bytes for `chunk` elements each, walked in units (wave loads)
// of `unit` elements, `trip` of them per wave per trip; returns the units of the call
static inline int check_mx(const char *op, const torch::Tensor &vals, const torch::Tensor &bytes,
                           long chunk, long records, long cbytes, long unit, long trip) {
  CHECK_IN(vals);
  CHECK_IN(bytes);
  TORCH_CHECK(vals.device() == bytes.device(), op, ": tensors must be on one device");
  TORCH_CHECK(vals.scalar_type() == torch::kFloat32, op, ": values must be fp32");
  TORCH_CHECK(bytes.scalar_type() == torch::kUInt8, op, ": packed data must be uint8");
  TORCH_CHECK(chunk >= 0 && chunk % 64 == 0, op, ": chunk must be a multiple of 64, got ", chunk);
  TORCH_CHECK(vals.numel() == records * chunk, op, ": values must hold ", records, " x ", chunk,
              " elements, got ", vals.numel());
  TORCH_CHECK(bytes.numel() == records * cbytes, op, ": packed data must hold ",
              records, " records of ", cbytes, " bytes, got ", bytes.numel());
  TORCH_CHECK((uintptr_t)vals.data_ptr() % 16 == 0 && (uintptr_t)bytes.data_ptr() % 16 == 0, op,
              ": tensors must be 16-byte aligned");
  long units = records * ((chunk + unit - 1) / unit);
  TORCH_CHECK(units <= 0x7fffffffL - trip, op, ": ", units, " wave loads exceed the 32-bit unit index");
  return (int)units;
}

static inline int check_mx8(const char *op, const torch::Tensor &vals, const torch::Tensor &bytes,
                            long chunk, long records) {
  return check_mx(op, vals, bytes, chunk, records, mx8_chunk_bytes(chunk), 256, MX8_TRIP);
}

void mx8_pack(torch::Tensor g, torch::Tensor out, long chunk) {
  long n = g.numel();
  TORCH_CHECK(g.dim() == 1 && out.dim() == 1, "mx8_pack: g and out must be 1D");
  TORCH_CHECK(chunk > 0 ? n % chunk == 0 : n == 0, "mx8_pack: length ", n,
              " is not a multiple of chunk ", chunk);
  int units = check_mx8("mx8_pack", g, out, chunk, chunk > 0 ? n / chunk : 0);
  if (units == 0) return;
  int upr = (int)((chunk + 255) / 256);
  int blocks = n_blocks((units + MX8_TRIP - 1) / MX8_TRIP, NTHREADS / WAVE);
  launch(k_mx8_pack, dim3(blocks), 0, (const uint4 *)g.data_ptr<float>(), out.data_ptr<uint8_t>(),
         chunk, mx8_chunk_bytes(chunk), upr, units);
}

void mx8_unpack(torch::Tensor packed, torch::Tensor out) {
  TORCH_CHECK(packed.dim() == 2 && out.dim() == 2 && packed.size(0) == out.size(0),
              "mx8_unpack: packed must be (P, chunk_bytes) and out (P, chunk)");
  long P = out.size(0), chunk = out.size(1);
  int units = check_mx8("mx8_unpack", out, packed, chunk, P);
  TORCH_CHECK(packed.size(1) == mx8_chunk_bytes(chunk), "mx8_unpack: packed rows must have ",
              mx8_chunk_bytes(chunk), " bytes for chunk ", chunk, ", got ", packed.size(1));
  if (units == 0) return;  // P = 0 or chunk = 0: no launch
  int upr = (int)((chunk + 255) / 256);
  int blocks = n_blocks((units + MX8_TRIP - 1) / MX8_TRIP, NTHREADS / WAVE);
  launch(k_mx8_unpack, dim3(blocks), 0, packed.data_ptr<uint8_t>(), (float4 *)out.data_ptr<float>(),
         chunk, mx8_chunk_bytes(chunk), upr, units);
}

// --------------------------------------------------------------------------- mx8 column rules
// mx8_column_trimmed_mean / mx8_column_mean_around: mx8_unpack followed by
// column_trimmed_mean / column_mean_around, bit for bit, in one launch that reads the packed
// records themselves: ~1.03 B per row and column instead of 1 B + 4 B written + 4 B read back,
// and no (P, chunk) fp32 block anywhere.
//
// Work split.  A wave walks units of 256 consecutive columns (grid-stride over units, one
// unit per wave per trip); a lane owns the FOUR adjacent columns 4*lane .. 4*lane+3 and per
// row loads one dword of codes, 256 contiguous bytes per wave: a quarter of the load
// instructions per column of k_col_trimmed_mean, whose layout and not whose sort bounds it.
// The four columns lie in one 32-element block, so one scale per row serves them; it is
// fetched as a per-lane byte load, as k_mx8_unpack does (eight lanes read the same byte, 8
// contiguous bytes per wave and row: one cache line, no select by lane / 8 afterwards).  The
// row base is wave-uniform and the lane offset 32-bit (checked on the host).  All P code
// loads and all P scale loads of a unit are issued before the first conversion, behind the
// same wave-uniform `p < P` tests as load_column's.
//
// Registers.  The codes stay packed: N dwords, and N scales.  Once the loads are in, a row's
// scale byte becomes the fp32 operand 2^(max(s,10)-127) in place, and a NaN block (s = 0xFF)
// is folded into the codes (all four become the NaN code), so the per-column work is the
// convert and the NaN -> +inf select alone.  COLS columns are live at a time: one
// v_cvt_scalef32_pk_f32_fp8 of the low half yields two columns, both are sorted and reduced
// (sort_columns and mean_around_sorted, unchanged), then the codes shift down by 16 bits and
// the loop runs again.  The loop is NOT unrolled: the convert's half select is an immediate,
// so shifting the codes is what lets one copy of the sort network serve all four columns, and
// the results rotate through a float4 (no run-time-indexed array).  COLS = 1 is the same
// loop four times over one column with 8-bit shifts, for the padded sizes at which two
// columns beside codes and scales do not fit (see mx8_cols).  s[] is indexed by compile-time
// constants only; no instantiation uses scratch (profiles/kernel_bw_mx8_fused.txt).
//
// Output: one float4 per lane, 1 KB contiguous per wave.  chunk % 64 == 0, so a lane's four
// columns are inside the record or outside as a whole; there is no cross-lane step, no LDS
// and no atomics, so an outside lane of the unit that ends the shard simply skips.
template <int N> constexpr int mx8_cols = N <= 32 ? 2 : 1;

// ranks [lo, hi) of a sorted column, k_col_trimmed_mean's arithmetic
template <int N>
__device__ __forceinline__ float trimmed_sorted(const float (&s)[N], int lo, int hi, float cnt) {
  float acc = -0.f;
#pragma unroll
  for (int r = 0; r < N; ++r)
    if (r >= lo && r < hi) acc += s[r];
  return acc / cnt;
}

// AROUND: (a, b, c) = (keep, clo, chi), (f, g) = (ccnt, kcnt); else (a, b) = (lo, hi), f = cnt
template <int N, int COLS, bool AROUND>
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mx8_col(const unsigned char *__restrict__ packed, int P, int a, int b, int c, float f, float g,
          float4 *__restrict__ out, unsigned chunk, long cbytes, int units) {
  const int lane = threadIdx.x % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const int ustride = gridDim.x * (NTHREADS / WAVE);
  constexpr bool PACK = COLS == 1;  // scale exponents four to a register
  for (int u = blockIdx.x * (NTHREADS / WAVE) + wave; u < units; u += ustride) {
    const unsigned o = (unsigned)u * 256u + 4u * lane;  // the lane's first column
    if (o >= chunk) continue;
    const unsigned so = chunk + o / 32;  // its block's scale byte
    unsigned codes[N], sb[N];
#pragma unroll
    for (int p = 0; p < N; ++p) {
      codes[p] = sb[p] = 0u;
      if (p < P) {
        const unsigned char *rec = packed + p * cbytes;
        codes[p] = *reinterpret_cast<const unsigned *>(rec + o);
        sb[p] = rec[so];
      }
    }
    unsigned sc[PACK ? N / 4 : N] = {};
#pragma unroll
    for (int p = 0; p < N; ++p) {
      bool nan_block = sb[p] == 0xffu;
      codes[p] = nan_block ? 0x7f7f7f7fu : codes[p];
      unsigned e = nan_block ? 127u : max(sb[p], 10u);
      if constexpr (PACK) sc[p / 4] |= e << (8 * (p % 4));
      else sc[p] = e << 23;
    }
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int k = 0; k < 4 / COLS; ++k) {
      float s[COLS][N];
      if constexpr (PACK) {
        // the unpacked scales are loop-invariant; an empty asm keeps the compiler from
        // hoisting all N of them out of the loop, back into N registers
#pragma unroll
        for (int p = 0; p < N / 4; ++p) asm volatile("" : "+v"(sc[p]));
      }
#pragma unroll
      for (int p = 0; p < N; ++p) {
        unsigned scale = PACK ? (sc[p / 4] >> (8 * (p % 4)) & 0xffu) << 23 : sc[p];
        mx8_v2f v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(codes[p], __uint_as_float(scale), false);
        codes[p] >>= 8 * COLS;
        s[0][p] = (p >= P || v.x != v.x) ? INFINITY : v.x;
        if constexpr (COLS == 2) s[1][p] = (p >= P || v.y != v.y) ? INFINITY : v.y;
      }
      float r[COLS];
#pragma unroll
      for (int q = 0; q < COLS; ++q) {
        sort_columns(s[q], std::make_integer_sequence<int, kMergeExchange<N>.n>{});
        r[q] = AROUND ? mean_around_sorted(s[q], P, a, b, c, f, g) : trimmed_sorted(s[q], a, b, f);
      }
      // the results move down one place per new column: after the last trip y holds
      // columns 0..3 in x..w
      if constexpr (COLS == 2) y = make_float4(y.z, y.w, r[0], r[1]);
      else y = make_float4(y.y, y.z, y.w, r[0]);
    }
    out[o / 4] = y;
  }
}

// The checks shared by the column ops of both block-scaled wires, before any launch; returns
// the units (wave loads of `unit` columns) of the call.  With chunk <= 2^30 every column and
// every byte offset inside a record fits 32 bits, the last unit's outside lanes included.
static inline int check_mx_col(const char *op, const torch::Tensor &packed,
                               const torch::Tensor &out, long (*chunk_bytes)(long), long unit) {
  CHECK_IN(packed);
  CHECK_IN(out);
  TORCH_CHECK(packed.device() == out.device(), op, ": tensors must be on one device");
  TORCH_CHECK(packed.scalar_type() == torch::kUInt8, op, ": packed data must be uint8");
  TORCH_CHECK(out.scalar_type() == torch::kFloat32, op, ": out must be fp32");
  long chunk = out.numel();
  TORCH_CHECK(chunk % 64 == 0, op, ": chunk must be a multiple of 64, got ", chunk);
  TORCH_CHECK(chunk <= 0x40000000L, op, ": chunk ", chunk, " exceeds the 32-bit column offset");
  TORCH_CHECK(packed.dim() == 2 && packed.size(1) == chunk_bytes(chunk), op,
              ": packed must be (P, ", chunk_bytes(chunk), ") for chunk ", chunk);
  long P = packed.size(0);
  TORCH_CHECK(P >= 1 && P <= 64, op, " kernel supports 1 <= P <= 64, got ", P);
  TORCH_CHECK((uintptr_t)packed.data_ptr() % 16 == 0 && (uintptr_t)out.data_ptr() % 16 == 0, op,
              ": tensors must be 16-byte aligned");
  return (int)((chunk + unit - 1) / unit);
}

static inline int check_mx8_col(const char *op, const torch::Tensor &packed,
                                const torch::Tensor &out) {
  return check_mx_col(op, packed, out, mx8_chunk_bytes, 256);
}

template <bool AROUND>
static inline void launch_mx8_col(const torch::Tensor &packed, const torch::Tensor &out, int units,
                                  int a, int b, int c, float f, float g) {
  if (units == 0) return;  // chunk = 0: no launch
  long P = packed.size(0), chunk = out.numel();
  dim3 grid(n_blocks(units, NTHREADS / WAVE));
  for_padded(P, [&](auto n) {
    constexpr int N = decltype(n)::value;
    launch(k_mx8_col<N, mx8_cols<N>, AROUND>, grid, 0, packed.data_ptr<uint8_t>(), (int)P, a, b, c,
           f, g, (float4 *)out.data_ptr<float>(), (unsigned)chunk, mx8_chunk_bytes(chunk), units);
  });
}

void mx8_column_trimmed_mean(torch::Tensor packed, long lo, long hi, torch::Tensor out) {
  int units = check_mx8_col("mx8_column_trimmed_mean", packed, out);
  long P = packed.size(0);
  TORCH_CHECK(0 <= lo && lo < hi && hi <= P,
              "mx8_column_trimmed_mean: need 0 <= lo < hi <= P, got lo=", lo, " hi=", hi, " P=", P);
  launch_mx8_col<false>(packed, out, units, (int)lo, (int)hi, 0, (float)(hi - lo), 0.f);
}

void mx8_column_mean_around(torch::Tensor packed, long keep, long clo, long chi,
                            torch::Tensor out) {
  int units = check_mx8_col("mx8_column_mean_around", packed, out);
  long P = packed.size(0);
  TORCH_CHECK(1 <= keep && keep <= P,
              "mx8_column_mean_around: need 1 <= keep <= P, got keep=", keep, " P=", P);
  TORCH_CHECK(0 <= clo && clo < chi && chi <= P,
              "mx8_column_mean_around: need 0 <= clo < chi <= P, got clo=", clo, " chi=", chi,
              " P=", P);
  launch_mx8_col<true>(packed, out, units, (int)keep, (int)clo, (int)chi, (float)(chi - clo),
                       (float)keep);
}

// --------------------------------------------------------------------------- mx8 iterative rules
// Centered clipping and the geometric median on the mx8 wire.  Both rules pass over the
// received block several times per step (iters + 1 and n_iter + 1 passes), and each pass
// holds one column of all P rows in registers, moves a centre and returns every row's
// squared distance to the new centre.  mx8_clip_step_ = clip_step_(mx8_unpack(.), ..) and
// mx8_weiszfeld_step = segment_weighted_mean(mx8_unpack(.), ..) followed by segment_sqdist
// at the new centre, in ONE pass over the packed records: ~1.03 B per row and column per
// pass instead of 4 B (8 B for the two Weiszfeld kernels), and no fp32 block anywhere.
//
// Shared by the two kernels: k_mx8_col's access (a wave walks units of 256 columns, a lane
// owns four adjacent columns: per row one dword of codes and its block's scale byte, all P
// code loads and all P scale loads issued before the first convert) and its registers (the
// codes stay packed, N dwords; a row's scale byte becomes the fp32 operand
// 2^(max(s,10)-127) in place and a NaN block is folded into the codes).  Every row is
// decoded TWICE from those registers, two columns per v_cvt_scalef32_pk_f32_fp8: once for
// the update of the centre and once for the distances to the updated centre, so no decoded
// column is kept: N codes + N scales + N distance accumulators, four columns per lane at
// every padded size (k_clip_step drops to two at N = 48 / 64).  No instantiation uses
// scratch (profiles/kernel_bw_mx8_iter.txt has the register counts).
template <int N>
__device__ __forceinline__ void mx8_fold_scales(unsigned (&codes)[N], unsigned (&sc)[N]) {
#pragma unroll
  for (int p = 0; p < N; ++p) {
    bool nan_block = sc[p] == 0xffu;
    codes[p] = nan_block ? 0x7f7f7f7fu : codes[p];
    sc[p] = (nan_block ? 127u : max(sc[p], 10u)) << 23;
  }
}

// One dword of codes and the block's scale byte per row, for the rows `want` names: the
// record of row p starts p * cb bytes into `packed` and every offset is 32-bit (the block is
// below 4 GiB, checked on the host), so the loads share ONE 64-bit base and a row costs a
// 32-bit add, not a base pointer of its own held across the kernel.
template <int N, typename Want>
__device__ __forceinline__ void mx8_load_rows(const unsigned char *__restrict__ packed, unsigned cb,
                                              unsigned o, unsigned so, unsigned (&codes)[N],
                                              unsigned (&sc)[N], Want want) {
  unsigned ro = 0u;
#pragma unroll
  for (int p = 0; p < N; ++p) {
    codes[p] = 0u;
    sc[p] = 127u;
    if (want(p)) {
      codes[p] = *reinterpret_cast<const unsigned *>(packed + (size_t)(ro + o));
      sc[p] = packed[(size_t)(ro + so)];
    }
    ro += cb;
  }
}

// the lane's four columns of one row
__device__ __forceinline__ float4 mx8_row4(unsigned codes, unsigned scale) {
  mx8_v2f a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(codes, __uint_as_float(scale), false);
  mx8_v2f b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(codes, __uint_as_float(scale), true);
  return make_float4(a.x, a.y, b.x, b.y);
}

// Before a row's second decode: an empty asm makes the codes opaque, so that the compiler
// converts them again instead of keeping the first decode's 4 N floats alive across the
// update (it did: 149 registers at N = 24 against 3 N of codes, scales and accumulators).
__device__ __forceinline__ void mx8_decode_again(unsigned &codes) { asm volatile("" : "+v"(codes)); }

__device__ __forceinline__ float sumsq_to(float4 x, float4 c) {
  float dx = x.x - c.x, dy = x.y - c.y, dz = x.z - c.z, dw = x.w - c.w;
  return dx * dx + dy * dy + dz * dz + dw * dw;
}

// k_mx8_clip_step: k_clip_step's arithmetic, unchanged, on the records.  w is wave-uniform:
// the row tests are scalar branches, a row with w[p] == 0 is never used by the update (and
// not loaded at all when !DIST), so its NaNs cannot reach v; with every weight zero v is not
// written.  Per column the terms enter in ascending row order, as there: v comes out bit
// for bit as from k_clip_step on the decoded block.  The distances take k_clip_step's
// route, no float atomics: lane accumulators over the lane's units, xor butterfly over the
// wave, the block's waves in ascending order through LDS, one row of the (gridDim, P)
// workspace per block, k_clip_finish.  The grid depends on chunk alone, so two runs agree
// bit for bit; the sum order is not k_clip_step's at N = 48 / 64 (four columns per lane
// here), so d2 agrees with it within the rounding bound only.
template <int N, bool DIST>
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mx8_clip_step(const unsigned char *__restrict__ packed, float4 *__restrict__ v,
                const float *__restrict__ w, float *__restrict__ ws, int P, unsigned chunk,
                unsigned cbytes, int units) {
  __shared__ float part[NTHREADS / WAVE][N];
  const int lane = threadIdx.x % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const int ustride = gridDim.x * (NTHREADS / WAVE);
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
  for (int u = blockIdx.x * (NTHREADS / WAVE) + wave; u < units; u += ustride) {
    const unsigned o = (unsigned)u * 256u + 4u * lane;  // the lane's first column
    if (o >= chunk) continue;  // no cross-lane step inside the loop
    const unsigned so = chunk + o / 32;
    unsigned codes[N], sc[N];
    mx8_load_rows(packed, cbytes, o, so, codes, sc,
                  [&](int p) { return p < P && (DIST || wr[p] != 0.f); });
    float4 vv = v[o / 4];
    mx8_fold_scales(codes, sc);
    float4 delta = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int p = 0; p < N; ++p) {
      if (wr[p] != 0.f) {  // wr[p] == 0 for p >= P
        float4 x = mx8_row4(codes[p], sc[p]);
        delta.x = fmaf(wr[p], x.x - vv.x, delta.x);
        delta.y = fmaf(wr[p], x.y - vv.y, delta.y);
        delta.z = fmaf(wr[p], x.z - vv.z, delta.z);
        delta.w = fmaf(wr[p], x.w - vv.w, delta.w);
      }
    }
    if (any) {
      vv = make_float4(vv.x + delta.x, vv.y + delta.y, vv.z + delta.z, vv.w + delta.w);
      v[o / 4] = vv;
    }
    if (DIST) {
#pragma unroll
      for (int p = 0; p < N; ++p) {
        if (p < P) {
          mx8_decode_again(codes[p]);
          acc[p] += sumsq_to(mx8_row4(codes[p], sc[p]), vv);
        }
      }
    }
  }
  if (DIST) {
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

// check_mx8_col's checks for the two ops, and the 32-bit byte offsets of mx8_load_rows
static inline int check_mx8_iter(const char *op, const torch::Tensor &packed,
                                 const torch::Tensor &vz) {
  TORCH_CHECK(vz.dim() == 1, op, ": the centre must be 1D");
  int units = check_mx8_col(op, packed, vz);
  TORCH_CHECK(packed.numel() <= 0xffffffffL, op, ": ", packed.numel(),
              " bytes of records exceed the 32-bit byte offset");
  return units;
}

c10::optional<torch::Tensor> mx8_clip_step(torch::Tensor packed, torch::Tensor v, torch::Tensor w,
                                           bool dist) {
  const char *op = "mx8_clip_step";
  int units = check_mx8_iter(op, packed, v);
  long P = packed.size(0), chunk = v.numel();
  const unsigned cb = (unsigned)mx8_chunk_bytes(chunk);
  CHECK_IN(w);
  TORCH_CHECK(w.scalar_type() == torch::kFloat32 && w.dim() == 1 && w.size(0) == P, op,
              ": w must be fp32 of shape (", P, ",)");
  TORCH_CHECK(w.device() == packed.device(), op, ": w must be on packed's device");
  c10::optional<torch::Tensor> out;
  if (dist) out = torch::zeros({P}, v.options());
  if (units == 0) return out;  // chunk = 0: no launch
  const unsigned char *pp = packed.data_ptr<uint8_t>();
  float4 *vp = (float4 *)v.data_ptr<float>();
  const float *wp = w.data_ptr<float>();
  int nb = n_blocks(units, NTHREADS / WAVE);
  for_padded(P, [&](auto n_pad) {
    constexpr int N = decltype(n_pad)::value;
    if (dist) {
      torch::Tensor ws = torch::empty({(long)nb, P}, v.options());
      launch(k_mx8_clip_step<N, true>, dim3(nb), 0, pp, vp, wp, ws.data_ptr<float>(), (int)P,
             (unsigned)chunk, cb, units);
      launch(k_clip_finish, dim3((int)P), 0, ws.data_ptr<float>(), out->data_ptr<float>(), nb,
             (int)P);
    } else {
      launch(k_mx8_clip_step<N, false>, dim3(nb), 0, pp, vp, wp, nullptr, (int)P, (unsigned)chunk,
             cb, units);
    }
  });
  return out;
}

// k_mx8_weiszfeld: one Weiszfeld iteration of the per-segment geometric median in one pass:
// UPD: z[j] = fmaf(w[P-1, l], x[P-1, j], .. fmaf(w[0, l], x[0, j], 0)) for every column j of
// a segment l (k_seg_wmean's chain, ascending p, no zero-weight skip: fmaf(0, NaN) is NaN);
// columns outside every segment are left untouched; !UPD: z is only read.  DIST:
// part[p, l] += sum over the segment's columns of (x[p, j] - z_new[j])^2 (k_seg_sqdist at
// the new centre).
//
// Work split.  Unlike the grid-stride kernels of this file a WAVE OWNS A CONTIGUOUS RUN of
// `upw` units (and so does a block), so it stays inside one segment for long stretches.  The
// bounds are staged in LDS and searched on the device; per unit the search is wave-uniform.
//   Fast path, the unit's 256 columns inside one segment: the P weights are wave-uniform
// loads, the P distance accumulators stay in registers across units and are flushed (wave
// tree, one LDS add per row) only when the wave's segment changes or its run ends.
//   Slow path, a unit that holds a bound, a gap or the tail of the record: one column at a
// time with the column's own segment, weights fetched per column, columns outside every
// segment masked out of z and of the distances, one LDS add per (row, column).  At most
// one unit per bound: it need not be fast.
// The block's (P, L) LDS partials go to `part` with at most one global float atomic per
// (block, segment, row), as k_seg_sqdist and k_mx8_seg_gram do: the order of those sums, and
// so the last bits of the distances, may differ between two runs.  z takes no part in any
// cross-lane step and is bit-repeatable, and bit for bit k_seg_wmean's on the decoded block.
// Whatever seg holds, no access leaves the record: every lane is held to o < chunk and the
// segment index to [0, L).
template <int N, bool UPD, bool DIST>
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mx8_weiszfeld(const unsigned char *__restrict__ packed, const float *__restrict__ w,
                const long *__restrict__ seg, int L, int P, float *__restrict__ z,
                float *__restrict__ part /* (P, L), zeroed */, unsigned chunk, unsigned cbytes,
                int units, int upw) {
  extern __shared__ char smem[];
  long *s_seg = (long *)smem;
  float *s_acc = (float *)(smem + (L + 1) * sizeof(long));  // (P, L)
  stage_segments(s_seg, seg, L);
  if (DIST)
    for (int i = threadIdx.x; i < P * L; i += blockDim.x) s_acc[i] = 0.f;
  __syncthreads();
  const int lane = threadIdx.x % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const long g = blockIdx.x * (long)(NTHREADS / WAVE) + wave;
  const int u0 = (int)min(g * upw, (long)units), u1 = (int)min((g + 1) * upw, (long)units);
  float acc[N];
#pragma unroll
  for (int p = 0; p < N; ++p) acc[p] = 0.f;
  int cur_l = -1;  // the segment the register accumulators belong to

  auto flush = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < N; ++p) {
      if (p < P) {
        float a = wave_reduce_sum(acc[p]);
        if (lane == 0) atomicAdd(&s_acc[p * L + cur_l], a);
        acc[p] = 0.f;
      }
    }
  };

  for (int u = u0; u < u1; ++u) {  // wave-uniform
    const unsigned c0 = (unsigned)u * 256u, o = c0 + 4u * lane;
    const bool in = o < chunk;
    const unsigned so = chunk + o / 32;
    unsigned codes[N], sc[N];
    mx8_load_rows(packed, cbytes, o, so, codes, sc, [&](int p) { return p < P && in; });
    int l = cur_l;
    if (l < 0 || (long)c0 < s_seg[l] || (long)c0 + 256 > s_seg[l + 1])
      l = __builtin_amdgcn_readfirstlane(find_segment(s_seg, L, (long)c0));
    const bool whole = __builtin_amdgcn_readfirstlane(
        (int)((long)c0 >= s_seg[l] && (long)c0 + 256 <= s_seg[l + 1] && c0 + 256u <= chunk));
    mx8_fold_scales(codes, sc);
    if (whole) {
      if (l != cur_l) {
        if (DIST && cur_l >= 0) flush();
        cur_l = l;
      }
      float4 zz;
      if (UPD) {
        float wr[N];
#pragma unroll
        for (int p = 0; p < N; ++p) wr[p] = p < P ? w[p * L + l] : 0.f;
        zz = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int p = 0; p < N; ++p) {
          if (p < P) {
            float4 x = mx8_row4(codes[p], sc[p]);
            zz.x = fmaf(wr[p], x.x, zz.x);
            zz.y = fmaf(wr[p], x.y, zz.y);
            zz.z = fmaf(wr[p], x.z, zz.z);
            zz.w = fmaf(wr[p], x.w, zz.w);
          }
        }
        *reinterpret_cast<float4 *>(z + o) = zz;
      } else {
        zz = *reinterpret_cast<const float4 *>(z + o);
      }
      if (DIST) {
#pragma unroll
        for (int p = 0; p < N; ++p) {
          if (p < P) {
            mx8_decode_again(codes[p]);
            acc[p] += sumsq_to(mx8_row4(codes[p], sc[p]), zz);
          }
        }
      }
    } else {
#pragma unroll 1
      for (int k = 0; k < 4; ++k) {
        const long col = (long)o + k;
        const bool valid = in && in_segments(s_seg, L, col);
        const int lc = valid ? find_segment(s_seg, L, col) : 0;
        float zc = 0.f;
        if (UPD) {
#pragma unroll
          for (int p = 0; p < N; ++p) {
            if (p < P) {
              mx8_v2f x = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(codes[p] >> (8 * k),
                                                                   __uint_as_float(sc[p]), false);
              zc = fmaf(w[p * L + lc], x.x, zc);
            }
          }
          if (valid) z[col] = zc;
        } else if (valid) {
          zc = z[col];
        }
        if (DIST) {
#pragma unroll
          for (int p = 0; p < N; ++p) {
            if (p < P) {
              mx8_v2f x = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(codes[p] >> (8 * k),
                                                                   __uint_as_float(sc[p]), false);
              float dlt = x.x - zc;
              if (valid) atomicAdd(&s_acc[p * L + lc], dlt * dlt);
            }
          }
        }
      }
    }
  }
  if (DIST) {
    if (cur_l >= 0) flush();
    __syncthreads();
    for (int i = threadIdx.x; i < P * L; i += blockDim.x)
      if (s_acc[i] != 0.f) atomicAdd(&part[i], s_acc[i]);
  }
}

// units per wave of k_mx8_weiszfeld: the runs grow once 1024 blocks of four waves are out
static inline int mx8_weiszfeld_run(int units) { return (units + 4095) / 4096; }

c10::optional<torch::Tensor> mx8_weiszfeld_step(torch::Tensor packed,
                                                c10::optional<torch::Tensor> w, torch::Tensor seg,
                                                torch::Tensor z, bool dist) {
  const char *op = "mx8_weiszfeld_step";
  int units = check_mx8_iter(op, packed, z);
  long P = packed.size(0), chunk = z.numel();
  SegmentLds sl = segment_lds(op, seg, (size_t)P * sizeof(float));
  TORCH_CHECK(seg.device() == packed.device(), op, ": seg must be on packed's device");
  const float *wp = nullptr;
  if (w.has_value()) {
    CHECK_IN((*w));
    TORCH_CHECK(w->scalar_type() == torch::kFloat32 && w->dim() == 2 && w->size(0) == P &&
                    w->size(1) == sl.L, op, ": w must be fp32 of shape (", P, ", ", sl.L, ")");
    TORCH_CHECK(w->device() == packed.device(), op, ": w must be on packed's device");
    wp = w->data_ptr<float>();
  }
  c10::optional<torch::Tensor> out;
  if (dist) out = torch::zeros({P, (long)sl.L}, z.options());
  if (units == 0 || sl.L == 0 || (!wp && !dist)) return out;  // nothing to do: no launch
  const unsigned char *pp = packed.data_ptr<uint8_t>();
  float *zp = z.data_ptr<float>(), *op_ = dist ? out->data_ptr<float>() : nullptr;
  const long *sp = seg.data_ptr<long>();
  int upw = mx8_weiszfeld_run(units);
  dim3 grid((units + upw * (NTHREADS / WAVE) - 1) / (upw * (NTHREADS / WAVE)));
  for_padded(P, [&](auto n_pad) {
    constexpr int N = decltype(n_pad)::value;
    auto go = [&](auto kernel) {
      launch(kernel, grid, sl.bytes, pp, wp, sp, sl.L, (int)P, zp, op_, (unsigned)chunk,
             (unsigned)mx8_chunk_bytes(chunk), units, upw);
    };
    if (wp && dist) go(k_mx8_weiszfeld<N, true, true>);
    else if (wp) go(k_mx8_weiszfeld<N, true, false>);
    else go(k_mx8_weiszfeld<N, false, true>);
  });
  return out;
}

// --------------------------------------------------------------------------- mx8 krum rules
// Multi-Krum and Bulyan on the mx8 wire: mx8_segment_gram = segment_gram(mx8_unpack(.)) and
// mx8_segment_mean_around = segment_mean_around(mx8_unpack(.), ..), both from the packed
// records; the fp32 (P, chunk) block is never formed.
//
// k_mx8_seg_gram.  Lane (h = lane / 32, q = lane % 32) holds ONE MX BLOCK OF ONE ROW: row q,
// block 2j + h of the 64-column span j, 32 code bytes in 8 registers loaded as two 16-byte
// accesses, plus the block's scale byte; rows >= P are zero codes and are never loaded.  The
// block is decoded in registers (16 v_cvt_scalef32_pk_f32_fp8, as k_mx8_unpack does) and
// multiplied with v_mfma_f32_32x32x2_f32, the instruction of k_mix_rows: step s takes float s
// of every lane, i.e. K = columns s and 32 + s of the span.  A Gram is A A^T and the A and B
// operands have the same lane layout, so the same register is both operands; no LDS for the
// operands.  With P <= 32 the 32 x 32 accumulator tile (16 registers) is a whole Gram.
//
// Why not the block-scaled FP8 instruction.  v_mfma_scale_f32_32x32x64_f8f6f4 was built first
// and measured on the MI355X.  Its layout: lane (h, q) supplies row q, registers 0..3 = 16
// codes of K block 0, registers 4..7 = 16 codes of K block 1 (both at K offset 16h), scale
// operand = the scale of block h; with that the per-block sums of squares agreed with fp64 to
// a factor 0.99997 .. 0.999999, always below 1: the instruction truncates the aligned
// products well above fp32's last bit (2e-5 relative against the 4e-6 that 32 fp32 additions
// may lose), and missed the bound len * 2^-23 * sum|x_a||x_b| of tests/test_mx8_gram_gpu.py
// by 3x at len = 67.  The fp32 instruction on exactly decoded values meets it.
//
// Work split.  The spans that meet [seg[0], seg[L]) are cut into one contiguous share per
// wave; a wave walks its share MX8_GRAM_TRIP spans per trip, all loads of a trip issued before
// the first multiply, and the accumulator stays in place for as long as the spans belong to
// one segment.  The bounds are staged in LDS (segment_lds / stage_segments): no host copy, no
// descriptor table.  Everything about segments is wave-uniform: a span inside the current
// segment is decoded as loaded; a span that meets a bound is multiplied once per
// piece [lo, hi), with the codes outside the piece set to 0x00 (a bound falls anywhere: inside
// a span, a block, a dword); when the segment changes the tile is flushed and zeroed.
//
// The format's rules are applied in registers, the instruction's own treatment of special
// inputs is not relied on.  The scale byte is clamped to >= 10 before the convert.
// What decodes to a non-finite value makes the row non-finite for its segment: a NaN code
// (0x7F / 0xFF), a 0xFF scale on a block with a column in the piece, and a product code x
// scale that overflows fp32 (exponent field + scale byte >= 262: only scale bytes >= 247 can).
// All three are byte-parallel integer tests on the masked codes; the wave keeps the 32-bit set
// of such rows, and the flush writes NaN to every entry of their rows and columns, exactly
// the entries that the definition makes non-finite through them (Inf x 0 = NaN, Inf x y =
// +-Inf).  Whatever the instruction computes from those inputs lands in those entries only.
//
// Output.  Float atomics, not a fixed-order reduction: a wave adds the upper triangle of its
// tile to out[l] (the lower one is the same number, formed from the same products), and
// k_gram_mirror, launched behind it, copies the upper triangle over the lower: exactly
// symmetric, zero where no column contributes, the sum order (and so the last bits) may
// differ between two runs as for k_seg_gram.  ~1.3 flushes per wave against one per 256
// columns there.
#define MX8_GRAM_TRIP 4
typedef int mx8_v8i __attribute__((ext_vector_type(8)));

__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mx8_seg_gram(const unsigned char *__restrict__ packed, const long *__restrict__ seg, int L, int P,
               float *__restrict__ out /* (L, P, P), zeroed */, long chunk, long cbytes) {
  extern __shared__ long s_seg[];
  stage_segments(s_seg, seg, L);
  __syncthreads();
  const int lane = threadIdx.x % WAVE, h = lane / 32, q = lane % 32;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const long first = min(max(s_seg[0], 0L), chunk), last = min(max(s_seg[L], 0L), chunk);
  const long sp0 = first / 64, sp1 = (last + 63) / 64;  // the spans that meet a segment
  if (sp1 <= sp0) return;
  const long nw = gridDim.x * (long)(NTHREADS / WAVE);
  const long per = (sp1 - sp0 + nw - 1) / nw;
  const long a = sp0 + (blockIdx.x * (long)(NTHREADS / WAVE) + wave) * per;
  const long b = min(a + per, sp1);
  const unsigned char *rec = packed + q * cbytes;  // read behind q < P only
  acc16 acc = 0.f;
  int cur_l = -1;     // the segment the tile belongs to
  unsigned bad = 0u;  // its rows with a non-finite element

  auto flush = [&]() __attribute__((always_inline)) {
    float *base = out + (long)cur_l * P * P;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      int i = 8 * (v / 4) + 4 * h + v % 4;  // the tile's row in register v; its column is q
      if (i <= q && q < P)
        atomicAdd(&base[i * P + q], ((bad >> i | bad >> q) & 1u) ? __uint_as_float(0x7fc00000u) : acc[v]);
    }
    acc = 0.f;
    bad = 0u;
  };

  // one span: its pieces, 32 multiply steps each (a lambda called once per span of the trip and not
  // a loop over them: the loop is not unrolled around the ballot, and codes[] must stay in
  // registers)
  auto span = [&](const mx8_v8i &codes_t, unsigned sb_t, long spn) __attribute__((always_inline)) {
    const long c0 = spn * 64;
    const long end = spn < b ? min(c0 + 64, last) : 0;  // no such span: no piece
    long cur = max(c0, first);
    // overflow: exponent field + scale byte >= 262, i.e. field + k >= 16 with k = byte - 246
    const unsigned k = (max(sb_t, 246u) - 246u) * 0x01010101u;
    const float scale = __uint_as_float((sb_t == 0xffu ? 127u : max(sb_t, 10u)) << 23);
    while (cur < end) {
      int l = cur_l;
      if (l < 0 || cur < s_seg[l] || cur >= s_seg[l + 1]) l = find_segment(s_seg, L, cur);
      if (l != cur_l) {
        if (cur_l >= 0) flush();
        cur_l = l;
      }
      const long hi = min(s_seg[l + 1], end);
      if (hi <= cur) break;  // bounds that do not ascend: nothing to add
      mx8_v8i c = codes_t;
      // the lane's block is columns [c0 + 32 h, + 32); [s, e) of it lies in the piece
      const int s = (int)min(max(cur - c0 - 32 * h, 0L), 32L);
      const int e = (int)min(max(hi - c0 - 32 * h, 0L), 32L);
      if (cur > c0 || hi < c0 + 64) {
#pragma unroll
        for (int d = 0; d < 8; ++d) {
          int s0 = min(max(s - 4 * d, 0), 4), e0 = min(max(e - 4 * d, 0), 4);
          unsigned m = s0 < e0 ? (0xffffffffu >> (8 * (4 - e0))) & (0xffffffffu << (8 * s0)) : 0u;
          c[d] &= (int)m;
        }
      }
      unsigned nf = (sb_t == 0xffu && s < e) ? 1u : 0u;  // a NaN block with a column here
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        unsigned x = (unsigned)c[d];
        nf |= ((x & 0x7f7f7f7fu) + 0x01010101u) & 0x80808080u;  // a NaN code
        nf |= (((x >> 3) & 0x0f0f0f0fu) + k) & 0x10101010u;     // code x scale overflows
      }
      unsigned long long rows = __ballot(nf != 0u);
      bad |= (unsigned)rows | (unsigned)(rows >> 32);
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        mx8_v2f lo2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c[d], scale, false);
        mx8_v2f hi2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c[d], scale, true);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lo2.x, lo2.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lo2.y, lo2.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(hi2.x, hi2.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(hi2.y, hi2.y, acc, 0, 0, 0);
      }
      cur = hi;
    }
  };

  for (long sp = a; sp < b; sp += MX8_GRAM_TRIP) {  // wave-uniform
    mx8_v8i codes[MX8_GRAM_TRIP];
    unsigned sb[MX8_GRAM_TRIP];
#pragma unroll
    for (int t = 0; t < MX8_GRAM_TRIP; ++t) {
      codes[t] = 0;
      sb[t] = 127u;
      if (sp + t < b && q < P) {
        const uint4 *src = reinterpret_cast<const uint4 *>(rec + (sp + t) * 64 + 32 * h);
        uint4 lo = src[0], hi = src[1];
        codes[t] = mx8_v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                           (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        sb[t] = rec[chunk + (sp + t) * 2 + h];
      }
    }
    static_assert(MX8_GRAM_TRIP == 4, "one call per span of the trip");
    span(codes[0], sb[0], sp);
    span(codes[1], sb[1], sp + 1);
    span(codes[2], sb[2], sp + 2);
    span(codes[3], sb[3], sp + 3);
  }
  if (cur_l >= 0) flush();
}

__global__ void k_gram_mirror(float *__restrict__ out, int P, long n /* L * P * P */) {
  long gstride = gridDim.x * (long)blockDim.x;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < n; t += gstride) {
    int r = (int)(t % (P * P)), i = r / P, j = r % P;
    if (j < i) out[t] = out[t - r + j * P + i];
  }
}

// the chunk whose record has `cbytes` bytes (mx8_chunk_bytes is increasing in chunk)
static inline long mx8_chunk_of(const char *op, long cbytes) {
  for (long c = std::max(0L, cbytes * 32 / 33 / 64 * 64 - 64); mx8_chunk_bytes(c) <= cbytes; c += 64)
    if (mx8_chunk_bytes(c) == cbytes) return c;
  TORCH_CHECK(false, op, ": ", cbytes, " bytes are no mx8 record of a chunk that is a multiple of 64");
  return 0;
}

torch::Tensor mx8_segment_gram(torch::Tensor packed, torch::Tensor seg) {
  const char *op = "mx8_segment_gram";
  CHECK_IN(packed);
  TORCH_CHECK(packed.scalar_type() == torch::kUInt8, op, ": packed data must be uint8");
  TORCH_CHECK(packed.dim() == 2, op, ": packed must be (P, chunk_bytes)");
  SegmentLds sl = segment_lds(op, seg, 0);
  TORCH_CHECK(seg.device() == packed.device(), op, ": tensors must be on one device");
  long P = packed.size(0), chunk = mx8_chunk_of(op, packed.size(1));
  TORCH_CHECK(P >= 1 && P <= 32, op, " kernel supports 1 <= P <= 32 (one 32x32 matrix tile), got ", P);
  TORCH_CHECK((uintptr_t)packed.data_ptr() % 16 == 0, op, ": packed must be 16-byte aligned");
  auto out = torch::zeros({(long)sl.L, P, P}, torch::dtype(torch::kFloat32).device(packed.device()));
  if (sl.L == 0 || chunk == 0) return out;
  long trips = (chunk / 64 + MX8_GRAM_TRIP - 1) / MX8_GRAM_TRIP;
  launch(k_mx8_seg_gram, dim3(n_blocks(trips, NTHREADS / WAVE)), sl.bytes, packed.data_ptr<uint8_t>(),
         seg.data_ptr<long>(), sl.L, (int)P, out.data_ptr<float>(), chunk, mx8_chunk_bytes(chunk));
  launch(k_gram_mirror, dim3(n_blocks(out.numel(), NTHREADS)), 0, out.data_ptr<float>(), (int)P,
         out.numel());
  return out;
}

// k_mx8_seg_mean_around: k_seg_mean_around's per-segment gather with k_mx8_col's access
// pattern.  A wave walks units of 256 columns; a lane owns the four adjacent columns of one
// dword of codes and stores one float4.  The bounds are staged in LDS, the (L, T) table is
// read from global memory, indices are clamped into [0, P), and an unselected row is never
// read, all as in k_seg_mean_around.
//
// Whole dwords.  When every lane of the wave has its four columns in ONE segment (or all four
// outside [seg[0], seg[L])), a lane reads per selected row one dword of codes and the block's
// scale byte (branch-free over the padded slots, which re-read entry T-1), folds a NaN block
// into the codes and then runs k_mx8_col's loop: one scaled convert gives two columns, both
// are sorted (sort_columns) and reduced (mean_around_sorted), the codes shift down 16 bits
// and the loop, which is not unrolled, runs once more.  T <= 32, so two columns fit.
//
// Per column.  A wave in which some dword straddles a bound takes every lane through the same
// loop one column at a time: the column's own segment, a byte of codes per selected row, one
// sort.  That is at most one wave per bound and need not be fast.
//
// Both give segment_mean_around's bits: NaN (a NaN code or a 0xFF scale) -> +inf, slots >= T
// +inf, the same network and window arithmetic.  Columns outside the segments get +0.0 and
// every element of out is written.
template <int N>
__device__ __forceinline__ float4 mx8_gather_dwords(const unsigned char *__restrict__ packed,
                                                    const long *__restrict__ row, int T, int P,
                                                    long cbytes, unsigned o, unsigned so, int keep,
                                                    int clo, int chi, float ccnt, float kcnt) {
  unsigned codes[N], sc[N];
#pragma unroll
  for (int p = 0; p < N; ++p) {
    long r = row[p < T ? p : T - 1];
    r = r < 0 ? 0 : (r >= P ? (long)P - 1 : r);
    const unsigned char *rec = packed + r * cbytes;
    codes[p] = *reinterpret_cast<const unsigned *>(rec + o);
    sc[p] = rec[so];
  }
#pragma unroll
  for (int p = 0; p < N; ++p) {
    bool nan_block = sc[p] == 0xffu;
    codes[p] = nan_block ? 0x7f7f7f7fu : codes[p];
    sc[p] = (nan_block ? 127u : max(sc[p], 10u)) << 23;
  }
  float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
  for (int k = 0; k < 2; ++k) {
    float s[2][N];
#pragma unroll
    for (int p = 0; p < N; ++p) {
      mx8_v2f v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(codes[p], __uint_as_float(sc[p]), false);
      codes[p] >>= 16;
      s[0][p] = (p >= T || v.x != v.x) ? INFINITY : v.x;
      s[1][p] = (p >= T || v.y != v.y) ? INFINITY : v.y;
    }
    float r[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      sort_columns(s[c], std::make_integer_sequence<int, kMergeExchange<N>.n>{});
      r[c] = mean_around_sorted(s[c], T, keep, clo, chi, ccnt, kcnt);
    }
    y = make_float4(y.z, y.w, r[0], r[1]);
  }
  return y;
}

template <int N>
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mx8_seg_mean_around(const unsigned char *__restrict__ packed, const long *__restrict__ sel,
                      const long *__restrict__ seg, int L, int T, int P, int keep, int clo, int chi,
                      float ccnt, float kcnt, float4 *__restrict__ out, unsigned chunk, long cbytes,
                      int units) {
  extern __shared__ long s_seg[];
  stage_segments(s_seg, seg, L);
  __syncthreads();
  const int lane = threadIdx.x % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const int ustride = gridDim.x * (NTHREADS / WAVE);
  for (int u = blockIdx.x * (NTHREADS / WAVE) + wave; u < units; u += ustride) {
    const unsigned o = (unsigned)u * 256u + 4u * lane;  // the lane's first column
    const bool inb = o < chunk;  // chunk % 64 == 0: four columns are inside or outside together
    const bool v0 = inb && in_segments(s_seg, L, o);
    const int l0 = v0 ? find_segment(s_seg, L, o) : 0;
    const bool same = v0 && (long)o + 3 < s_seg[l0 + 1];
    const bool none = !inb || (long)o + 3 < s_seg[0] || (long)o >= s_seg[L];
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (__all(same || none)) {
      if (same)
        y = mx8_gather_dwords<N>(packed, sel + (long)l0 * T, T, P, cbytes, o, chunk + o / 32, keep,
                                 clo, chi, ccnt, kcnt);
    } else {
#pragma unroll 1
      for (int k = 0; k < 4; ++k) {
        const unsigned col = o + k;
        const bool valid = inb && in_segments(s_seg, L, col);
        float s[N];
#pragma unroll
        for (int p = 0; p < N; ++p) s[p] = INFINITY;
        if (valid) {
          const long *row = sel + (long)find_segment(s_seg, L, col) * T;
#pragma unroll
          for (int p = 0; p < N; ++p) {
            long r = row[p < T ? p : T - 1];
            r = r < 0 ? 0 : (r >= P ? (long)P - 1 : r);
            const unsigned char *rec = packed + r * cbytes;
            unsigned code = rec[col], sbyte = rec[chunk + col / 32];
            bool nan_block = sbyte == 0xffu;
            float scale = __uint_as_float((nan_block ? 127u : max(sbyte, 10u)) << 23);
            mx8_v2f v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(nan_block ? 0x7fu : code, scale, false);
            s[p] = (p < T && v.x == v.x) ? v.x : INFINITY;
          }
        }
        sort_columns(s, std::make_integer_sequence<int, kMergeExchange<N>.n>{});
        float r = mean_around_sorted(s, T, keep, clo, chi, ccnt, kcnt);
        y = make_float4(y.y, y.z, y.w, valid ? r : 0.f);
      }
    }
    if (inb) out[o / 4] = y;
  }
}

void mx8_segment_mean_around(torch::Tensor packed, torch::Tensor sel, torch::Tensor seg, long keep,
                             long clo, long chi, torch::Tensor out) {
  const char *op = "mx8_segment_mean_around";
  int units = check_mx8_col(op, packed, out);
  CHECK_IDX(sel);
  TORCH_CHECK(sel.dim() == 2, op, ": sel must be 2D (L, T)");
  SegmentLds sl = segment_lds(op, seg, 0);
  TORCH_CHECK(sel.device() == packed.device() && seg.device() == packed.device(), op,
              ": tensors must be on one device");
  long P = packed.size(0), T = sel.size(1), chunk = out.numel();
  TORCH_CHECK(P <= 32, op, " kernel supports 1 <= P <= 32, got ", P);
  TORCH_CHECK(sel.size(0) == sl.L, op, ": sel must have one row per segment, got ", sel.size(0),
              " rows for L=", sl.L);
  TORCH_CHECK(T >= 1 && T <= P, op, ": need 1 <= T <= P, got T=", T, " P=", P);
  TORCH_CHECK(1 <= keep && keep <= T, op, ": need 1 <= keep <= T, got keep=", keep, " T=", T);
  TORCH_CHECK(0 <= clo && clo < chi && chi <= T, op, ": need 0 <= clo < chi <= T, got clo=", clo,
              " chi=", chi, " T=", T);
  if (units == 0) return;  // chunk = 0: no launch
  dim3 grid(n_blocks(units, NTHREADS / WAVE));
  for_padded(T, [&](auto n) {
    constexpr int N = decltype(n)::value;
    if constexpr (N <= 32)  // T <= P <= 32
      launch(k_mx8_seg_mean_around<N>, grid, sl.bytes, packed.data_ptr<uint8_t>(),
             sel.data_ptr<long>(), seg.data_ptr<long>(), sl.L, (int)T, (int)P, (int)keep, (int)clo,
             (int)chi, (float)(chi - clo), (float)keep, (float4 *)out.data_ptr<float>(),
             (unsigned)chunk, mx8_chunk_bytes(chunk), units);
  });
}

// --------------------------------------------------------------------------- mx4 wire
// A 4-bit block-scaled wire format for gradient rows: OCP Microscaling MXFP4, E2M1 elements
// with one E8M0 scale per 32 elements, rounded to nearest or STOCHASTICALLY (unbiased per
// element).  Like the mx8 wire it decodes to an ordinary fp32 block that every rule reads.
//
// WIRE FORMAT (the one description; fallback.mx4_pack / mx4_unpack produce the same bytes).
// Element code: one nibble, E2M1: 1 sign, 2 exponent (bias 1), 1 mantissa bit; the
// magnitudes of codes 0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6; no NaN or Inf codes.  Element 2k
// of a row is the low nibble of byte k, element 2k+1 the high nibble.  Block: 32 consecutive
// elements share a scale byte s, an E8M0 exponent meaning 2^(s-127); s = 0xFF is NaN for the
// whole block.
//   Encoding a block: if any element is NaN or +-Inf the scale byte is 0xFF (the format's
// price: one non-finite element costs that worker 32 coordinates of NaN, never more, and a
// non-finite element stays non-finite); the 16 code bytes are still written as below, with
// a non-finite element coded as 0 with its sign, and decoders ignore them.  amax = the
// largest |x| over the block's finite elements; e = the smallest integer with
// amax / 2^e <= 6, read off amax's bits: e = exponent(amax) - 2, plus 1 if the mantissa
// field exceeds 0x400000 (6 = 1.5 * 2^2); e is clamped to >= -125 (also taken when amax = 0)
// and s = e + 127 is in [2, 253].  Nothing saturates.  x's sign bit is kept, also for -0.0
// and for values that round to zero.
//   Rounding of t = |x| * 2^-e (t < 2^-126 counts as 0).  Nearest: the nearest grid value,
// ties to the even code.  Stochastic: with lo the largest grid value <= t, hi the next one
// and step = hi - lo, round up iff float(r) < ((t - lo) / step) * 2^24 for a 24-bit random
// integer r (every operation of that line is exact in fp32): P(up) is within 2^-24 of
// (t - lo) / step, and t on the grid never moves.  r of element i of the row (i mod 2^32)
// under a 64-bit seed is a stateless hash, whatever the launch geometry:
// h(a): a ^= a >> 16; a *= 0x7feb352d; a ^= a >> 15; a *= 0x846ca68b; a ^= a >> 16 (32-bit),
// key = h(seed_lo ^ h(seed_hi + 0x9e3779b9)), r = h(i ^ key) >> 8.
//   Both roundings are stated in integers on x's significand M (24 bits, hidden bit
// included) and q = max(exponent field, 1) - s, t = M * 2^(q-23), q <= 2: the grid steps
// by 2^(22-sh) * t / M with sh = 22 - min(q, 0), so lo's code is (M >> sh) + 2 * max(q, 0),
// the next code is hi's, and (t - lo) / step = frac / 2^sh with frac = M mod 2^sh.
//   Decoding: s = 0xFF gives 32 NaNs; otherwise s is clamped to >= 2 and value = code value
// * 2^(s-127) in fp32.  With the clamp every finite non-zero result is a normal fp32 number
// (0.5 * 2^-125 = 2^-126); an overflowing product (6 * 2^127) is +-Inf.  Every byte pattern
// decodes to an fp32 value, NaN or +-Inf.
//   Packed row: packed against a chunk (the shard length) with n % chunk == 0 and
// chunk % 64 == 0 into n / chunk records of chunk_bytes = chunk / 2 + round_up(chunk / 32,
// 16) bytes: the code bytes, the scale bytes, zero padding.  Records and scale runs start
// 16-byte aligned, a record depends on its chunk's elements alone, and the even all_to_all
// split of a packed row lands each rank's codes and scales on it, as for mx8.
//   Error: nearest, |decode(encode(x)) - x| <= max(|x| / 4, X / 4) with X = 2^e < amax / 3;
// stochastic, below one grid step (at most max(|x| / 2, X / 2)) and E[decode(encode(x))] = x
// up to 2^-24 of a step.
//
// The gfx950 scaled converts (v_cvt_scalef32_pk_fp4_f32 / v_cvt_scalef32_pk_f32_fp4) do the
// element work of the nearest encode and of the decode.  Measured once on the MI355X with a
// stand-alone probe program that is not in the tree (the exact tests of
// tests/test_mx4_gpu.py are what stays), against the integer statement above: the encode,
// issued as the kernel issues it (four converts filling bytes 0..3 of a dword, source 0 in
// the low nibble), gives the format's nibble for every fp32 bit pattern of either sign that
// is in range for scales 2, 3, 60, 127, 200, 252 and 253 (nearest, ties to the even code,
// fp32 subnormal inputs honoured, sign of zero and of values that round to zero kept); the
// decode is exact for all 256 code bytes at every scale 2..254, the overflow to +-Inf and
// -0.0 included.  Neither needed a patch.  The scale operand is the fp32 number 2^(s-127),
// always normal here.  Non-finite elements reach the convert as signed zeros and
// out-of-range inputs are never converted, so what the instruction does with them is not
// relied on.  The stochastic rounding is NOT the hardware's v_cvt_scalef32_sr_pk_fp4_f32
// (its use of the random operand is not documented and was not probed): it is the integer
// statement above in plain VALU arithmetic.
//
// Both kernels walk "units": a unit is 512 consecutive elements of one record, eight per
// lane, MX4_TRIP units per wave per trip with all loads issued before any conversion.
// chunk % 64 == 0: in k_mx4_pack a lane's eight consecutive elements and a 32-element block
// (one quad of lanes) are inside or outside the record as a whole, and a unit's 16 scale
// bytes are one 16-byte store: round_up(chunk / 32, 16) is whole units of them.
#define MX4_TRIP 2

static inline long mx4_chunk_bytes(long chunk) { return chunk / 2 + (chunk / 32 + 15) / 16 * 16; }

__device__ __forceinline__ unsigned mx4_hash(unsigned a) {
  a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15; a *= 0x846ca68bu; a ^= a >> 16;
  return a;
}

// max over the four lanes of a block, in every one of them: two quad permutes
__device__ __forceinline__ unsigned mx4_block_max(unsigned v) {
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));  // lane ^ 1
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));  // lane ^ 2
  return v;
}

// the stochastically rounded code (no sign) of a finite magnitude `a` (fp32 bits) in a block
// of scale byte s, by the integer statement above; r: the element's 24 random bits
__device__ __forceinline__ unsigned mx4_code_sr(unsigned a, int s, unsigned r) {
  int ex = (int)(a >> 23);
  unsigned M = (a & 0x7fffffu) | (ex ? 0x800000u : 0u);
  int q = max(ex, 1) - s;
  int sh = 22 - min(q, 0);  // 22 .. 274
  unsigned lo = (M >> min(sh, 31)) + 2u * (unsigned)max(q, 0);
  unsigned frac = M & ((1u << min(sh, 31)) - 1u);
  // up iff r < frac * 2^24 / 2^sh: an integer threshold either way (past sh = 48 it is r == 0)
  int d = min(sh - 24, 24);
  unsigned thr = sh <= 24 ? frac << (24 - sh) : (frac + (1u << d) - 1u) >> d;
  bool tiny = sh > 125 && (M >> min(sh - 125, 31)) == 0u;  // t < 2^-126
  return lo + (unsigned)(r < thr && !tiny);
}

// k_mx4_pack<SR>: one streaming pass, 4 B read and ~0.53 B written per element, no LDS, no
// atomics.  Per unit a lane holds eight elements: non-finite ones are replaced by a signed
// zero (their code) and flagged, the finite amax and the flag are reduced over the quad by
// DPP, the scale byte comes from amax's exponent and mantissa fields.  Nearest (SR = false):
// four scaled converts give the lane's dword of codes.  Stochastic: eight integer roundings
// (mx4_code_sr), each with its own hash of the element index.  A wave stores 256 contiguous
// code bytes.  The unit's 16 scale bytes: every lane shifts its block's byte to the block's
// place in its row's dword (a row is 16 lanes, four blocks), two mirror DPP steps OR the
// row's four bytes together in every lane, four v_readlane collect the rows, and lane 0
// stores one 16-byte vector.  An outside block contributes 0, which is the record's padding.
// The loop's trip count is wave-uniform: every lane runs the DPP and readlane steps.
template <bool SR>
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mx4_pack(const uint4 *__restrict__ g, unsigned char *__restrict__ out, long chunk, long cbytes,
           int upr, int units, unsigned seed_lo, unsigned seed_hi) {
  const int lane = threadIdx.x % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const unsigned place = 8u * ((unsigned)(lane >> 2) & 3u);
  const unsigned key = mx4_hash(seed_lo ^ mx4_hash(seed_hi + 0x9e3779b9u));
  long u0 = (blockIdx.x * (long)(NTHREADS / WAVE) + wave) * MX4_TRIP;
  long ustride = gridDim.x * (long)(NTHREADS / WAVE) * MX4_TRIP;
  for (; u0 < units; u0 += ustride) {
    // u0 < units fits an int (checked on the host): a 32-bit division, once per trip
    const int u = (int)u0;
    int r = u / upr, j = u - r * upr;  // record, unit of the record
    uint4 v[MX4_TRIP][2];
    long base[MX4_TRIP];  // byte offset of the unit's record; -1: no such unit
    long first[MX4_TRIP];  // the row index of the record's first element
    int uj[MX4_TRIP];
#pragma unroll
    for (int t = 0; t < MX4_TRIP; ++t) {
      long o = (long)j * 512 + 8 * lane;  // the lane's first element in the record
      base[t] = u0 + t < units ? r * cbytes : -1;
      first[t] = r * chunk;
      uj[t] = j;
      v[t][0] = v[t][1] = make_uint4(0u, 0u, 0u, 0u);
      if (base[t] >= 0 && o < chunk) {
        v[t][0] = g[(first[t] + o) / 4];
        v[t][1] = g[(first[t] + o) / 4 + 1];
      }
      if (++j == upr) { j = 0; ++r; }
    }
#pragma unroll
    for (int t = 0; t < MX4_TRIP; ++t) {
      long o = (long)uj[t] * 512 + 8 * lane;
      bool in = base[t] >= 0 && o < chunk;
      unsigned x[8] = {v[t][0].x, v[t][0].y, v[t][0].z, v[t][0].w,
                       v[t][1].x, v[t][1].y, v[t][1].z, v[t][1].w};
      unsigned amax = 0u, bad = 0u;
#pragma unroll
      for (int k = 0; k < 8; ++k) {  // NaN, +-Inf: a zero with the element's sign, and the flag
        unsigned a = x[k] & 0x7fffffffu;
        bool fin = a < 0x7f800000u;
        a = fin ? a : 0u;
        amax = max(amax, a);
        bad |= (unsigned)!fin;
        x[k] = a | (x[k] & 0x80000000u);
      }
      amax = mx4_block_max(amax);
      bad = mx4_block_max(bad);
      int s = (int)(amax >> 23) - 2 + ((amax & 0x7fffffu) > 0x400000u);
      s = max(s, 2);
      unsigned codes = 0u;
      if constexpr (SR) {
        const unsigned i0 = (unsigned)(first[t] + o);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          unsigned r24 = mx4_hash((i0 + k) ^ key) >> 8;
          codes |= (mx4_code_sr(x[k] & 0x7fffffffu, s, r24) | (x[k] >> 28 & 8u)) << (4 * k);
        }
      } else {
        float scale = __uint_as_float((unsigned)s << 23);
        codes = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(codes, __uint_as_float(x[0]), __uint_as_float(x[1]), scale, 0);
        codes = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(codes, __uint_as_float(x[2]), __uint_as_float(x[3]), scale, 1);
        codes = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(codes, __uint_as_float(x[4]), __uint_as_float(x[5]), scale, 2);
        codes = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(codes, __uint_as_float(x[6]), __uint_as_float(x[7]), scale, 3);
      }
      if (in) *reinterpret_cast<unsigned *>(out + base[t] + o / 2) = codes;
      unsigned w = (in ? (bad ? 0xffu : (unsigned)s) : 0u) << place;
      w |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0x141, 0xF, 0xF, false);  // 7 - lane
      w |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0x140, 0xF, 0xF, false);  // 15 - lane
      uint4 sc = make_uint4((unsigned)__builtin_amdgcn_readlane((int)w, 0),
                            (unsigned)__builtin_amdgcn_readlane((int)w, 16),
                            (unsigned)__builtin_amdgcn_readlane((int)w, 32),
                            (unsigned)__builtin_amdgcn_readlane((int)w, 48));
      if (lane == 0 && base[t] >= 0)
        *reinterpret_cast<uint4 *>(out + base[t] + chunk / 2 + 16L * uj[t]) = sc;
    }
  }
}

// k_mx4_unpack: ~0.53 B read and 4 B written per element.  The writes are what the kernel
// moves, so the lanes are laid out for them and not as in k_mx4_pack: of a unit's 128 float4 a
// lane owns numbers `lane` and `64 + lane`, so that each of its two stores is 1 KB contiguous
// per wave (a lane storing two adjacent float4 fills half of every cache line per store, which
// measured 25% slower than k_mx8_unpack; this layout is still 6 to 11% slower than it, see
// profiles/kernel_bw_mx4.txt).  It reads the two 16-bit code pairs of
// those float4 (128 contiguous bytes per wave each) and their blocks' scale bytes (one byte
// shared by eight lanes, a cached byte load), and runs four scaled converts, byte selects 0
// and 1 of each pair.  The load loop only loads: combining the two pairs into one dword there
// made the compiler wait for each load before issuing the next (three s_waitcnt vmcnt per
// trip, read off the ISA).  The rows are flattened into the unit index.  No cross-lane step,
// so an outside lane simply skips.
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mx4_unpack(const unsigned char *__restrict__ packed, float4 *__restrict__ out, long chunk,
             long cbytes, int upr, int units) {
  const int lane = threadIdx.x % WAVE;
  long u0 = (blockIdx.x * (long)(NTHREADS / WAVE) + threadIdx.x / WAVE) * MX4_TRIP;
  long ustride = gridDim.x * (long)(NTHREADS / WAVE) * MX4_TRIP;
  for (; u0 < units; u0 += ustride) {
    const int u = (int)u0;  // as in k_mx4_pack
    int r = u / upr, j = u - r * upr;
    unsigned codes[MX4_TRIP][2], sbyte[MX4_TRIP][2];  // loaded values are not touched in this loop
    long dst[MX4_TRIP];  // float4 index in out of the lane's first float4; -1: nothing to do
    bool second[MX4_TRIP];  // the lane's second float4 is inside the record too
#pragma unroll
    for (int t = 0; t < MX4_TRIP; ++t) {
      long o = (long)j * 512 + 4 * lane;  // the first float4's elements; the second: o + 256
      bool in = u0 + t < units && o < chunk;
      second[t] = in && o + 256 < chunk;
      dst[t] = in ? (r * chunk + o) / 4 : -1;
      codes[t][0] = codes[t][1] = sbyte[t][0] = sbyte[t][1] = 0u;
      const unsigned char *rec = packed + r * cbytes;
      if (in) {
        codes[t][0] = *reinterpret_cast<const unsigned short *>(rec + o / 2);
        sbyte[t][0] = rec[chunk / 2 + o / 32];
      }
      if (second[t]) {
        codes[t][1] = *reinterpret_cast<const unsigned short *>(rec + o / 2 + 128);
        sbyte[t][1] = rec[chunk / 2 + o / 32 + 8];
      }
      if (++j == upr) { j = 0; ++r; }
    }
#pragma unroll
    for (int t = 0; t < MX4_TRIP; ++t) {
      const float nan = __uint_as_float(0x7fc00000u);
      float s0 = __uint_as_float(max(sbyte[t][0], 2u) << 23);
      float s1 = __uint_as_float(max(sbyte[t][1], 2u) << 23);
      mx8_v2f a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(codes[t][0], s0, 0);
      mx8_v2f b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(codes[t][0], s0, 1);
      mx8_v2f c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(codes[t][1], s1, 0);
      mx8_v2f d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(codes[t][1], s1, 1);
      float4 y0 = make_float4(a.x, a.y, b.x, b.y), y1 = make_float4(c.x, c.y, d.x, d.y);
      if (sbyte[t][0] == 0xffu) y0.x = y0.y = y0.z = y0.w = nan;
      if (sbyte[t][1] == 0xffu) y1.x = y1.y = y1.z = y1.w = nan;
      if (dst[t] >= 0) out[dst[t]] = y0;
      if (second[t]) out[dst[t] + 64] = y1;
    }
  }
}

static inline int check_mx4(const char *op, const torch::Tensor &vals, const torch::Tensor &bytes,
                            long chunk, long records) {
  return check_mx(op, vals, bytes, chunk, records, mx4_chunk_bytes(chunk), 512, MX4_TRIP);
}

// seed: read only with stochastic = true; it reaches the kernel by value, as two words
void mx4_pack(torch::Tensor g, torch::Tensor out, long chunk, bool stochastic, uint64_t seed) {
  long n = g.numel();
  TORCH_CHECK(g.dim() == 1 && out.dim() == 1, "mx4_pack: g and out must be 1D");
  TORCH_CHECK(chunk > 0 ? n % chunk == 0 : n == 0, "mx4_pack: length ", n,
              " is not a multiple of chunk ", chunk);
  int units = check_mx4("mx4_pack", g, out, chunk, chunk > 0 ? n / chunk : 0);
  if (units == 0) return;
  int upr = (int)((chunk + 511) / 512);
  int blocks = n_blocks((units + MX4_TRIP - 1) / MX4_TRIP, NTHREADS / WAVE);
  launch(stochastic ? k_mx4_pack<true> : k_mx4_pack<false>, dim3(blocks), 0,
         (const uint4 *)g.data_ptr<float>(), out.data_ptr<uint8_t>(), chunk, mx4_chunk_bytes(chunk),
         upr, units, (unsigned)seed, (unsigned)(seed >> 32));
}

void mx4_unpack(torch::Tensor packed, torch::Tensor out) {
  TORCH_CHECK(packed.dim() == 2 && out.dim() == 2 && packed.size(0) == out.size(0),
              "mx4_unpack: packed must be (P, chunk_bytes) and out (P, chunk)");
  long P = out.size(0), chunk = out.size(1);
  int units = check_mx4("mx4_unpack", out, packed, chunk, P);
  TORCH_CHECK(packed.size(1) == mx4_chunk_bytes(chunk), "mx4_unpack: packed rows must have ",
              mx4_chunk_bytes(chunk), " bytes for chunk ", chunk, ", got ", packed.size(1));
  if (units == 0) return;  // P = 0 or chunk = 0: no launch
  int upr = (int)((chunk + 511) / 512);
  int blocks = n_blocks((units + MX4_TRIP - 1) / MX4_TRIP, NTHREADS / WAVE);
  launch(k_mx4_unpack, dim3(blocks), 0, packed.data_ptr<uint8_t>(), (float4 *)out.data_ptr<float>(),
         chunk, mx4_chunk_bytes(chunk), upr, units);
}

// --------------------------------------------------------------------------- mx4 column rules
// mx4_column_trimmed_mean / mx4_column_mean_around: mx4_unpack followed by
// column_trimmed_mean / column_mean_around, bit for bit, in one launch that reads the packed
// records themselves: ~0.53 B per row and column instead of 0.53 B + 4 B written + 4 B read
// back, and no (P, chunk) fp32 block anywhere.  The sort and the rule arithmetic are
// k_mx8_col's (sort_columns, trimmed_sorted, mean_around_sorted, unchanged); the record is
// not: two codes per byte, no NaN code, a scale clamp of 2.
//
// Work split.  A wave walks units of 512 consecutive columns, k_mx4_pack's unit (grid-stride
// over units, one unit per wave per trip); a lane owns the EIGHT adjacent columns 8*lane ..
// 8*lane+7 and per row loads one dword of codes, 256 contiguous bytes per wave.  Eight
// aligned columns lie in one 32-element block, so one scale byte per row serves them; it is a
// per-lane byte load (four lanes read the same byte, 16 contiguous bytes per wave and row).
// The row base is wave-uniform and the lane offsets 32-bit (checked on the host).  All P code
// loads and all P scale loads of a unit are issued before the first conversion, behind
// wave-uniform `p < P` tests.  chunk % 64 == 0, so a lane's eight columns are inside the
// record or outside as a whole: no cross-lane step, no LDS, no atomics, and an outside lane
// of the unit that ends the shard simply skips.
//
// Registers.  The codes stay packed, N dwords.  A row's scale byte becomes the fp32 operand
// 2^(max(s,2)-127): a register per row, or its exponent alone, four to a register, for the
// padded sizes at which one sorted column is all that fits beside the codes (mx4_cols).
// E2M1 has no NaN code, so a NaN block (s = 0xFF) cannot be folded into the codes as a NaN,
// which is what k_mx8_col does.  It is folded in as what the fp32 column op turns a NaN
// into before it sorts, +inf: the row's dword becomes eight codes 7 (0x77777777) and its
// scale operand 2^127, and 6 * 2^127 overflows to +inf in the convert, the same overflow an
// honest code 7 at s = 254 takes.  All eight of a lane's columns share the block, so the
// whole dword goes; a padding row (p >= P) starts as such a row.  The conversion loop then
// has no NaN test and no select at all.  (A 64-bit row mask per lane with a select per
// value was built first: the compiler kept the N mask tests as N lane masks in SGPR pairs,
// spilled to VGPR lanes, at 130 / 169 VGPRs for N = 24 / 32 trimmed mean against 112 / 144
// here, one wave per SIMD fewer at each.)  The scale operand is never a NaN.
//
// Conversion loop.  v_cvt_scalef32_pk_f32_fp4 of byte 0 yields two columns, the low nibble
// then the high one; its byte select is an immediate, so the loop over a lane's columns is
// NOT unrolled: it always converts byte 0 and shifts the codes down by 8 bits, so one copy
// of the sort network serves all eight columns.  Where two sorted columns do not fit
// (COLS = 1) the codes shift by 4 bits and .x alone is taken.  The results rotate through two
// float4 (no run-time-indexed array) and leave as two 16-byte stores per lane; the output is
// 1/P of the traffic, so k_mx4_unpack's store layout is not worth a lane shuffle here.
//
// Relied on from the convert: what k_mx4_unpack relies on and the header of the mx4 wire
// records as measured (every code byte exact at every scale operand 2^-125 .. 2^127, -0.0
// and the overflow of code 7 at s = 254 to +-Inf included, which is also what makes a NaN
// block +inf here; +-Inf sort as themselves, as they do after mx4_unpack).  Not relied on: a NaN or subnormal scale operand (never issued), and
// bytes 1..3 of the source (shifted into byte 0 instead of selected).  s[] is indexed by
// compile-time constants only; no instantiation uses scratch
// (profiles/kernel_bw_mx4_fused.txt).
template <int N> constexpr int mx4_cols = N <= 32 ? 2 : 1;

// AROUND: (a, b, c) = (keep, clo, chi), (f, g) = (ccnt, kcnt); else (a, b) = (lo, hi), f = cnt
template <int N, int COLS, bool AROUND>
__global__ void __launch_bounds__(NTHREADS) NO_PACKED_FP32
k_mx4_col(const unsigned char *__restrict__ packed, int P, int a, int b, int c, float f, float g,
          float4 *__restrict__ out, unsigned chunk, long cbytes, int units) {
  const int lane = threadIdx.x % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const int ustride = gridDim.x * (NTHREADS / WAVE);
  constexpr bool PACK = COLS == 1;  // scale exponents four to a register
  for (int u = blockIdx.x * (NTHREADS / WAVE) + wave; u < units; u += ustride) {
    const unsigned o = (unsigned)u * 512u + 8u * lane;  // the lane's first column
    if (o >= chunk) continue;
    const unsigned co = o / 2, so = chunk / 2 + o / 32;  // its code dword, its block's scale byte
    unsigned codes[N], sb[N];
#pragma unroll
    for (int p = 0; p < N; ++p) {
      codes[p] = 0u;
      sb[p] = 0xffu;  // a padding row is a NaN block
      if (p < P) {
        const unsigned char *rec = packed + p * cbytes;
        codes[p] = *reinterpret_cast<const unsigned *>(rec + co);
        sb[p] = rec[so];
      }
    }
    unsigned sc[PACK ? N / 4 : N] = {};
#pragma unroll
    for (int p = 0; p < N; ++p) {
      bool nan_block = sb[p] == 0xffu;
      codes[p] = nan_block ? 0x77777777u : codes[p];  // 6 * 2^127 = +inf, eight times
      unsigned e = nan_block ? 254u : max(sb[p], 2u);
      if constexpr (PACK) sc[p / 4] |= e << (8 * (p % 4));
      else sc[p] = e << 23;
    }
    float4 y0 = make_float4(0.f, 0.f, 0.f, 0.f), y1 = y0;
#pragma unroll 1
    for (int k = 0; k < 8 / COLS; ++k) {
      float s[COLS][N];
      if constexpr (PACK) {
        // as in k_mx8_col: keeps the compiler from hoisting the N unpacked scales out of
        // the loop, back into N registers
#pragma unroll
        for (int p = 0; p < N / 4; ++p) asm volatile("" : "+v"(sc[p]));
      }
#pragma unroll
      for (int p = 0; p < N; ++p) {
        unsigned scale = PACK ? (sc[p / 4] >> (8 * (p % 4)) & 0xffu) << 23 : sc[p];
        // ... and from issuing all N converts first, each holding a register pair for the
        // one value that is taken: a convert waits for the one before it
        if (PACK && p > 0) asm volatile("" : "+v"(s[0][p - 1]), "+v"(codes[p]));
        mx8_v2f v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(codes[p], __uint_as_float(scale), 0);
        codes[p] >>= 4 * COLS;
        s[0][p] = v.x;
        if constexpr (COLS == 2) s[1][p] = v.y;
      }
      float r[COLS];
#pragma unroll
      for (int q = 0; q < COLS; ++q) {
        sort_columns(s[q], std::make_integer_sequence<int, kMergeExchange<N>.n>{});
        r[q] = AROUND ? mean_around_sorted(s[q], P, a, b, c, f, g) : trimmed_sorted(s[q], a, b, f);
      }
      // the results move down COLS places per trip: after the last one y0 holds columns
      // 0..3 and y1 columns 4..7
      if constexpr (COLS == 2) {
        y0 = make_float4(y0.z, y0.w, y1.x, y1.y);
        y1 = make_float4(y1.z, y1.w, r[0], r[1]);
      } else {
        y0 = make_float4(y0.y, y0.z, y0.w, y1.x);
        y1 = make_float4(y1.y, y1.z, y1.w, r[0]);
      }
    }
    out[o / 4] = y0;
    out[o / 4 + 1] = y1;
  }
}

static inline int check_mx4_col(const char *op, const torch::Tensor &packed,
                                const torch::Tensor &out) {
  return check_mx_col(op, packed, out, mx4_chunk_bytes, 512);
}

template <bool AROUND>
static inline void launch_mx4_col(const torch::Tensor &packed, const torch::Tensor &out, int units,
                                  int a, int b, int c, float f, float g) {
  if (units == 0) return;  // chunk = 0: no launch
  long P = packed.size(0), chunk = out.numel();
  dim3 grid(n_blocks(units, NTHREADS / WAVE));
  for_padded(P, [&](auto n) {
    constexpr int N = decltype(n)::value;
    launch(k_mx4_col<N, mx4_cols<N>, AROUND>, grid, 0, packed.data_ptr<uint8_t>(), (int)P, a, b, c,
           f, g, (float4 *)out.data_ptr<float>(), (unsigned)chunk, mx4_chunk_bytes(chunk), units);
  });
}

void mx4_column_trimmed_mean(torch::Tensor packed, long lo, long hi, torch::Tensor out) {
  int units = check_mx4_col("mx4_column_trimmed_mean", packed, out);
  long P = packed.size(0);
  TORCH_CHECK(0 <= lo && lo < hi && hi <= P,
              "mx4_column_trimmed_mean: need 0 <= lo < hi <= P, got lo=", lo, " hi=", hi, " P=", P);
  launch_mx4_col<false>(packed, out, units, (int)lo, (int)hi, 0, (float)(hi - lo), 0.f);
}

void mx4_column_mean_around(torch::Tensor packed, long keep, long clo, long chi,
                            torch::Tensor out) {
  int units = check_mx4_col("mx4_column_mean_around", packed, out);
  long P = packed.size(0);
  TORCH_CHECK(1 <= keep && keep <= P,
              "mx4_column_mean_around: need 1 <= keep <= P, got keep=", keep, " P=", P);
  TORCH_CHECK(0 <= clo && clo < chi && chi <= P,
              "mx4_column_mean_around: need 0 <= clo < chi <= P, got clo=", clo, " chi=", chi,
              " P=", P);
  launch_mx4_col<true>(packed, out, units, (int)keep, (int)clo, (int)chi, (float)(chi - clo),
                       (float)keep);
}

// --------------------------------------------------------------------------- gradient sink
// scatter_grads: the gradients of one backward (a list of dense fp32 / bf16 tensors) into
// the worker's flat fp32 payload row, every element of the row written exactly once: the
// range of source i becomes float(src_i) in the order of its storage, everything else
// (gaps, the pad tail) becomes +0.0.  It replaces the row's memset, autograd's per-tensor
// cast of a bf16 gradient to a new fp32 tensor and the per-parameter `grad += g` into the
// zeroed row: one pass, the sources read once and the row written once.
//
// The call sits inside a captured graph, so nothing about the list may live in device
// memory that the host writes: pointers, offsets, lengths and dtypes travel BY VALUE in
// the kernel arguments, SINK_CAP ranges per launch (ResNet-18: 62 tensors + the tail, one
// launch).  A block takes one SINK_CHUNK-element chunk of one range and finds it by a
// binary search over the prefix of chunk counts in the same arguments.  Accesses are
// 16 bytes wide wherever the destination offset and the source pointer allow: the head up
// to the destination's first 16-byte boundary and the tail are scalar, and a source that
// is not 16-byte aligned at that boundary is read element by element (the stores stay
// 16 bytes).  bf16 -> fp32 is the exact widening (a 16-bit shift): NaN payloads, +-Inf,
// -0.0 and subnormals are kept.  Definition: fallback.scatter_grads_.
#define SINK_CAP 64
#define SINK_CHUNK 4096

struct SinkTable {
  const void *src[SINK_CAP];  // nullptr: the range is zero-filled
  long off[SINK_CAP];         // first destination element
  long len[SINK_CAP];         // elements
  int first[SINK_CAP + 1];    // first[e] = chunks of the ranges before e; first[n] = grid size
  unsigned long bf16;         // bit e: source e is bf16 (else fp32)
  int n;
};

__device__ __forceinline__ float sink_cvt(float v) { return v; }
__device__ __forceinline__ float sink_cvt(unsigned short h) {
  return __uint_as_float((unsigned)h << 16);
}

// 16 bytes of source -> 16 / sizeof(T) floats
__device__ __forceinline__ void sink_vec(float4 *dst, const float *src, bool aligned) {
  if (aligned) {
    dst[0] = *(const float4 *)src;
  } else {
    dst[0] = make_float4(src[0], src[1], src[2], src[3]);
  }
}
__device__ __forceinline__ void sink_vec(float4 *dst, const unsigned short *src, bool aligned) {
  unsigned short h[8];
  if (aligned) {
    uint4 v = *(const uint4 *)src;
    unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      h[2 * k] = (unsigned short)(w[k] & 0xffffu);
      h[2 * k + 1] = (unsigned short)(w[k] >> 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = src[k];
  }
  dst[0] = make_float4(sink_cvt(h[0]), sink_cvt(h[1]), sink_cvt(h[2]), sink_cvt(h[3]));
  dst[1] = make_float4(sink_cvt(h[4]), sink_cvt(h[5]), sink_cvt(h[6]), sink_cvt(h[7]));
}

// Elements [start, end) of one range: dst and src point at the range's element 0.  T is
// float or unsigned short (bf16 bits); src == nullptr zero-fills.
template <typename T>
__device__ __forceinline__ void sink_chunk(float *__restrict__ dst, const T *__restrict__ src,
                                           long start, long end) {
  constexpr int V = 16 / sizeof(T);  // elements per 16-byte load: 4 or 8 (whole float4 stores)
  // head: up to the destination's first 16-byte boundary at or after `start`
  long head = start + (long)((4 - (((uintptr_t)(dst + start) >> 2) & 3)) & 3);
  if (head > end) head = end;
  long nvec = (end - head) / V;
  long tail = head + nvec * V;
  if (src == nullptr) {
    for (long i = start + threadIdx.x; i < head; i += NTHREADS) dst[i] = 0.f;
    float4 *d4 = (float4 *)(dst + head);
    for (long v = threadIdx.x; v < nvec * (V / 4); v += NTHREADS) d4[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long i = tail + threadIdx.x; i < end; i += NTHREADS) dst[i] = 0.f;
    return;
  }
  for (long i = start + threadIdx.x; i < head; i += NTHREADS) dst[i] = sink_cvt(src[i]);
  bool aligned = ((uintptr_t)(src + head) & 15) == 0;  // the same for every lane of the block
  for (long v = threadIdx.x; v < nvec; v += NTHREADS)
    sink_vec((float4 *)(dst + head + v * V), src + head + v * V, aligned);
  for (long i = tail + threadIdx.x; i < end; i += NTHREADS) dst[i] = sink_cvt(src[i]);
}

__global__ void __launch_bounds__(NTHREADS)
k_scatter_grads(float *__restrict__ out, const SinkTable t) {
  // the range e with first[e] <= blockIdx.x < first[e + 1] (ranges are never empty)
  int b = (int)blockIdx.x;
  int lo = 0, hi = t.n - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (t.first[mid] <= b) lo = mid; else hi = mid - 1;
  }
  long start = (long)(b - t.first[lo]) * SINK_CHUNK;
  long len = t.len[lo];
  long end = start + SINK_CHUNK < len ? start + SINK_CHUNK : len;
  float *dst = out + t.off[lo];
  if ((t.bf16 >> lo) & 1ul) sink_chunk(dst, (const unsigned short *)t.src[lo], start, end);
  else sink_chunk(dst, (const float *)t.src[lo], start, end);
}

// srcs[i] -> out[offsets[i] : offsets[i] + srcs[i].numel()).  The ranges [skip_off[j],
// skip_off[j] + skip_len[j]) are the caller's: it writes them itself (a source that is not
// dense in the flat order goes through a strided copy there), so they are neither written
// nor zeroed here.  Everything outside both lists becomes +0.0.
void scatter_grads(std::vector<torch::Tensor> srcs, std::vector<int64_t> offsets,
                   std::vector<int64_t> skip_off, std::vector<int64_t> skip_len,
                   torch::Tensor out) {
  CHECK_IN(out);
  TORCH_CHECK(out.scalar_type() == torch::kFloat32 && out.dim() == 1,
              "scatter_grads: out must be a 1-D fp32 row");
  TORCH_CHECK(srcs.size() == offsets.size(), "scatter_grads: ", srcs.size(), " sources, ",
              offsets.size(), " offsets");
  TORCH_CHECK(skip_off.size() == skip_len.size(), "scatter_grads: skip lists differ in length");
  long d = out.numel();
  if (d == 0) {
    TORCH_CHECK(srcs.empty() && skip_off.empty(), "scatter_grads: ranges beyond an empty out");
    return;
  }
  float *op = out.data_ptr<float>();
  TORCH_CHECK((uintptr_t)op % 16 == 0, "scatter_grads: out must be 16-byte aligned");

  struct Range { long off, len; const void *src; bool bf16; bool skip; };
  std::vector<Range> ranges;
  for (size_t i = 0; i < srcs.size(); ++i) {
    const torch::Tensor &s = srcs[i];
    TORCH_CHECK(s.is_cuda() && s.device() == out.device(), "scatter_grads: source ", i,
                " must be on out's device");
    bool bf = s.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(bf || s.scalar_type() == torch::kFloat32, "scatter_grads: source ", i,
                " must be fp32 or bf16");
    TORCH_CHECK(s.is_non_overlapping_and_dense(), "scatter_grads: source ", i,
                " must be dense");
    if (s.numel() == 0) continue;
    ranges.push_back({offsets[i], s.numel(), s.data_ptr(), bf, false});
  }
  for (size_t j = 0; j < skip_off.size(); ++j)
    if (skip_len[j] != 0) ranges.push_back({skip_off[j], skip_len[j], nullptr, false, true});
  std::sort(ranges.begin(), ranges.end(),
            [](const Range &a, const Range &b) { return a.off < b.off; });
  long pos = 0;
  for (const Range &r : ranges) {
    TORCH_CHECK(r.len > 0 && r.off >= 0 && r.off <= d && r.len <= d - r.off,
                "scatter_grads: range [", r.off, ", ", r.off + r.len, ") beyond out's ", d,
                " elements");
    TORCH_CHECK(r.off >= pos, "scatter_grads: range [", r.off, ", ", r.off + r.len,
                ") overlaps the one before it");
    pos = r.off + r.len;
  }

  SinkTable t;
  t.n = 0; t.bf16 = 0; t.first[0] = 0;
  auto flush = [&]() {
    if (t.n == 0) return;
    launch(k_scatter_grads, dim3(t.first[t.n]), 0, op, t);
    t.n = 0; t.bf16 = 0;
  };
  auto push = [&](long off, long len, const void *src, bool bf) {
    // a range of more chunks than a grid may have blocks is split
    const long max_len = (long)(1 << 20) * SINK_CHUNK;
    while (len > 0) {
      long n = len < max_len ? len : max_len;
      if (t.n == SINK_CAP) flush();
      int e = t.n++;
      t.src[e] = src; t.off[e] = off; t.len[e] = n;
      if (bf) t.bf16 |= 1ul << e;
      t.first[e + 1] = t.first[e] + (int)((n + SINK_CHUNK - 1) / SINK_CHUNK);
      if (src != nullptr) src = (const char *)src + n * (bf ? 2 : 4);
      off += n; len -= n;
      if (t.first[t.n] > (1 << 24)) flush();
    }
  };
  pos = 0;
  for (const Range &r : ranges) {
    if (r.off > pos) push(pos, r.off - pos, nullptr, false);  // the gap before it
    if (!r.skip) push(r.off, r.len, r.src, r.bf16);
    pos = r.off + r.len;
  }
  if (pos < d) push(pos, d - pos, nullptr, false);  // the pad tail
  flush();
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
  m.def("mix_rows", &mix_rows);
  m.def("sign_pack", &sign_pack);
  m.def("sign_majority", &sign_majority);
  m.def("mx8_pack", &mx8_pack);
  m.def("mx8_unpack", &mx8_unpack);
  m.def("mx8_column_trimmed_mean", &mx8_column_trimmed_mean);
  m.def("mx8_column_mean_around", &mx8_column_mean_around);
  m.def("mx8_clip_step", &mx8_clip_step);
  m.def("mx8_weiszfeld_step", &mx8_weiszfeld_step);
  m.def("mx8_segment_gram", &mx8_segment_gram);
  m.def("mx8_segment_mean_around", &mx8_segment_mean_around);
  m.def("mx4_pack", &mx4_pack);
  m.def("mx4_unpack", &mx4_unpack);
  m.def("mx4_column_trimmed_mean", &mx4_column_trimmed_mean);
  m.def("mx4_column_mean_around", &mx4_column_mean_around);
  m.def("scatter_grads", &scatter_grads);
}
