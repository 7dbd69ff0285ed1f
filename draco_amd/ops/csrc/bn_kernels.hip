// Training-mode BatchNorm2d fused with the residual add and ReLU that follow it in a
// ResNet block, for bf16 NHWC activations on MI355X (gfx950).
//
// An NHWC tensor is a row-major (M = N*H*W, C) matrix and BatchNorm is a per-column
// normalisation of it.  I/O is bf16; all arithmetic, gamma, beta, the saved and the
// running statistics are fp32.  Each direction is three launches:
//
//   forward   k_bn_fwd_stats     per-block (mean, M2) partials of x        reads x
//             k_bn_fwd_finalize  Chan-combine the partials; save_mean, save_invstd,
//                                running stats and num_batches_tracked     (tiny)
//             k_bn_fwd_apply     y = [relu]((x-mean)*invstd*gamma + beta [+ res])
//   backward  k_bn_bwd_stats     partial sums of dz and dz*xhat, dz = dy*(y>0);
//                                with a residual, dz is written once in bf16 and is
//                                the residual's gradient
//             k_bn_bwd_finalize  dgamma, dbeta                             (tiny)
//             k_bn_bwd_apply     dx = gamma*invstd*(dz - dbeta/M - xhat*dgamma/M)
//
// Tiling: a block is 8 x 32 threads; a thread owns 8 consecutive channels (one 16 B
// load), so 8 threads span a 64-channel tile and the block covers 32 rows per
// iteration.  blockIdx.x walks channel tiles, blockIdx.y row chunks; the grid is a
// function of (M, C) alone (bn_geom).  No atomics: partials go to a workspace that is
// fully written before it is read, and every reduction runs in a fixed order, so two
// calls on the same inputs give the same bits.
//
// Variance: a thread accumulates sum(x-K) and sum((x-K)^2) with K its own first row
// (a sample, so the subtraction cancels nothing that matters over its few rows),
// converts to (n, mean, M2), and from there on everything is combined with Chan's
// parallel formula — never E[x^2]-E[x]^2 over all rows.

#include <torch/extension.h>
#include <c10/hip/HIPException.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#define BN_THREADS 256
#define BN_TX 8        // threads across one 64-channel tile
#define BN_TY 32       // rows per block iteration
#define BN_TILE_C 64   // channels per tile
#define BN_UNROLL 4    // rows in flight per thread
#define BN_BLOCKS 1024 // target blocks per streaming launch
#define BN_FIN_C 16    // finalize: channels per block
#define BN_FIN_L 16    // finalize: chunk lanes per block

static inline hipStream_t bn_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

struct BnGeom {
  int M, C;
  int rpc;     // rows per chunk (a multiple of BN_TY)
  int chunks;  // row chunks, none empty
  int ctiles;  // 64-channel tiles
};

static BnGeom bn_geom(long M, long C) {
  BnGeom g;
  g.M = (int)M;
  g.C = (int)C;
  g.ctiles = (int)((C + BN_TILE_C - 1) / BN_TILE_C);
  long want = BN_BLOCKS / g.ctiles;
  if (want < 1) want = 1;
  long c0 = (M + BN_TY - 1) / BN_TY;
  if (c0 > want) c0 = want;
  long rpc = (M + c0 - 1) / c0;
  rpc = (rpc + BN_TY - 1) / BN_TY * BN_TY;
  g.rpc = (int)rpc;
  g.chunks = (int)((M + rpc - 1) / rpc);
  return g;
}

// ------------------------------------------------------------------ bf16 <-> fp32
__device__ __forceinline__ void bn_unpack8(const uint4 v, float f[8]) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ unsigned bn_f2bf(float f) {  // round to nearest even
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

__device__ __forceinline__ uint4 bn_pack8(const float f[8]) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = bn_f2bf(f[2 * i]) | (bn_f2bf(f[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void bn_load8(const float *__restrict__ p, float f[8]) {
  const float4 a = *reinterpret_cast<const float4 *>(p);
  const float4 b = *reinterpret_cast<const float4 *>(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

__device__ __forceinline__ void bn_store8(float *__restrict__ p, const float f[8]) {
  *reinterpret_cast<float4 *>(p) = make_float4(f[0], f[1], f[2], f[3]);
  *reinterpret_cast<float4 *>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

// Chan: fold (nb, mb, m2b) into (na, ma, m2a); nb > 0.
__device__ __forceinline__ void bn_chan(float &na, float &ma, float &m2a, float nb, float mb,
                                        float m2b) {
  const float n = na + nb;
  const float w = nb / n;
  const float delta = mb - ma;
  ma = fmaf(delta, w, ma);
  m2a = m2a + m2b + delta * delta * na * w;
  na = n;
}

// ------------------------------------------------------------------ forward stats
__global__ void __launch_bounds__(BN_THREADS)
k_bn_fwd_stats(const uint4 *__restrict__ x, int M, int C, int rpc,
               float *__restrict__ p_mean, float *__restrict__ p_m2) {
  __shared__ float s_mean[BN_TY][BN_TILE_C];
  __shared__ float s_m2[BN_TY][BN_TILE_C];
  __shared__ float s_n[BN_TY];
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c0 = blockIdx.x * BN_TILE_C + tx * 8;
  const bool cok = c0 < C;
  const int row0 = blockIdx.y * rpc;
  const int row1 = min(M, row0 + rpc);
  const size_t C8 = (size_t)(C / 8);

  float K[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { K[j] = 0.f; s1[j] = 0.f; s2[j] = 0.f; }
  int n = 0;
  if (cok) {
    const uint4 *xp = x + c0 / 8;
    for (int r = row0 + ty; r < row1; r += BN_TY * BN_UNROLL) {
      uint4 v[BN_UNROLL];
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) {
        const int rr = r + u * BN_TY;
        if (rr < row1) v[u] = xp[(size_t)rr * C8];
      }
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) {
        const int rr = r + u * BN_TY;
        if (rr < row1) {
          float f[8];
          bn_unpack8(v[u], f);
          if (n == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) K[j] = f[j];
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float d = f[j] - K[j];
            s1[j] += d;
            s2[j] = fmaf(d, d, s2[j]);
          }
          ++n;
        }
      }
    }
  }
  float fn = (float)n, mean[8], m2[8];
  {
    const float inv = n > 0 ? 1.f / fn : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mean[j] = fmaf(s1[j], inv, K[j]);
      m2[j] = fmaxf(s2[j] - s1[j] * s1[j] * inv, 0.f);
    }
  }
  // fixed-order tree over the 32 row lanes; a lane keeps its own node in registers
  // and publishes it for the step at which it becomes the partner
  bn_store8(&s_mean[ty][tx * 8], mean);
  bn_store8(&s_m2[ty][tx * 8], m2);
  if (tx == 0) s_n[ty] = fn;
  for (int s = BN_TY / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (ty < s) {
      const float nb = s_n[ty + s];
      if (nb > 0.f) {
        float mb[8], m2b[8];
        bn_load8(&s_mean[ty + s][tx * 8], mb);
        bn_load8(&s_m2[ty + s][tx * 8], m2b);
        float nn = fn;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          nn = fn;
          bn_chan(nn, mean[j], m2[j], nb, mb[j], m2b[j]);
        }
        fn = nn;
        bn_store8(&s_mean[ty][tx * 8], mean);
        bn_store8(&s_m2[ty][tx * 8], m2);
        if (tx == 0) s_n[ty] = fn;
      }
    }
  }
  if (ty == 0 && cok) {
    const size_t o = (size_t)blockIdx.y * C + c0;
    bn_store8(p_mean + o, mean);
    bn_store8(p_m2 + o, m2);
  }
}

// ------------------------------------------------------------------ forward finalize
__global__ void __launch_bounds__(BN_THREADS)
k_bn_fwd_finalize(const float *__restrict__ p_mean, const float *__restrict__ p_m2, int M, int C,
                  int rpc, int chunks, float *__restrict__ save_mean,
                  float *__restrict__ save_invstd, float *__restrict__ running_mean,
                  float *__restrict__ running_var, long *__restrict__ num_batches_tracked,
                  float momentum, float eps) {
  __shared__ float s_mean[BN_FIN_L][BN_FIN_C];
  __shared__ float s_m2[BN_FIN_L][BN_FIN_C];
  __shared__ float s_n[BN_FIN_L][BN_FIN_C];
  const int tx = threadIdx.x % BN_FIN_C, ty = threadIdx.x / BN_FIN_C;
  const int c = blockIdx.x * BN_FIN_C + tx;
  const bool cok = c < C;
  float fn = 0.f, mean = 0.f, m2 = 0.f;
  if (cok) {
    for (int i = ty; i < chunks; i += BN_FIN_L) {
      const float nb = (float)min(rpc, M - i * rpc);
      bn_chan(fn, mean, m2, nb, p_mean[(size_t)i * C + c], p_m2[(size_t)i * C + c]);
    }
  }
  s_mean[ty][tx] = mean;
  s_m2[ty][tx] = m2;
  s_n[ty][tx] = fn;
  for (int s = BN_FIN_L / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (ty < s) {
      const float nb = s_n[ty + s][tx];
      if (nb > 0.f) {
        bn_chan(fn, mean, m2, nb, s_mean[ty + s][tx], s_m2[ty + s][tx]);
        s_mean[ty][tx] = mean;
        s_m2[ty][tx] = m2;
        s_n[ty][tx] = fn;
      }
    }
  }
  if (ty == 0 && cok) {
    const float var = m2 / (float)M;
    save_mean[c] = mean;
    save_invstd[c] = 1.f / sqrtf(var + eps);
    const float unbiased = m2 / (float)(M - 1);
    running_mean[c] = fmaf(momentum, mean - running_mean[c], running_mean[c]);
    running_var[c] = fmaf(momentum, unbiased - running_var[c], running_var[c]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *num_batches_tracked += 1;
}

// ------------------------------------------------------------------ forward apply
template <bool RELU, bool RES>
__global__ void __launch_bounds__(BN_THREADS)
k_bn_fwd_apply(const uint4 *__restrict__ x, const uint4 *__restrict__ res, uint4 *__restrict__ y,
               const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
               const float *__restrict__ gamma, const float *__restrict__ beta, int M, int C,
               int rpc) {
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c0 = blockIdx.x * BN_TILE_C + tx * 8;
  if (c0 >= C) return;
  const int row0 = blockIdx.y * rpc;
  const int row1 = min(M, row0 + rpc);
  const size_t C8 = (size_t)(C / 8);
  float mean[8], scale[8], shift[8];
  bn_load8(save_mean + c0, mean);
  bn_load8(save_invstd + c0, scale);
  bn_load8(gamma + c0, shift);
#pragma unroll
  for (int j = 0; j < 8; ++j) scale[j] *= shift[j];
  bn_load8(beta + c0, shift);
  const size_t cv = (size_t)(c0 / 8);
  for (int r = row0 + ty; r < row1; r += BN_TY * BN_UNROLL) {
    uint4 v[BN_UNROLL], w[BN_UNROLL];
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      const int rr = r + u * BN_TY;
      if (rr < row1) {
        v[u] = x[(size_t)rr * C8 + cv];
        if (RES) w[u] = res[(size_t)rr * C8 + cv];
      }
    }
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      const int rr = r + u * BN_TY;
      if (rr < row1) {
        float f[8], g[8];
        bn_unpack8(v[u], f);
        if (RES) bn_unpack8(w[u], g);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float o = fmaf(f[j] - mean[j], scale[j], shift[j]);
          if (RES) o += g[j];
          if (RELU) o = o < 0.f ? 0.f : o;  // keeps NaN, as torch's relu does
          f[j] = o;
        }
        y[(size_t)rr * C8 + cv] = bn_pack8(f);
      }
    }
  }
}

// ------------------------------------------------------------------ backward stats
template <bool RELU, bool WRITE_DZ>
__global__ void __launch_bounds__(BN_THREADS)
k_bn_bwd_stats(const uint4 *__restrict__ dy, const uint4 *__restrict__ x,
               const uint4 *__restrict__ y, uint4 *__restrict__ dz_out,
               const float *__restrict__ save_mean, const float *__restrict__ save_invstd, int M,
               int C, int rpc, float *__restrict__ p_db, float *__restrict__ p_dg) {
  __shared__ float s_db[BN_TY][BN_TILE_C];
  __shared__ float s_dg[BN_TY][BN_TILE_C];
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c0 = blockIdx.x * BN_TILE_C + tx * 8;
  const bool cok = c0 < C;
  const int row0 = blockIdx.y * rpc;
  const int row1 = min(M, row0 + rpc);
  const size_t C8 = (size_t)(C / 8);
  float db[8], dg[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { db[j] = 0.f; dg[j] = 0.f; }
  if (cok) {
    float mean[8], invstd[8];
    bn_load8(save_mean + c0, mean);
    bn_load8(save_invstd + c0, invstd);
    const size_t cv = (size_t)(c0 / 8);
    for (int r = row0 + ty; r < row1; r += BN_TY * BN_UNROLL) {
      uint4 a[BN_UNROLL], b[BN_UNROLL], m[BN_UNROLL];
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) {
        const int rr = r + u * BN_TY;
        if (rr < row1) {
          a[u] = dy[(size_t)rr * C8 + cv];
          b[u] = x[(size_t)rr * C8 + cv];
          if (RELU) m[u] = y[(size_t)rr * C8 + cv];
        }
      }
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) {
        const int rr = r + u * BN_TY;
        if (rr < row1) {
          float g[8], f[8], o[8];
          bn_unpack8(a[u], g);
          bn_unpack8(b[u], f);
          if (RELU) {
            bn_unpack8(m[u], o);
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = o[j] > 0.f ? g[j] : 0.f;
          }
          if (WRITE_DZ) dz_out[(size_t)rr * C8 + cv] = bn_pack8(g);  // exact: dy or 0
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            db[j] += g[j];
            dg[j] = fmaf(g[j], (f[j] - mean[j]) * invstd[j], dg[j]);
          }
        }
      }
    }
  }
  bn_store8(&s_db[ty][tx * 8], db);
  bn_store8(&s_dg[ty][tx * 8], dg);
  for (int s = BN_TY / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (ty < s) {
      float t0[8], t1[8];
      bn_load8(&s_db[ty + s][tx * 8], t0);
      bn_load8(&s_dg[ty + s][tx * 8], t1);
#pragma unroll
      for (int j = 0; j < 8; ++j) { db[j] += t0[j]; dg[j] += t1[j]; }
      bn_store8(&s_db[ty][tx * 8], db);
      bn_store8(&s_dg[ty][tx * 8], dg);
    }
  }
  if (ty == 0 && cok) {
    const size_t o = (size_t)blockIdx.y * C + c0;
    bn_store8(p_db + o, db);
    bn_store8(p_dg + o, dg);
  }
}

// ------------------------------------------------------------------ backward finalize
__global__ void __launch_bounds__(BN_THREADS)
k_bn_bwd_finalize(const float *__restrict__ p_db, const float *__restrict__ p_dg, int C,
                  int chunks, float *__restrict__ dgamma, float *__restrict__ dbeta) {
  __shared__ float s_db[BN_FIN_L][BN_FIN_C];
  __shared__ float s_dg[BN_FIN_L][BN_FIN_C];
  const int tx = threadIdx.x % BN_FIN_C, ty = threadIdx.x / BN_FIN_C;
  const int c = blockIdx.x * BN_FIN_C + tx;
  const bool cok = c < C;
  float db = 0.f, dg = 0.f;
  if (cok) {
    for (int i = ty; i < chunks; i += BN_FIN_L) {
      db += p_db[(size_t)i * C + c];
      dg += p_dg[(size_t)i * C + c];
    }
  }
  s_db[ty][tx] = db;
  s_dg[ty][tx] = dg;
  for (int s = BN_FIN_L / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (ty < s) {
      db += s_db[ty + s][tx];
      dg += s_dg[ty + s][tx];
      s_db[ty][tx] = db;
      s_dg[ty][tx] = dg;
    }
  }
  if (ty == 0 && cok) {
    dbeta[c] = db;
    dgamma[c] = dg;
  }
}

// ------------------------------------------------------------------ backward apply
// RELU: dz is formed here from dy and the saved output y; otherwise `dz` already is dz
// (no activation, or the bf16 dz that k_bn_bwd_stats wrote for the residual).
template <bool RELU>
__global__ void __launch_bounds__(BN_THREADS)
k_bn_bwd_apply(const uint4 *__restrict__ dz, const uint4 *__restrict__ x,
               const uint4 *__restrict__ y, uint4 *__restrict__ dx,
               const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
               const float *__restrict__ gamma, const float *__restrict__ dgamma,
               const float *__restrict__ dbeta, int M, int C, int rpc) {
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c0 = blockIdx.x * BN_TILE_C + tx * 8;
  if (c0 >= C) return;
  const int row0 = blockIdx.y * rpc;
  const int row1 = min(M, row0 + rpc);
  const size_t C8 = (size_t)(C / 8);
  const float inv_m = 1.f / (float)M;
  float mean[8], invstd[8], gs[8], kb[8], kg[8];
  bn_load8(save_mean + c0, mean);
  bn_load8(save_invstd + c0, invstd);
  bn_load8(gamma + c0, gs);
  bn_load8(dbeta + c0, kb);
  bn_load8(dgamma + c0, kg);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    gs[j] *= invstd[j];
    kb[j] *= inv_m;
    kg[j] *= inv_m;
  }
  const size_t cv = (size_t)(c0 / 8);
  for (int r = row0 + ty; r < row1; r += BN_TY * BN_UNROLL) {
    uint4 a[BN_UNROLL], b[BN_UNROLL], m[BN_UNROLL];
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      const int rr = r + u * BN_TY;
      if (rr < row1) {
        a[u] = dz[(size_t)rr * C8 + cv];
        b[u] = x[(size_t)rr * C8 + cv];
        if (RELU) m[u] = y[(size_t)rr * C8 + cv];
      }
    }
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      const int rr = r + u * BN_TY;
      if (rr < row1) {
        float g[8], f[8], o[8];
        bn_unpack8(a[u], g);
        bn_unpack8(b[u], f);
        if (RELU) bn_unpack8(m[u], o);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float d = g[j];
          if (RELU) d = o[j] > 0.f ? d : 0.f;
          const float xh = (f[j] - mean[j]) * invstd[j];
          g[j] = gs[j] * (d - kb[j] - xh * kg[j]);
        }
        dx[(size_t)rr * C8 + cv] = bn_pack8(g);
      }
    }
  }
}

// ------------------------------------------------------------------ host side
static void bn_check_act(const at::Tensor &t, const char *name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 4, name, " must be 4D (N, C, H, W)");
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast),
              name, " must be dense in channels_last");
}

static void bn_check_vec(const at::Tensor &t, long C, const char *name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
  TORCH_CHECK(t.dim() == 1 && t.size(0) == C && t.is_contiguous(),
              name, " must be a contiguous vector of C=", C, " elements");
}

static BnGeom bn_check_shape(const at::Tensor &x) {
  const long C = x.size(1);
  const long M = x.numel() / (C > 0 ? C : 1);
  TORCH_CHECK(C > 0 && C % 8 == 0, "fused BN needs C to be a multiple of 8, got ", C);
  TORCH_CHECK(M >= 2, "fused BN needs at least 2 values per channel, got ", M);
  TORCH_CHECK(x.numel() < (1L << 31), "fused BN supports fewer than 2^31 elements");
  return bn_geom(M, C);
}

// y, save_mean, save_invstd; running_mean / running_var / num_batches_tracked are
// updated in place.  residual: empty tensor = none.
std::vector<at::Tensor> bn_act_forward(const at::Tensor &x, const at::Tensor &residual,
                                       const at::Tensor &gamma, const at::Tensor &beta,
                                       at::Tensor running_mean, at::Tensor running_var,
                                       at::Tensor num_batches_tracked, double momentum,
                                       double eps, bool relu) {
  bn_check_act(x, "x");
  const BnGeom g = bn_check_shape(x);
  const bool has_res = residual.numel() > 0;
  if (has_res) {
    bn_check_act(residual, "residual");
    TORCH_CHECK(residual.sizes() == x.sizes(), "residual must have x's shape");
  }
  bn_check_vec(gamma, g.C, "gamma");
  bn_check_vec(beta, g.C, "beta");
  bn_check_vec(running_mean, g.C, "running_mean");
  bn_check_vec(running_var, g.C, "running_var");
  TORCH_CHECK(num_batches_tracked.is_cuda() && num_batches_tracked.numel() == 1 &&
                  num_batches_tracked.scalar_type() == torch::kInt64,
              "num_batches_tracked must be one int64 on GPU");

  auto y = at::empty(x.sizes(), x.options(), at::MemoryFormat::ChannelsLast);
  auto fopt = x.options().dtype(torch::kFloat32);
  auto save_mean = at::empty({g.C}, fopt);
  auto save_invstd = at::empty({g.C}, fopt);
  auto ws = at::empty({2, g.chunks, g.C}, fopt);
  float *p_mean = ws.data_ptr<float>();
  float *p_m2 = p_mean + (size_t)g.chunks * g.C;

  hipStream_t s = bn_stream();
  const dim3 grid(g.ctiles, g.chunks), block(BN_THREADS);
  const uint4 *xp = reinterpret_cast<const uint4 *>(x.data_ptr());
  const uint4 *rp = has_res ? reinterpret_cast<const uint4 *>(residual.data_ptr()) : nullptr;
  uint4 *yp = reinterpret_cast<uint4 *>(y.data_ptr());

  hipLaunchKernelGGL(k_bn_fwd_stats, grid, block, 0, s, xp, g.M, g.C, g.rpc, p_mean, p_m2);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bn_fwd_finalize, dim3((g.C + BN_FIN_C - 1) / BN_FIN_C), block, 0, s,
                     p_mean, p_m2, g.M, g.C, g.rpc, g.chunks, save_mean.data_ptr<float>(),
                     save_invstd.data_ptr<float>(), running_mean.data_ptr<float>(),
                     running_var.data_ptr<float>(),
                     reinterpret_cast<long *>(num_batches_tracked.data_ptr<int64_t>()),
                     (float)momentum, (float)eps);
  C10_HIP_KERNEL_LAUNCH_CHECK();
#define BN_FWD_APPLY(RELU, RES)                                                              \
  hipLaunchKernelGGL((k_bn_fwd_apply<RELU, RES>), grid, block, 0, s, xp, rp, yp,             \
                     save_mean.data_ptr<float>(), save_invstd.data_ptr<float>(),             \
                     gamma.data_ptr<float>(), beta.data_ptr<float>(), g.M, g.C, g.rpc)
  if (relu && has_res) BN_FWD_APPLY(true, true);
  else if (relu) BN_FWD_APPLY(true, false);
  else if (has_res) BN_FWD_APPLY(false, true);
  else BN_FWD_APPLY(false, false);
#undef BN_FWD_APPLY
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {y, save_mean, save_invstd};
}

// dx, dgamma, dbeta, dz.  dz (the residual's gradient) is a bf16 tensor when
// relu && want_dz, else an empty tensor: without ReLU the residual's gradient is dy.
std::vector<at::Tensor> bn_act_backward(const at::Tensor &dy, const at::Tensor &x,
                                        const at::Tensor &y, const at::Tensor &gamma,
                                        const at::Tensor &save_mean,
                                        const at::Tensor &save_invstd, bool relu, bool want_dz) {
  bn_check_act(x, "x");
  const BnGeom g = bn_check_shape(x);
  bn_check_act(dy, "dy");
  TORCH_CHECK(dy.sizes() == x.sizes(), "dy must have x's shape");
  if (relu) {
    bn_check_act(y, "y");
    TORCH_CHECK(y.sizes() == x.sizes(), "y must have x's shape");
  }
  bn_check_vec(gamma, g.C, "gamma");
  bn_check_vec(save_mean, g.C, "save_mean");
  bn_check_vec(save_invstd, g.C, "save_invstd");

  const bool write_dz = relu && want_dz;
  auto dx = at::empty(x.sizes(), x.options(), at::MemoryFormat::ChannelsLast);
  auto dz = write_dz ? at::empty(x.sizes(), x.options(), at::MemoryFormat::ChannelsLast)
                     : at::empty({0}, x.options());
  auto fopt = x.options().dtype(torch::kFloat32);
  auto dgamma = at::empty({g.C}, fopt);
  auto dbeta = at::empty({g.C}, fopt);
  auto ws = at::empty({2, g.chunks, g.C}, fopt);
  float *p_db = ws.data_ptr<float>();
  float *p_dg = p_db + (size_t)g.chunks * g.C;

  hipStream_t s = bn_stream();
  const dim3 grid(g.ctiles, g.chunks), block(BN_THREADS);
  const uint4 *dyp = reinterpret_cast<const uint4 *>(dy.data_ptr());
  const uint4 *xp = reinterpret_cast<const uint4 *>(x.data_ptr());
  const uint4 *yp = relu ? reinterpret_cast<const uint4 *>(y.data_ptr()) : nullptr;
  uint4 *dzp = write_dz ? reinterpret_cast<uint4 *>(dz.data_ptr()) : nullptr;
  uint4 *dxp = reinterpret_cast<uint4 *>(dx.data_ptr());

#define BN_BWD_STATS(RELU, WDZ)                                                              \
  hipLaunchKernelGGL((k_bn_bwd_stats<RELU, WDZ>), grid, block, 0, s, dyp, xp, yp, dzp,       \
                     save_mean.data_ptr<float>(), save_invstd.data_ptr<float>(), g.M, g.C,   \
                     g.rpc, p_db, p_dg)
  if (write_dz) BN_BWD_STATS(true, true);
  else if (relu) BN_BWD_STATS(true, false);
  else BN_BWD_STATS(false, false);
#undef BN_BWD_STATS
  C10_HIP_KERNEL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((g.C + BN_FIN_C - 1) / BN_FIN_C), block, 0, s,
                     p_db, p_dg, g.C, g.chunks, dgamma.data_ptr<float>(),
                     dbeta.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
#define BN_BWD_APPLY(RELU, SRC)                                                              \
  hipLaunchKernelGGL((k_bn_bwd_apply<RELU>), grid, block, 0, s, SRC, xp, yp, dxp,            \
                     save_mean.data_ptr<float>(), save_invstd.data_ptr<float>(),             \
                     gamma.data_ptr<float>(), dgamma.data_ptr<float>(),                      \
                     dbeta.data_ptr<float>(), g.M, g.C, g.rpc)
  if (write_dz) BN_BWD_APPLY(false, (const uint4 *)dzp);
  else if (relu) BN_BWD_APPLY(true, dyp);
  else BN_BWD_APPLY(false, dyp);
#undef BN_BWD_APPLY
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dx, dgamma, dbeta, dz};
}

// (M, C) -> rows per chunk, row chunks, channel tiles: the launch geometry, for tests
// and the bandwidth tool.
std::vector<long> bn_act_geometry(long M, long C) {
  TORCH_CHECK(C > 0 && C % 8 == 0 && M >= 2, "bn_act_geometry: need C % 8 == 0 and M >= 2");
  const BnGeom g = bn_geom(M, C);
  return {g.rpc, g.chunks, g.ctiles, BN_TY};
}

void register_bn_ops(pybind11::module &m) {
  m.def("bn_act_forward", &bn_act_forward);
  m.def("bn_act_backward", &bn_act_backward);
  m.def("bn_act_geometry", &bn_act_geometry);
}
