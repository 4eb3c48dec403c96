// N x N elementwise / reduction kernels of the attack step (HBM-bound).
//
// Every matrix is row-major fp32 with leading dimension ld (ld % 4 == 0,
// pad columns hold zeros).  Row kernels use one 256-thread block per row with
// 16-byte loads; reductions are deterministic (fixed trees, per-row partials
// reduced by a second single-block kernel) so that two runs on the same inputs
// give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace mcgra {

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define ROW_THREADS 256

// ---------------------------------------------------------------------------
// get_modified_adj (:365) + adding_noise (:474) + rowsum of normalize_adj (:218)
// A = clamp((i!=j) * M + ori + eps*noise, 0, 1); d = 1 + rowsum(A); r = d^-1/2.
// GENERAL=false: ori == 0, eps == 0 and 0 <= M <= 1, so A == M (no copy).
// ---------------------------------------------------------------------------
template <bool GENERAL>
__global__ __launch_bounds__(ROW_THREADS) void k_prep(int n, int ld, const float* __restrict__ M,
                                                      const float* __restrict__ ori,
                                                      const float* __restrict__ noise, float eps,
                                                      float* __restrict__ A, unsigned char* __restrict__ gate,
                                                      float* __restrict__ d, float* __restrict__ r,
                                                      double* __restrict__ rowsq, double* __restrict__ rowsum, int row0) {
  __shared__ float shf[16];
  __shared__ double shd[16];
  const int i = row0 + blockIdx.x;
  const size_t base = (size_t)i * ld;
  float s = 0.f;
  double sq = 0.0;
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    f32x4 m = *reinterpret_cast<const f32x4*>(M + base + j);
    f32x4 a = m;
    if (GENERAL) {
      f32x4 o = ori ? *reinterpret_cast<const f32x4*>(ori + base + j) : f32x4{0, 0, 0, 0};
      f32x4 z = (noise && eps != 0.f) ? *reinterpret_cast<const f32x4*>(noise + base + j) : f32x4{0, 0, 0, 0};
      unsigned char g[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int jj = j + t;
        float pre = (jj != i ? m[t] : 0.f) + o[t];
        if (noise && eps != 0.f) pre += z[t] * eps;
        g[t] = (pre >= 0.f && pre <= 1.f) ? 1 : 0;
        a[t] = jj < n ? fminf(fmaxf(pre, 0.f), 1.f) : 0.f;
      }
      *reinterpret_cast<f32x4*>(A + base + j) = a;
      *reinterpret_cast<uchar4*>(gate + base + j) = make_uchar4(g[0], g[1], g[2], g[3]);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int jj = j + t;
      if (jj < n) {
        s += a[t];
        if (jj != i) sq += (double)m[t] * (double)m[t];
      }
    }
  }
  const float tot = block_sum(s, shf);
  const double tsq = block_sum_d(sq, shd);
  if (threadIdx.x == 0) {
    const float di = tot + 1.0f;  // rowsum(A + I)
    float ri = 1.0f / sqrtf(di);
    if (isinf(ri)) ri = 0.f;      // r_inv[isinf] = 0 (utils.py:225)
    d[i] = di;
    r[i] = ri;
    rowsq[i] = tsq;
    rowsum[i] = (double)tot;
  }
}

// adj_norm = (r_i * (A + I)_ij) * r_j   (utils.py:226-228)
// rowsum (optional): row sums of the result in fp64 (same per-thread order as k_rowsum) -- the column means of the
// symmetric adj_norm for the centring of linear_HSIC, saving a pass over the matrix.
__global__ __launch_bounds__(ROW_THREADS) void k_adjn(int n, int ld, const float* __restrict__ A,
                                                      const float* __restrict__ r, float* __restrict__ out,
                                                      double* __restrict__ rowsum) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  const float ri = r[i];
  double s = 0;
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    f32x4 a = *reinterpret_cast<const f32x4*>(A + base + j);
    f32x4 rj = *reinterpret_cast<const f32x4*>(r + j);
    f32x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int jj = j + t;
      const float mx = a[t] + (jj == i ? 1.f : 0.f);
      o[t] = jj < n ? (ri * mx) * rj[t] : 0.f;
      s += (double)o[t];
    }
    *reinterpret_cast<f32x4*>(out + base + j) = o;
  }
  if (rowsum) {
    s = block_sum_d(s, shd);
    if (threadIdx.x == 0) rowsum[i] = s;
  }
}

// modified_adj1 = (1-I) * relu(Zn Zn^T) (+ ori)   (:187-188), in place on S.
// nmask (optional): number of off-diagonal pairs with S_ij <= 0, i.e. pairs the relu masks in the backward
// (integer atomics: order-independent, so still deterministic).
__global__ __launch_bounds__(ROW_THREADS) void k_decode_post(int n, int ld, float* __restrict__ S,
                                                             const float* __restrict__ ori,
                                                             unsigned int* __restrict__ nmask) {
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  int masked = 0;
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    f32x4 s = *reinterpret_cast<f32x4*>(S + base + j);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int jj = j + t;
      if (jj != i && jj < n && !(s[t] > 0.f)) ++masked;
      float v = (jj != i && jj < n) ? fmaxf(s[t], 0.f) : 0.f;
      if (ori && jj < n) v += ori[base + jj];
      s[t] = v;
    }
    *reinterpret_cast<f32x4*>(S + base + j) = s;
  }
  if (nmask) {      // one atomic per row (an ELU embedding masks pairs in every wave: per-wave adds to the one address were 130 us at n = 3312)
    __shared__ int wsum[ROW_THREADS / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) masked += __shfl_xor(masked, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = masked;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
#pragma unroll
      for (int w = 0; w < ROW_THREADS / 64; ++w) t += wsum[w];
      if (t) atomicAdd(nmask, (unsigned int)t);
    }
  }
}

// ---------------------------------------------------------------------------
// Elementwise loss terms on (adj_norm, modified_adj1, feature_adj):
//   c1 = calc(feature_adj, adj_norm) (:212)   c2 = calc(adj_norm, A1) (:221)
//   c6 = Info_entropy(adj_norm) (:230)        c7 = Info_entropy(A1) (:233)
// MSE: value and gradient are elementwise.  Other measures: only the entropy
// terms are handled here; their calc() parts come from GEMMs.
// kmse1/kmse2 are the full scalar multipliers (w * align * 2/n^2), 0 to skip.
// rowvals[4][n]: per-row partials of sum (f-x)^2, (x-y)^2, q log2 q (x), (y).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ROW_THREADS) void k_loss_elem(
    int n, int ld, const float* __restrict__ X, const float* __restrict__ Y,
    const float* __restrict__ F, float kmse1, float kmse2, float kie6, float kie7,
    float* __restrict__ GX, float* __restrict__ GY, double* __restrict__ rowvals) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  double v1 = 0, v2 = 0, v6 = 0, v7 = 0;
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(X + base + j);
    f32x4 y = {0, 0, 0, 0};
    if (Y) y = *reinterpret_cast<const f32x4*>(Y + base + j);      // Y == nullptr: X-side terms only
    f32x4 f = {0, 0, 0, 0};
    if (kmse1 != 0.f) f = *reinterpret_cast<const f32x4*>(F + base + j);
    f32x4 gx, gy;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float a = 0.f, b = 0.f;
      if (j + t < n) {
        if (kmse1 != 0.f) { const float e = f[t] - x[t]; v1 += (double)e * e; a -= kmse1 * e; }
        if (kmse2 != 0.f) { const float e = x[t] - y[t]; v2 += (double)e * e; a += kmse2 * e; b -= kmse2 * e; }
        if (kie6 != 0.f) { float v, g; ie_term(x[t], kie6, v, g); v6 += v; a += g; }
        if (kie7 != 0.f && Y) { float v, g; ie_term(y[t], kie7, v, g); v7 += v; b += g; }
      }
      gx[t] = a; gy[t] = b;
    }
    *reinterpret_cast<f32x4*>(GX + base + j) = gx;
    if (GY) *reinterpret_cast<f32x4*>(GY + base + j) = gy;
  }
  v1 = block_sum_d(v1, shd); v2 = block_sum_d(v2, shd);
  v6 = block_sum_d(v6, shd); v7 = block_sum_d(v7, shd);
  if (threadIdx.x == 0) {
    rowvals[i] = v1; rowvals[(size_t)n + i] = v2;
    rowvals[2 * (size_t)n + i] = v6; rowvals[3 * (size_t)n + i] = v7;
  }
}

// out[k] = sum_i rowvals[k][i]; one block per vector, deterministic.
__global__ __launch_bounds__(1024) void k_reduce_rows(const double* __restrict__ rowvals, int n,
                                                      double* __restrict__ out) {
  __shared__ double shd[16];
  const double* v = rowvals + (size_t)blockIdx.x * n;
  double s = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += v[i];
  s = block_sum_d(s, shd);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// row sums of a matrix (double partial per row) - Gram centering (utils.py:1060)
__global__ __launch_bounds__(ROW_THREADS) void k_rowsum(int n, int ld, const float* __restrict__ K,
                                                        double* __restrict__ rows) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  double s = 0;
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    const f32x4 k = *reinterpret_cast<const f32x4*>(K + base + j);
#pragma unroll
    for (int t = 0; t < 4; ++t) if (j + t < n) s += k[t];
  }
  s = block_sum_d(s, shd);
  if (threadIdx.x == 0) rows[i] = s;
}

// In-place Gram centering: K <- K - rm_i - rm_j + tm   (H K H of utils.py:1065;
// Gram matrices are symmetric so column means equal row means).
__global__ __launch_bounds__(ROW_THREADS) void k_center(int n, int ld, float* __restrict__ K,
                                                        const double* __restrict__ rows,
                                                        const double* __restrict__ total) {
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  const double inv = 1.0 / n;
  const double rmi = rows[i] * inv, tm = total[0] * inv * inv;
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    f32x4 k = *reinterpret_cast<f32x4*>(K + base + j);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      k[t] = (j + t < n) ? (float)((double)k[t] - rmi - rows[j + t] * inv + tm) : 0.f;
    *reinterpret_cast<f32x4*>(K + base + j) = k;
  }
}

// Column-centre a symmetric matrix: out_ij = X_ij - colmean_j, colmean_j = rows[j] / n
// (row sums == column sums by symmetry).  H X of CudaCKA.centering (utils.py:1060-1065):
// H X X^T H = (H X)(H X)^T, so the centred Gram is formed from centred operands.  This is the
// same matrix as centring the Gram afterwards, but the fp32 GEMM then sums zero-mean products
// instead of cancelling an O(n) mean (measured on Cora's feature_adj: 3e-7 vs 2e-4 relative).
// rowsq (optional): |row|^2 of the centred result in fp64 (diag of the centred Gram, lowrank_kernels.hip).
// The column means arrive as fp32 (k_colmean_f32: fp64 sum / n rounded once), so the pass is pure fp32 streaming.
__global__ void k_colmean_f32(int n, int ld, const double* __restrict__ colsum, float* __restrict__ mean,
                              unsigned* __restrict__ absmax) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (absmax && j == 0) *absmax = 0u;      // reset for k_center_cols' atomicMax (next launch on the stream)
  if (j < ld) mean[j] = j < n ? (float)(colsum[j] / (double)n) : 0.f;
}
__global__ __launch_bounds__(ROW_THREADS) void k_center_cols(int n, int ld, const float* __restrict__ X,
                                                             const float* __restrict__ mean,
                                                             float* __restrict__ out, double* __restrict__ rowsq,
                                                             unsigned* __restrict__ absmax) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, amx = 0.f;
  double s = 0;
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    f32x4 x = *reinterpret_cast<const f32x4*>(X + base + j);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + j);      // padded with zeros to ld
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = (j + t < n) ? x[t] - mu[t] : 0.f;
    s0 = fmaf(x[0], x[0], s0); s1 = fmaf(x[1], x[1], s1); s2 = fmaf(x[2], x[2], s2); s3 = fmaf(x[3], x[3], s3);
    amx = fmaxf(fmaxf(amx, fmaxf(fabsf(x[0]), fabsf(x[1]))), fmaxf(fabsf(x[2]), fabsf(x[3])));
    *reinterpret_cast<f32x4*>(out + base + j) = x;
  }
  if (absmax) {     // largest |xc| (operand scale of the 2-plane fp16 split); non-negative floats order as uints
    __shared__ float shm[16];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amx = fmaxf(amx, __shfl_xor(amx, o));
    if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = amx;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < ROW_THREADS / 64; ++w) amx = fmaxf(amx, shm[w]);
      // one atomic per row at most, and none once the running maximum already covers this row (the atomics of
      // 10 000 blocks on one address cost 0.28 ms otherwise)
      const unsigned bits = __float_as_uint(amx);
      if (bits > __hip_atomic_load(absmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(absmax, bits);
    }
  }
  if (rowsq) {      // <= ceil(n / 1024) fp32 terms per partial, then fp64
    s = (double)s0 + (double)s1 + (double)s2 + (double)s3;
    s = block_sum_d(s, shd);
    if (threadIdx.x == 0) rowsq[i] = s;
  }
}

// linear_HSIC on N x N operands (utils.py:1085-1089), value + left factors of
// the gradient GEMMs.  KX = Xc Xc^T, KY = Yc Yc^T (centred Grams), KFC = centred
// Gram of feature_adj (constant).  On exit
//   KY <- 2*(s1*KFC + s2*KY)   so that  G_X += KY @ Xc
//   KX <- 2*s2*KX              so that  G_Y += KX @ Yc
// rowvals[0][i] = sum_j KFC_ij*KX_ij (c1), rowvals[1][i] = sum_j KX_ij*KY_ij (c2).
__global__ __launch_bounds__(ROW_THREADS) void k_hsic_combine(
    int n, int ld, float* __restrict__ KX, float* __restrict__ KY, const float* __restrict__ KFC,
    float s1, float s2, double* __restrict__ rowvals, int lower, unsigned* __restrict__ amax_kx, unsigned* __restrict__ amax_ky) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  double v1 = 0, v2 = 0;
  float mxa = 0.f, mxb = 0.f;     // largest magnitudes of the two results (operand scales of the fp16 split, optional)
  // lower != 0: KX / KY are in lower tile storage (common.h).  Only that region is read and
  // written; tiles left of the diagonal tile stand for their mirror image too (weight 2).
  const int jdiag = lower ? (i / SYM_TILE) * SYM_TILE : 0;
  const int jend = lower ? min(n, jdiag + SYM_TILE) : n;
  for (int j = threadIdx.x * 4; j < jend; j += ROW_THREADS * 4) {
    const double wgt = (lower && j < jdiag) ? 2.0 : 1.0;
    f32x4 kx = *reinterpret_cast<f32x4*>(KX + base + j);
    f32x4 ky = {0, 0, 0, 0}, kf = {0, 0, 0, 0};
    if (s2 != 0.f) ky = *reinterpret_cast<f32x4*>(KY + base + j);
    if (s1 != 0.f) kf = *reinterpret_cast<const f32x4*>(KFC + base + j);
    f32x4 ox, oy;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float a = 0.f, b = 0.f;
      if (j + t < n) {
        v1 += wgt * ((double)kf[t] * kx[t]);
        v2 += wgt * ((double)kx[t] * ky[t]);
        a = 2.f * s2 * kx[t];
        b = 2.f * (s1 * kf[t] + s2 * ky[t]);
      }
      ox[t] = a; oy[t] = b;
      mxa = fmaxf(mxa, fabsf(a)); mxb = fmaxf(mxb, fabsf(b));
    }
    *reinterpret_cast<f32x4*>(KX + base + j) = ox;
    *reinterpret_cast<f32x4*>(KY + base + j) = oy;
  }
  v1 = block_sum_d(v1, shd); v2 = block_sum_d(v2, shd);
  if (threadIdx.x == 0) { rowvals[i] = v1; rowvals[(size_t)n + i] = v2; }
  if (amax_kx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mxa = fmaxf(mxa, __shfl_xor(mxa, o)); mxb = fmaxf(mxb, __shfl_xor(mxb, o)); }
    if ((threadIdx.x & 63) == 0) {      // non-negative floats order as unsigned integers
      const unsigned ba = __float_as_uint(mxa), bb = __float_as_uint(mxb);
      if (ba > __hip_atomic_load(amax_kx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(amax_kx, ba);
      if (bb > __hip_atomic_load(amax_ky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(amax_ky, bb);
    }
  }
}

// ---------------------------------------------------------------------------
// normalize_adj backward.  adj_norm_ij = r_i mx_ij r_j, r = d^-1/2, d = rowsum(mx).
//   gr_i = sum_j G_ij mx_ij r_j  +  sum_j G_ji mx_ji r_j
// k_normbwd_row gives the first sum per row; k_colsum_part gives column partials
// of W_ij = G_ij mx_ij r_i (second sum, index renamed) for row strips.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ROW_THREADS) void k_normbwd_row(int n, int ld, const float* __restrict__ G,
                                                             const float* __restrict__ A,
                                                             const float* __restrict__ r,
                                                             float* __restrict__ rowpart) {
  __shared__ float shf[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  float s = 0.f;
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(G + base + j);
    const f32x4 a = *reinterpret_cast<const f32x4*>(A + base + j);
    const f32x4 rj = *reinterpret_cast<const f32x4*>(r + j);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (j + t < n) s += g[t] * (a[t] + (j + t == i ? 1.f : 0.f)) * rj[t];
  }
  s = block_sum(s, shf);
  if (threadIdx.x == 0) rowpart[i] = s;
}

// column partial sums: part[strip][j] = sum_{i in strip} G_ij mx_ij r_i
__global__ __launch_bounds__(256) void k_normbwd_colpart(int n, int ld, const float* __restrict__ G,
                                                         const float* __restrict__ A,
                                                         const float* __restrict__ r, int rows_per_strip,
                                                         float* __restrict__ part) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int strip = blockIdx.y;
  const int i0 = strip * rows_per_strip, i1 = min(n, i0 + rows_per_strip);
  if (j >= n) return;
  float s = 0.f;
  for (int i = i0; i < i1; ++i) {
    const size_t o = (size_t)i * ld + j;
    s += G[o] * (A[o] + (i == j ? 1.f : 0.f)) * r[i];
  }
  part[(size_t)strip * n + j] = s;
}

// gd_i = -1/2 d_i^-3/2 (rowpart_i + sum_strips part[s][i])
__global__ void k_normbwd_gd(int n, const float* __restrict__ rowpart, const float* __restrict__ part,
                             int nstrips, const float* __restrict__ d, float* __restrict__ gd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // (four independent chains: up to 128 strips of dependent 300 ns loads would otherwise take 40 us)
  float s0 = rowpart[i], s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int t = 0;
  for (; t + 3 < nstrips; t += 4) {
    s0 += part[(size_t)t * n + i]; s1 += part[(size_t)(t + 1) * n + i];
    s2 += part[(size_t)(t + 2) * n + i]; s3 += part[(size_t)(t + 3) * n + i];
  }
  for (; t < nstrips; ++t) s0 += part[(size_t)t * n + i];
  const float s = (s0 + s1) + (s2 + s3);
  const float di = d[i];
  gd[i] = di > 0.f ? -0.5f * s * (1.0f / (di * sqrtf(di))) : 0.f;
}

// G_A_ij = G_adjn_ij r_i r_j + gd_i   (A = mx - I)
__global__ __launch_bounds__(ROW_THREADS) void k_normbwd_apply(int n, int ld, const float* __restrict__ G,
                                                               const float* __restrict__ r,
                                                               const float* __restrict__ gd,
                                                               float* __restrict__ GA) {
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  const float ri = r[i], gdi = gd[i];
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(G + base + j);
    const f32x4 rj = *reinterpret_cast<const f32x4*>(r + j);
    f32x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = (j + t < n) ? fmaf(g[t] * ri, rj[t], gdi) : 0.f;
    *reinterpret_cast<f32x4*>(GA + base + j) = o;
  }
}

// ---------------------------------------------------------------------------
// Tile-pair kernels: out_ij needs G_ij and G_ji.  64x64 tiles, transposed tile
// staged through LDS ([64][65] floats, conflict-free column reads).
// ---------------------------------------------------------------------------
#define TP 64

// decode backward (S = Zn Zn^T, A1 = (1-I) sym_lower(relu(S)) + ori):
// out_ij = (i != j) [S_ij > 0] (G_ij + G_ji).  `pos` marks S > 0 (A1 - ori > 0).
__global__ __launch_bounds__(256) void k_sym_mask(int n, int ld, const float* __restrict__ G,
                                                  const float* __restrict__ A1,
                                                  const float* __restrict__ ori, float* __restrict__ out) {
  __shared__ float tile[TP][TP + 1];
  const int bi = blockIdx.y * TP, bj = blockIdx.x * TP;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4
  for (int rr = ty; rr < TP; rr += 4) {  // load G[bj + rr][bi + tx] (the mirrored tile)
    const int gi = bj + rr, gj = bi + tx;
    tile[rr][tx] = (gi < n && gj < n) ? G[(size_t)gi * ld + gj] : 0.f;
  }
  __syncthreads();
  for (int rr = ty; rr < TP; rr += 4) {
    const int i = bi + rr, j = bj + tx;
    if (i < n && j < n) {
      const size_t o = (size_t)i * ld + j;
      float s = A1[o];
      if (ori) s -= ori[o];
      out[o] = (i != j && s > 0.f) ? G[o] + tile[tx][rr] : 0.f;
    }
  }
}

// Packed gradient mirrored to both halves + torch.optim.Adam + projection clamp:
//   g_ij = gate_ij*G_A_ij + gate_ji*G_A_ji + cn * M_ij     (i != j)
//   m <- m + (1-b1)(g - m); v <- b2 v + (1-b2) g^2
//   M <- clamp(M - step_size * m / (sqrt(v)/sqrt(bc2) + eps), 0, 1)   (:279-283)
// M, am, av are symmetric bit for bit (g_ij and g_ji are the same sum), so only the tile pairs on or below the
// diagonal are computed: a block reads its tile of the state once, G_A's tile and mirrored tile, and writes the
// results to both halves (the mirrored half through an LDS transpose): 5.5 n^2 floats instead of 8 n^2.
__global__ __launch_bounds__(256) void k_adam_sym(int n, int ld, const float* __restrict__ GA,
                                                  const unsigned char* __restrict__ gate,
                                                  float* __restrict__ M, float* __restrict__ am,
                                                  float* __restrict__ av, const float* __restrict__ cn_ptr, float omb1, float b2,
                                                  float omb2, float step_size, float sqrt_bc2, float eps,
                                                  float* __restrict__ gsym_dbg, int do_clamp) {
  // (fp contraction is left on: torch's vectorised CPU Adam fuses multiply-adds too, and the 100-epoch Cora run of the
  // reference -- tests/test_gpu_parity.py::test_cora_readme_100_epochs -- is matched with it on, not with it off)
  if (blockIdx.x > blockIdx.y) return;            // upper tile pairs: written by their mirror blocks
  __shared__ float tile[TP][TP + 1];
  const int bi = blockIdx.y * TP, bj = blockIdx.x * TP;
  const bool offdiag = blockIdx.x != blockIdx.y;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const float cn = cn_ptr[0];   // weight_sup * 0.001 / |adj_changes|_2 (0 at the origin), device scalar
  for (int rr = ty; rr < TP; rr += 4) {
    const int gi = bj + rr, gj = bi + tx;
    float v = 0.f;
    if (gi < n && gj < n) {
      const size_t o = (size_t)gi * ld + gj;
      v = GA[o];
      if (gate && !gate[o]) v = 0.f;
    }
    tile[rr][tx] = v;
  }
  __syncthreads();
  float rp[TP / 4], rm[TP / 4], rv[TP / 4], rg[TP / 4];
#pragma unroll
  for (int q = 0; q < TP / 4; ++q) {
    const int rr = ty + 4 * q;
    const int i = bi + rr, j = bj + tx;
    rp[q] = rm[q] = rv[q] = rg[q] = 0.f;
    if (i < n && j < n && i != j) {
      const size_t o = (size_t)i * ld + j;
      float g0 = GA[o];
      if (gate && !gate[o]) g0 = 0.f;
      const float p = M[o];
      const float g = g0 + tile[tx][rr] + cn * p;
      float m = am[o], v = av[o];
      m = m + omb1 * (g - m);            // exp_avg.lerp_(grad, 1 - beta1)
      v = v * b2 + omb2 * g * g;         // mul_(beta2).addcmul_(grad, grad, 1 - beta2)
      const float denom = sqrtf(v) / sqrt_bc2 + eps;
      float pn = p - step_size * (m / denom);
      if (do_clamp) pn = fminf(fmaxf(pn, 0.f), 1.f);
      am[o] = m; av[o] = v; M[o] = pn;
      if (gsym_dbg) gsym_dbg[o] = g;
      rp[q] = pn; rm[q] = m; rv[q] = v; rg[q] = g;
    }
  }
  if (!offdiag) return;                 // a diagonal tile holds both halves itself
  // mirrored half: element (j, i) = element (i, j); one array at a time through the (now free) LDS tile
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float* dst = a == 0 ? M : a == 1 ? am : a == 2 ? av : gsym_dbg;
    if (!dst) continue;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TP / 4; ++q) tile[ty + 4 * q][tx] = a == 0 ? rp[q] : a == 1 ? rm[q] : a == 2 ? rv[q] : rg[q];
    __syncthreads();
    for (int rr = ty; rr < TP; rr += 4) {
      const int gi = bj + rr, gj = bi + tx;      // row of the mirrored tile, column = original row
      if (gi < n && gj < n) dst[(size_t)gi * ld + gj] = tile[tx][rr];
    }
  }
}

// projection helpers (:338-347, :397-412): sum_{i>j} clamp(M_ij - x, 0, 1) as
// per-row partials over the full symmetric matrix (halved by the caller),
// plus min/max of M over i != j.
__global__ __launch_bounds__(ROW_THREADS) void k_clamp_rowsum(int n, int ld, const float* __restrict__ M,
                                                              float x, double* __restrict__ rows,
                                                              float* __restrict__ rowmin,
                                                              float* __restrict__ rowmax) {
  __shared__ double shd[16];
  __shared__ float shmn[4], shmx[4];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  double s = 0;
  float mn = INFINITY, mx = -INFINITY;
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) {
    if (j == i) continue;
    const float m = M[base + j];
    s += fminf(fmaxf(m - x, 0.f), 1.f);
    mn = fminf(mn, m); mx = fmaxf(mx, m);
  }
  s = block_sum_d(s, shd);
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
  if ((threadIdx.x & 63) == 0) { shmn[threadIdx.x >> 6] = mn; shmx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    rows[i] = s;
    if (rowmin) { rowmin[i] = fminf(fminf(shmn[0], shmn[1]), fminf(shmn[2], shmn[3]));
                  rowmax[i] = fmaxf(fmaxf(shmx[0], shmx[1]), fmaxf(shmx[2], shmx[3])); }
  }
}

__global__ __launch_bounds__(ROW_THREADS) void k_shift_clamp(int n, int ld, float* __restrict__ M, float x) {
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  for (int j = threadIdx.x; j < n; j += ROW_THREADS)
    if (j != i) M[base + j] = fminf(fmaxf(M[base + j] - x, 0.f), 1.f);
}

__global__ void k_minmax(int n, const float* __restrict__ rowmin, const float* __restrict__ rowmax,
                         float* __restrict__ out) {
  __shared__ float smn[16], smx[16];
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < n; i += blockDim.x) { mn = fminf(mn, rowmin[i]); mx = fmaxf(mx, rowmax[i]); }
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
  if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int w = 1; w < nw; ++w) { mn = fminf(mn, smn[w]); mx = fmaxf(mx, smx[w]); }
    out[0] = mn; out[1] = mx;
  }
}

// packed <-> dense data movement (topology_attack.py:371-377)
__global__ void k_unpack_sym(int n, int ld, const float* __restrict__ packed, const float* __restrict__ ori,
                             int ori_ld, float* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= n) return;
  float v = 0.f;
  if (i != j) {
    const int a = i > j ? i : j, b = i > j ? j : i;
    v = packed[(size_t)a * (a - 1) / 2 + b];
  }
  if (ori) v += ori[(size_t)i * ori_ld + j];
  out[(size_t)i * ld + j] = v;
}

__global__ void k_pack_tril(int n, int ld, const float* __restrict__ M, float* __restrict__ packed) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= i) return;
  packed[(size_t)i * (i - 1) / 2 + j] = M[(size_t)i * ld + j];
}

// dot_product_decode packed output (:414-419): out[p(i,j)] = relu(S_ij), i > j
__global__ void k_pack_tril_relu(int n, int ld, const float* __restrict__ S, float* __restrict__ packed) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= i) return;
  packed[(size_t)i * (i - 1) / 2 + j] = fmaxf(S[(size_t)i * ld + j], 0.f);
}

// dot_product_decode2 epilogues (:421-467), accumulated into the ensemble:
//   mode 0: out += sigmoid(relu(S - I))       mode 2: out += relu(S - I)
//   mode 3: out += relu(S / max(|S_i|_2, 1e-12) - I)   (rownorm = |S_i|_2 given)
__global__ __launch_bounds__(ROW_THREADS) void k_dd2_accum(int n, int ld, const float* __restrict__ S,
                                                           int mode, const float* __restrict__ rownorm,
                                                           float* __restrict__ out, int out_ld) {
  const int i = blockIdx.x;
  float inv = 1.f;
  if (mode == 3) inv = 1.f / fmaxf(rownorm[i], 1e-12f);
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) {
    float s = S[(size_t)i * ld + j];
    if (mode == 3) s *= inv;
    s = fmaxf(s - (i == j ? 1.f : 0.f), 0.f);
    if (mode == 0) s = 1.f / (1.f + expf(-s));
    out[(size_t)i * out_ld + j] += s;
  }
}

__global__ __launch_bounds__(ROW_THREADS) void k_row_l2(int n, int ld, const float* __restrict__ S,
                                                        float* __restrict__ rownorm) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  double s = 0;
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) { const float v = S[(size_t)i * ld + j]; s += (double)v * v; }
  s = block_sum_d(s, shd);
  if (threadIdx.x == 0) rownorm[i] = (float)sqrt(s);
}

// out (ld_o) = a * X (ld_x) + b * Y (ld_y) over an n x n window; Y may be NULL
__global__ void k_axpby2d(int n, const float* __restrict__ X, int ldx, float a, const float* __restrict__ Y,
                          int ldy, float b, float* __restrict__ out, int ldo) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= n) return;
  float v = a * X[(size_t)i * ldx + j];
  if (Y) v += b * Y[(size_t)i * ldy + j];
  out[(size_t)i * ldo + j] = v;
}

// generic elementwise sum of squares of differences (mcgra_mse), double partials
__global__ void k_sqdiff_part(size_t count, const float* __restrict__ X, const float* __restrict__ Y,
                              double* __restrict__ part) {
  __shared__ double shd[16];
  double s = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const float e = X[i] - Y[i];
    s += (double)e * e;
  }
  s = block_sum_d(s, shd);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// info entropy value only (mcgra_info_entropy)
__global__ __launch_bounds__(ROW_THREADS) void k_ie_rows(int n, int ld, const float* __restrict__ P,
                                                         double* __restrict__ rows) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  double s = 0;
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) {
    float v, g;
    ie_term(P[(size_t)i * ld + j], 0.f, v, g);
    s += v;
  }
  s = block_sum_d(s, shd);
  if (threadIdx.x == 0) rows[i] = s;
}


// ---------------------------------------------------------------------------
// PGDAttack.calc_kl on N x N operands (topology_attack.py:483-487):
//   calc_kl(X, Y) = sum_ij softmax(X)_ij (log softmax(X)_ij - log_softmax(Y)_ij) / n   (rows = batch)
//   c1 = k1 calc_kl(feature_adj, adj_norm)   c2 = k2 calc_kl(adj_norm, A1)
// FS = row softmax of feature_adj (constant).  One block per row; the row (<= 160 KB) stays in L1/L2
// across the passes.  Gradients are ACCUMULATED into GA (adj_norm) and GB (A1).
//   d/dY = (softmax(Y) - softmax(X)) / n
//   d/dX = xs * (g - <g, xs>),  g = (log xs + 1 - log_softmax(Y)) / n
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ROW_THREADS) void k_row_softmax(int n, int ld, const float* __restrict__ X,
                                                             float* __restrict__ out) {
  __shared__ float shf[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) mx = fmaxf(mx, X[base + j]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) shf[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(shf[0], shf[1]), fmaxf(shf[2], shf[3]));
  float s = 0.f;
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) s += expf(X[base + j] - mx);
  s = block_sum(s, shf);
  const float ls = logf(s);
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) out[base + j] = expf(X[base + j] - mx - ls);
}

__device__ __forceinline__ float block_max4(float v, float* sh) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

__global__ __launch_bounds__(ROW_THREADS) void k_kl_rows(int n, int ld, const float* __restrict__ A,
                                                         const float* __restrict__ B, const float* __restrict__ FS,
                                                         float k1, float k2, float* __restrict__ GA,
                                                         float* __restrict__ GB, double* __restrict__ rowvals) {
  __shared__ float shf[16];
  __shared__ double shd[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  const float invn = 1.f / (float)n;
  float ma = -INFINITY, mb = -INFINITY;
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) { ma = fmaxf(ma, A[base + j]); if (k2 != 0.f) mb = fmaxf(mb, B[base + j]); }
  ma = block_max4(ma, shf);
  if (k2 != 0.f) mb = block_max4(mb, shf);
  float sa = 0.f, sb = 0.f;
  double sa8 = 0, sb8 = 0;
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) {
    const float ea = expf(A[base + j] - ma);
    sa += ea; sa8 += (double)ea;
    if (k2 != 0.f) { const float eb = expf(B[base + j] - mb); sb += eb; sb8 += (double)eb; }
  }
  sa = block_sum(sa, shf);
  if (k2 != 0.f) sb = block_sum(sb, shf);
  const float lsa = ma + logf(sa), lsb = (k2 != 0.f) ? mb + logf(sb) : 0.f;
  // The VALUES take the rows' log-sum-exps in float64: a value is a difference of log-sum-exps of ~ log n that agree to three
  // digits, and the rows of adj_norm are so alike that every row's float32 log-sum-exp rounds the same way -- a bias of 3e-5 (c1)
  // and 2e-4 (c2) of the value at n = 700, ten times the float32 reference's (tests/test_gpu_terms.py).  The gradients keep
  // the float32 ones (their bits are unchanged).
  sa8 = block_sum_d(sa8, shd);
  if (k2 != 0.f) sb8 = block_sum_d(sb8, shd);
  const double lsa8 = (double)ma + log(sa8), lsb8 = (k2 != 0.f) ? (double)mb + log(sb8) : 0.0;
  // <g, xs> of the c2 term and the two values
  double v1 = 0, v2 = 0;
  float dot = 0.f;
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) {
    const float la = A[base + j] - lsa;
    const double la8 = (double)A[base + j] - lsa8;
    if (k1 != 0.f) { const float f = FS[base + j]; if (f > 0.f) v1 += (double)f * ((double)logf(f) - la8); }
    if (k2 != 0.f) {
      const float lb = B[base + j] - lsb, xs = expf(la);
      if (xs > 0.f) v2 += (double)xs * (la8 - ((double)B[base + j] - lsb8));
      dot += (la + 1.f - lb) * invn * xs;
    }
  }
  v1 = block_sum_d(v1, shd); v2 = block_sum_d(v2, shd);
  if (k2 != 0.f) dot = block_sum(dot, shf);
  for (int j = threadIdx.x; j < n; j += ROW_THREADS) {
    const float la = A[base + j] - lsa, xs = expf(la);
    float ga = 0.f;
    if (k1 != 0.f) ga += k1 * invn * (xs - FS[base + j]);
    if (k2 != 0.f) {
      const float lb = B[base + j] - lsb;
      ga += k2 * xs * ((la + 1.f - lb) * invn - dot);
      GB[base + j] += k2 * invn * (expf(lb) - xs);
    }
    GA[base + j] += ga;
  }
  if (threadIdx.x == 0) { rowvals[i] = v1 * invn; rowvals[(size_t)n + i] = v2 * invn; }
}


// row sums of squares (double) - |P|_F^2 of PGDAttack.dot_product (:480-481)
__global__ __launch_bounds__(ROW_THREADS) void k_rowsumsq(int n, int ld, const float* __restrict__ P,
                                                          double* __restrict__ rows) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  double s = 0;
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(P + base + j);
#pragma unroll
    for (int t = 0; t < 4; ++t) if (j + t < n) s += (double)v[t] * v[t];
  }
  s = block_sum_d(s, shd);
  if (threadIdx.x == 0) rows[i] = s;
}

// G += (k / sqrt(*sumsq)) * T   (0 when *sumsq == 0: torch.norm backward at the origin)
__global__ __launch_bounds__(ROW_THREADS) void k_axpy_invnorm(int n, int ld, const float* __restrict__ T,
                                                              const double* __restrict__ sumsq, float k,
                                                              float* __restrict__ G) {
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  const double sq = sumsq[0];
  const float c = sq > 0.0 ? (float)(k / sqrt(sq)) : 0.f;
  for (int j = threadIdx.x * 4; j < n; j += ROW_THREADS * 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(T + base + j);
    f32x4 g = *reinterpret_cast<f32x4*>(G + base + j);
#pragma unroll
    for (int q = 0; q < 4; ++q) if (j + q < n) g[q] += c * t[q];
    *reinterpret_cast<f32x4*>(G + base + j) = g;
  }
}


// ---------------------------------------------------------------------------
// CudaCKA.linear_CKA on N x N operands (utils.py:1091-1096): hsic(X,Y) / (sqrt(hsic(X,X)) sqrt(hsic(Y,Y))).
// KX, KY: centred Grams of adj_norm / A1 (lower tile storage when lower != 0), KFC: centred Gram of
// feature_adj.  k_cka_sums gives per-row partials of <KFC,KX>, <KX,KX>, <KX,KY>, <KY,KY>;
// k_cka_coef turns the five inner products into the coefficients of the gradient left factors
//   L1 = af KFC + ax KX + ay KY  (G_adjn += L1 @ Xc),   L2 = bx KX + by KY  (G_A1 += L2 @ Yc)
// and k_cka_lincomb writes L1 -> KY, L2 -> KX in place.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ROW_THREADS) void k_cka_sums(int n, int ld, const float* __restrict__ KX,
                                                          const float* __restrict__ KY, const float* __restrict__ KFC,
                                                          int use1, int use2, double* __restrict__ rowvals, int lower) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  const int jdiag = lower ? (i / SYM_TILE) * SYM_TILE : 0;
  const int jend = lower ? min(n, jdiag + SYM_TILE) : n;
  double fx = 0, xx = 0, xy = 0, yy = 0;
  for (int j = threadIdx.x; j < jend; j += ROW_THREADS) {
    const double w = (lower && j < jdiag) ? 2.0 : 1.0;
    const double kx = KX[base + j];
    xx += w * kx * kx;
    if (use1) fx += w * kx * (double)KFC[base + j];
    if (use2) { const double ky = KY[base + j]; xy += w * kx * ky; yy += w * ky * ky; }
  }
  fx = block_sum_d(fx, shd); xx = block_sum_d(xx, shd); xy = block_sum_d(xy, shd); yy = block_sum_d(yy, shd);
  if (threadIdx.x == 0) {
    rowvals[i] = fx; rowvals[(size_t)n + i] = xx; rowvals[2 * (size_t)n + i] = xy; rowvals[3 * (size_t)n + i] = yy;
  }
}

// in: s[0..3] = hfx, hxx, hxy, hyy; hff; k1, k2 (0 = term off).  out: coef[0..4] = af, ax, ay, bx, by.
// A vanishing denominator (identical rows) is the documented 0/0 case: that term contributes nothing.
__global__ void k_cka_coef(const double* __restrict__ s, const double* __restrict__ hff, float k1, float k2,
                           float* __restrict__ coef) {
  const double hfx = s[0], hxx = s[1], hxy = s[2], hyy = s[3];
  double af = 0, ax = 0, ay = 0, bx = 0, by = 0;
  if (k1 != 0.f) {
    const double den = sqrt(hff[0]) * sqrt(hxx);
    if (den > 0) { af = k1 * 2.0 / den; ax += -k1 * 2.0 * hfx / (den * hxx); }
  }
  if (k2 != 0.f) {
    const double den = sqrt(hxx) * sqrt(hyy);
    if (den > 0) { ay = k2 * 2.0 / den; ax += -k2 * 2.0 * hxy / (den * hxx); bx = k2 * 2.0 / den; by = -k2 * 2.0 * hxy / (den * hyy); }
  }
  coef[0] = (float)af; coef[1] = (float)ax; coef[2] = (float)ay; coef[3] = (float)bx; coef[4] = (float)by;
}

__global__ __launch_bounds__(ROW_THREADS) void k_cka_lincomb(int n, int ld, float* __restrict__ KX,
                                                             float* __restrict__ KY, const float* __restrict__ KFC,
                                                             const float* __restrict__ coef, int use1, int use2, int lower,
                                                             unsigned* __restrict__ amax_l2, unsigned* __restrict__ amax_l1) {
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  const int jend = lower ? min(n, (i / SYM_TILE + 1) * SYM_TILE) : n;
  const float af = coef[0], ax = coef[1], ay = coef[2], bx = coef[3], by = coef[4];
  float m1 = 0.f, m2 = 0.f;       // largest magnitudes of L1 / L2 (operand scales of the fp16 split, optional)
  for (int j = threadIdx.x; j < jend; j += ROW_THREADS) {
    const float kx = KX[base + j];
    const float ky = use2 ? KY[base + j] : 0.f;
    const float kf = use1 ? KFC[base + j] : 0.f;
    const float l1 = af * kf + ax * kx + ay * ky, l2 = bx * kx + by * ky;
    KY[base + j] = l1;
    KX[base + j] = l2;
    m1 = fmaxf(m1, fabsf(l1)); m2 = fmaxf(m2, fabsf(l2));
  }
  if (amax_l1) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m1 = fmaxf(m1, __shfl_xor(m1, o)); m2 = fmaxf(m2, __shfl_xor(m2, o)); }
    if ((threadIdx.x & 63) == 0) {
      const unsigned b1 = __float_as_uint(m1), b2 = __float_as_uint(m2);
      if (b1 > __hip_atomic_load(amax_l1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(amax_l1, b1);
      if (b2 > __hip_atomic_load(amax_l2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(amax_l2, b2);
    }
  }
}


// column sums of an n x n matrix (asymmetric adj_norm when eps != 0): strip partials then a fixed-order sum
__global__ __launch_bounds__(256) void k_colsum_part(int n, int ld, const float* __restrict__ X, int rows_per_strip,
                                                     double* __restrict__ part) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int strip = blockIdx.y;
  const int i0 = strip * rows_per_strip, i1 = min(n, i0 + rows_per_strip);
  if (j >= n) return;
  double s = 0;
  for (int i = i0; i < i1; ++i) s += X[(size_t)i * ld + j];
  part[(size_t)strip * n + j] = s;
}
__global__ void k_colsum_fin(int n, const double* __restrict__ part, int nstrips, double* __restrict__ cols) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double s = 0;
  for (int t = 0; t < nstrips; ++t) s += part[(size_t)t * n + j];
  cols[j] = s;
}


// ---------------------------------------------------------------------------
// hsic.py (Gaussian-kernel HSIC): distmat (:20-27) + kernelmat (:30-47) + hsic_regular (:117-124).
//   D_ij = r_i - 2 a_ij + r_j,  K = exp(-D / (2 sigma^2)),  Kc = K H  (row i minus its mean),
//   hsic_regular = mean_ij Kxc_ij Kyc_ji.  K is symmetric, so Kyc_ji = Ky_ij - rowmean_y[j].
// k_gauss_kernel turns the Gram a = X X^T into K in place and leaves row sums of K.
// ---------------------------------------------------------------------------
// (sq2 != nullptr, m2 columns: the cross form D_xy of mmd (hsic.py:83-85); inv2s2 == 0: leave the distance matrix itself)
__global__ __launch_bounds__(ROW_THREADS) void k_gauss_kernel(int m, int ld, float* __restrict__ A,
                                                              const float* __restrict__ sq, float inv2s2,
                                                              double* __restrict__ rows, const float* __restrict__ sq2, int m2) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  const float ri = sq[i];
  const float* sc = sq2 ? sq2 : sq;
  const int mc = sq2 ? m2 : m;
  double s = 0;
  for (int j = threadIdx.x; j < mc; j += ROW_THREADS) {
    // (r_i + r_j) first: the sum commutes, so D_ij and D_ji -- and K with them -- are the same bits for the symmetric Gram of the
    // square form.  k_hsic_gauss_rows and mcgra_mmd_pxpy_pxy read K's row means as its column means.  (r_i - 2 a) + r_j is not.
    const float d = (ri + sc[j]) - 2.f * A[base + j];
    const float k = inv2s2 != 0.f ? expf(-d * inv2s2) : d;
    A[base + j] = k;
    s += k;
  }
  s = block_sum_d(s, shd);
  if (threadIdx.x == 0) rows[i] = s;
}

// rows[i] = sum_j (Kx_ij - mx_i) (Ky_ij - my_j)
__global__ __launch_bounds__(ROW_THREADS) void k_hsic_gauss_rows(int m, int ld, const float* __restrict__ KX,
                                                                 const float* __restrict__ KY,
                                                                 const double* __restrict__ rowsx,
                                                                 const double* __restrict__ rowsy,
                                                                 double* __restrict__ rows) {
  __shared__ double shd[16];
  const int i = blockIdx.x;
  const size_t base = (size_t)i * ld;
  const double inv = 1.0 / m;
  const float mxi = (float)(rowsx[i] * inv);
  double s = 0;
  for (int j = threadIdx.x; j < m; j += ROW_THREADS)
    s += (double)(KX[base + j] - mxi) * (double)(KY[base + j] - (float)(rowsy[j] * inv));
  s = block_sum_d(s, shd);
  if (threadIdx.x == 0) rows[i] = s;
}

// sq[i] = |X_i|^2 (torch.sum(X*X, 1), hsic.py:23)
__global__ void k_row_sqnorm(int m, int d, const float* __restrict__ X, int ldx, float* __restrict__ sq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  float s = 0.f;
  for (int k = 0; k < d; ++k) { const float v = X[(size_t)i * ldx + k]; s += v * v; }
  sq[i] = s;
}

// ---- host launchers ---------------------------------------------------------
#define LAUNCH(k, g, b, st, ...) hipLaunchKernelGGL(k, g, b, 0, st, __VA_ARGS__)

void launch_prep(hipStream_t st, bool general, int n, int ld, const float* M, const float* ori,
                 const float* noise, float eps, float* A, unsigned char* gate, float* d, float* r,
                 double* rowsq, double* rowsum, int row0, int row1) {
  if (row1 < 0) row1 = n;            // rows [row0, row1) only (row-block ranks); default: all
  if (row1 <= row0) return;
  if (general) LAUNCH(k_prep<true>, dim3(row1 - row0), dim3(ROW_THREADS), st, n, ld, M, ori, noise, eps, A, gate, d, r, rowsq, rowsum, row0);
  else LAUNCH(k_prep<false>, dim3(row1 - row0), dim3(ROW_THREADS), st, n, ld, M, ori, noise, eps, A, gate, d, r, rowsq, rowsum, row0);
}
void launch_adjn(hipStream_t st, int n, int ld, const float* A, const float* r, float* out, double* rowsum) {
  LAUNCH(k_adjn, dim3(n), dim3(ROW_THREADS), st, n, ld, A, r, out, rowsum);
}
void launch_decode_post(hipStream_t st, int n, int ld, float* S, const float* ori, unsigned int* nmask) {
  LAUNCH(k_decode_post, dim3(n), dim3(ROW_THREADS), st, n, ld, S, ori, nmask);
}
void launch_loss_elem(hipStream_t st, int n, int ld, const float* X, const float* Y, const float* F,
                      float kmse1, float kmse2, float kie6, float kie7, float* GX, float* GY,
                      double* rowvals) {
  LAUNCH(k_loss_elem, dim3(n), dim3(ROW_THREADS), st, n, ld, X, Y, F, kmse1, kmse2, kie6, kie7, GX, GY, rowvals);
}
void launch_reduce_rows(hipStream_t st, const double* rowvals, int n, int nvec, double* out) {
  LAUNCH(k_reduce_rows, dim3(nvec), dim3(1024), st, rowvals, n, out);
}
void launch_rowsum(hipStream_t st, int n, int ld, const float* K, double* rows) {
  LAUNCH(k_rowsum, dim3(n), dim3(ROW_THREADS), st, n, ld, K, rows);
}
void launch_center(hipStream_t st, int n, int ld, float* K, const double* rows, const double* total) {
  LAUNCH(k_center, dim3(n), dim3(ROW_THREADS), st, n, ld, K, rows, total);
}
void launch_center_cols(hipStream_t st, int n, int ld, const float* X, const double* rows, float* mean_scratch,
                        float* out, double* rowsq, float* absmax) {
  LAUNCH(k_colmean_f32, dim3((ld + 255) / 256), dim3(256), st, n, ld, rows, mean_scratch, (unsigned*)absmax);
  LAUNCH(k_center_cols, dim3(n), dim3(ROW_THREADS), st, n, ld, X, mean_scratch, out, rowsq, (unsigned*)absmax);
}
void launch_colmean_f32(hipStream_t st, int n, int ld, const double* colsum, float* mean) {
  LAUNCH(k_colmean_f32, dim3((ld + 255) / 256), dim3(256), st, n, ld, colsum, mean, (unsigned*)nullptr);
}
void launch_hsic_combine(hipStream_t st, int n, int ld, float* KX, float* KY, const float* KFC, float s1, float s2,
                         double* rowvals, bool lower, float* amax_kx, float* amax_ky) {
  LAUNCH(k_hsic_combine, dim3(n), dim3(ROW_THREADS), st, n, ld, KX, KY, KFC, s1, s2, rowvals, lower ? 1 : 0, (unsigned*)amax_kx,
         (unsigned*)amax_ky);
}
void launch_row_softmax(hipStream_t st, int n, int ld, const float* X, float* out) {
  LAUNCH(k_row_softmax, dim3(n), dim3(ROW_THREADS), st, n, ld, X, out);
}
void launch_kl_rows(hipStream_t st, int n, int ld, const float* A, const float* B, const float* FS, float k1, float k2,
                    float* GA, float* GB, double* rowvals) {
  LAUNCH(k_kl_rows, dim3(n), dim3(ROW_THREADS), st, n, ld, A, B, FS, k1, k2, GA, GB, rowvals);
}
void launch_rowsumsq(hipStream_t st, int n, int ld, const float* P, double* rows) {
  LAUNCH(k_rowsumsq, dim3(n), dim3(ROW_THREADS), st, n, ld, P, rows);
}
void launch_axpy_invnorm(hipStream_t st, int n, int ld, const float* T, const double* sumsq, float k, float* G) {
  LAUNCH(k_axpy_invnorm, dim3(n), dim3(ROW_THREADS), st, n, ld, T, sumsq, k, G);
}
void launch_cka_sums(hipStream_t st, int n, int ld, const float* KX, const float* KY, const float* KFC, bool use1,
                     bool use2, double* rowvals, bool lower) {
  LAUNCH(k_cka_sums, dim3(n), dim3(ROW_THREADS), st, n, ld, KX, KY, KFC, use1 ? 1 : 0, use2 ? 1 : 0, rowvals, lower ? 1 : 0);
}
void launch_cka_coef(hipStream_t st, const double* s4, const double* hff, float k1, float k2, float* coef) {
  LAUNCH(k_cka_coef, dim3(1), dim3(1), st, s4, hff, k1, k2, coef);
}
void launch_cka_lincomb(hipStream_t st, int n, int ld, float* KX, float* KY, const float* KFC, const float* coef,
                        bool use1, bool use2, bool lower, float* amax_l2, float* amax_l1) {
  LAUNCH(k_cka_lincomb, dim3(n), dim3(ROW_THREADS), st, n, ld, KX, KY, KFC, coef, use1 ? 1 : 0, use2 ? 1 : 0, lower ? 1 : 0,
         (unsigned*)amax_l2, (unsigned*)amax_l1);
}
void launch_colsum(hipStream_t st, int n, int ld, const float* X, double* part, int nstrips, double* cols) {
  const int rows_per_strip = (n + nstrips - 1) / nstrips;
  LAUNCH(k_colsum_part, dim3((n + 255) / 256, nstrips), dim3(256), st, n, ld, X, rows_per_strip, part);
  LAUNCH(k_colsum_fin, dim3((n + 255) / 256), dim3(256), st, n, part, nstrips, cols);
}
void launch_gauss_kernel(hipStream_t st, int m, int ld, float* A, const float* sq, float inv2s2, double* rows, const float* sq2,
                         int m2) {
  LAUNCH(k_gauss_kernel, dim3(m), dim3(ROW_THREADS), st, m, ld, A, sq, inv2s2, rows, sq2, m2);
}
void launch_hsic_gauss_rows(hipStream_t st, int m, int ld, const float* KX, const float* KY, const double* rowsx,
                            const double* rowsy, double* rows) {
  LAUNCH(k_hsic_gauss_rows, dim3(m), dim3(ROW_THREADS), st, m, ld, KX, KY, rowsx, rowsy, rows);
}
void launch_row_sqnorm(hipStream_t st, int m, int d, const float* X, int ldx, float* sq) {
  LAUNCH(k_row_sqnorm, dim3((m + 255) / 256), dim3(256), st, m, d, X, ldx, sq);
}
void launch_normbwd(hipStream_t st, int n, int ld, const float* G, const float* A, const float* r,
                    const float* d, float* rowpart, float* colpart, int nstrips, float* gd, float* GA, bool have_parts) {
  const int rows_per_strip = (n + nstrips - 1) / nstrips;
  if (!have_parts) {
    LAUNCH(k_normbwd_row, dim3(n), dim3(ROW_THREADS), st, n, ld, G, A, r, rowpart);
    LAUNCH(k_normbwd_colpart, dim3((n + 255) / 256, nstrips), dim3(256), st, n, ld, G, A, r, rows_per_strip, colpart);
  }
  LAUNCH(k_normbwd_gd, dim3((n + 255) / 256), dim3(256), st, n, rowpart, colpart, nstrips, d, gd);
  if (GA) LAUNCH(k_normbwd_apply, dim3(n), dim3(ROW_THREADS), st, n, ld, G, r, gd, GA);   // NULL: folded into the consumer
}
void launch_sym_mask(hipStream_t st, int n, int ld, const float* G, const float* A1, const float* ori, float* out) {
  const int t = (n + TP - 1) / TP;
  LAUNCH(k_sym_mask, dim3(t, t), dim3(256), st, n, ld, G, A1, ori, out);
}
void launch_adam_sym(hipStream_t st, int n, int ld, const float* GA, const unsigned char* gate, const AdamUpdate& u) {
  const int t = (n + TP - 1) / TP;
  LAUNCH(k_adam_sym, dim3(t, t), dim3(256), st, n, ld, GA, gate, u.M, u.am, u.av, u.cn, u.omb1, u.b2, u.omb2, u.step_size, u.sqrt_bc2, u.eps,
         u.gsym_dbg, u.do_clamp);
}
void launch_clamp_rowsum(hipStream_t st, int n, int ld, const float* M, float x, double* rows, float* rowmin, float* rowmax) {
  LAUNCH(k_clamp_rowsum, dim3(n), dim3(ROW_THREADS), st, n, ld, M, x, rows, rowmin, rowmax);
}
void launch_shift_clamp(hipStream_t st, int n, int ld, float* M, float x) {
  LAUNCH(k_shift_clamp, dim3(n), dim3(ROW_THREADS), st, n, ld, M, x);
}
void launch_minmax(hipStream_t st, int n, const float* rowmin, const float* rowmax, float* out) {
  LAUNCH(k_minmax, dim3(1), dim3(1024), st, n, rowmin, rowmax, out);
}
void launch_unpack_sym(hipStream_t st, int n, int ld, const float* packed, const float* ori, int ori_ld, float* out) {
  LAUNCH(k_unpack_sym, dim3((n + 255) / 256, n), dim3(256), st, n, ld, packed, ori, ori_ld, out);
}
void launch_pack_tril(hipStream_t st, int n, int ld, const float* M, float* packed, bool relu) {
  if (relu) LAUNCH(k_pack_tril_relu, dim3((n + 255) / 256, n), dim3(256), st, n, ld, M, packed);
  else LAUNCH(k_pack_tril, dim3((n + 255) / 256, n), dim3(256), st, n, ld, M, packed);
}
void launch_dd2_accum(hipStream_t st, int n, int ld, const float* S, int mode, float* rownorm, float* out, int out_ld) {
  if (mode == 3) LAUNCH(k_row_l2, dim3(n), dim3(ROW_THREADS), st, n, ld, S, rownorm);
  LAUNCH(k_dd2_accum, dim3(n), dim3(ROW_THREADS), st, n, ld, S, mode, rownorm, out, out_ld);
}
void launch_axpby2d(hipStream_t st, int n, const float* X, int ldx, float a, const float* Y, int ldy, float b,
                    float* out, int ldo) {
  LAUNCH(k_axpby2d, dim3((n + 255) / 256, n), dim3(256), st, n, X, ldx, a, Y, ldy, b, out, ldo);
}
void launch_sqdiff(hipStream_t st, size_t count, const float* X, const float* Y, double* part, int nblocks) {
  LAUNCH(k_sqdiff_part, dim3(nblocks), dim3(256), st, count, X, Y, part);
}
void launch_ie_rows(hipStream_t st, int n, int ld, const float* P, double* rows) {
  LAUNCH(k_ie_rows, dim3(n), dim3(ROW_THREADS), st, n, ld, P, rows);
}

}  // namespace mcgra
