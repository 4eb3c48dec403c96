// Edge-level differential privacy on the true graph (mcgra_dp_perturb_graph): EdgeRand and LapGraph of Wu et al., "LinkTeller:
// Recovering Private Edges from Graph Neural Networks via Influence Analysis" (IEEE S&P 2022), one pass over the
// m = n (n - 1) / 2 unordered pairs a > b in the project's packed order p = a (a - 1) / 2 + b.
//
// Randomness: one Philox4x32-10 call per pair (Salmon et al., SC'11), key = (seed & 0xffffffff, seed >> 32), counter =
// (p, 0, replicate, 0), no state: pair p's draw depends on nothing but (seed, replicate, p), so the result is the same on every
// call, every rank and every grid, and a prefix of the pairs of a larger graph.
//   EdgeRand  T = floor(2^32 / (1 + e^eps) + 1/2) on the host; pair p flips iff w0 < T.  Integers only.
//   LapGraph  u = ((w0 >> 8) + 1/2) 2^-24 in (0, 1), sigma = +1 iff bit 31 of w1 is clear, Lap(beta) = sigma beta (-ln u), all in
//             double (dp_laplace, host and device); v_p = float32(A_p + Lap(1 / (0.99 eps))), one rounding of the double sum;
//             target = clamp(rint(E + Lap(1 / (0.01 eps))), 0, m) at counter (m, 0, replicate, 0), on the host; the result is
//             the target best pairs by v descending, ties by ascending p: the selection of mcgra_topk_metrics (topk_mark).
//
// Passes, each over the 64 x 64 tiles on or below the diagonal, a tile's mirror image written through an LDS transpose
// ([64][65] floats) so that both halves leave as 256-byte row segments:
//   k_dp_edgerand    reads adj's tile (2 n^2 bytes in all), writes out's tile and mirror (4 n^2): HBM-bound by design
//   k_dp_lap_noise   reads adj's tile, writes v's tile and mirror; counts E
//   topk_mark        the radix select of topk.hip on v: a byte per pair
//   k_dp_lap_write   reads the bytes and adj's tile, writes out's tile and mirror
// E, kept, added and removed are per-block integer sums merged by 64-bit integer atomics: the same bits whatever order the
// blocks run in.  A label other than 0 or 1 sets a flag; the host refuses then.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>

#include "../../include/mcgra.h"
#include "common.h"
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int DP_TILE = 64;                 // a block of AUC_THREADS lanes owns one DP_TILE x DP_TILE tile: 64 columns x 4 rows a step
constexpr int DP_ROWS = AUC_THREADS / DP_TILE;
constexpr int DP_MAX_N = 65535;             // a packed position fits 32 bits

enum { DP_EDGES, DP_KEPT, DP_ADDED, DP_REMOVED, DP_COUNTS };
struct DpState {
  unsigned long long c[DP_COUNTS];
  int flags;
};

// Philox4x32-10: w = the ten rounds of counter c under key k
__host__ __device__ inline void dp_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// Lap(beta) of a draw's words w0, w1, in double; no contraction: beta (-ln u) is rounded before anything is added to it
__host__ __device__ inline double dp_laplace(uint32_t w0, uint32_t w1, double beta) {
#pragma clang fp contract(off)
  const double u = ((double)(w0 >> 8) + 0.5) * (1.0 / 16777216.0);
  const double mag = beta * -log(u);
  return (w1 & 0x80000000u) ? -mag : mag;
}

__host__ __device__ inline double dp_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// tile (I, J), J <= I, of linear index t = I (I + 1) / 2 + J
__device__ __forceinline__ void dp_tile_of(uint32_t t, int& I, int& J) {
  uint32_t x = (uint32_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((uint64_t)x * (x + 1) / 2 > t) --x;
  while ((uint64_t)(x + 1) * (x + 2) / 2 <= t) ++x;
  I = (int)x;
  J = (int)(t - (uint32_t)((uint64_t)x * (x + 1) / 2));
}

// One tile: value(i, j, p, a) for every pair j < i of it (a = adj[i][j] == 1) goes to dst[i][j] and, through the LDS tile,
// to dst[j][i]; the tile's diagonal entries get 0.  Returns the flags of the labels read.
template <class V>
__device__ __forceinline__ int dp_tile_pass(int n, const float* __restrict__ adj, int64_t lda, float* __restrict__ dst, int64_t ldd,
                                            float (*tile)[DP_TILE + 1], V&& value) {
  int I, J;
  dp_tile_of(blockIdx.x, I, J);
  const int bi = I * DP_TILE, bj = J * DP_TILE;
  const int tx = threadIdx.x & (DP_TILE - 1), ty = threadIdx.x / DP_TILE;
  int f = 0;
  for (int rr = ty; rr < DP_TILE; rr += DP_ROWS) {
    const int i = bi + rr, j = bj + tx;
    float o = 0.f;
    if (i < n && j < i) {                                         // (j < i < n)
      const float l = adj[(int64_t)i * lda + j];
      const bool a = auc_pos(l);
      if (!a && !auc_neg(l)) f |= AUC_BAD_LABEL;                  // also NaN
      o = value(i, j, (uint32_t)((uint64_t)i * (i - 1) / 2 + j), a);
    }
    tile[rr][tx] = o;
    if (i < n && j <= i) dst[(int64_t)i * ldd + j] = o;    // j == i: the diagonal's 0
  }
  __syncthreads();
  for (int rr = ty; rr < DP_TILE; rr += DP_ROWS) {
    const int gi = bj + rr, gj = bi + tx;                         // row of the mirrored tile; its column is the original row
    if (gj < n && gi < gj) dst[(int64_t)gi * ldd + gj] = tile[tx][rr];      // (gi < gj < n; in a diagonal tile: its upper half)
  }
  return f;
}

__device__ __forceinline__ void dp_merge(const uint64_t (&part)[DP_COUNTS], int f, DpState* __restrict__ st) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  if (f) atomicOr(&st->flags, f);
  block_add_u64(part, sh, st->c);
}

__global__ __launch_bounds__(AUC_THREADS) void k_dp_edgerand(int n, const float* __restrict__ adj, int64_t lda, uint32_t T,
                                                             uint32_t k0, uint32_t k1, uint32_t replicate,
                                                             float* __restrict__ out, int64_t ldo, DpState* __restrict__ st) {
  __shared__ float tile[DP_TILE][DP_TILE + 1];
  uint64_t part[DP_COUNTS] = {0, 0, 0, 0};
  const int f = dp_tile_pass(n, adj, lda, out, ldo, tile, [&](int, int, uint32_t p, bool a) {
    uint32_t w[4];
    dp_philox(p, 0u, replicate, 0u, k0, k1, w);
    const bool o = a != (w[0] < T);
    part[DP_EDGES] += a;
    part[DP_KEPT] += a && o;
    part[DP_ADDED] += !a && o;
    part[DP_REMOVED] += a && !o;
    return o ? 1.f : 0.f;
  });
  dp_merge(part, f, st);
}

__global__ __launch_bounds__(AUC_THREADS) void k_dp_lap_noise(int n, const float* __restrict__ adj, int64_t lda, double beta,
                                                              uint32_t k0, uint32_t k1, uint32_t replicate,
                                                              float* __restrict__ v, int64_t ldv, DpState* __restrict__ st) {
  __shared__ float tile[DP_TILE][DP_TILE + 1];
  uint64_t part[DP_COUNTS] = {0, 0, 0, 0};
  const int f = dp_tile_pass(n, adj, lda, v, ldv, tile, [&](int, int, uint32_t p, bool a) {
    uint32_t w[4];
    dp_philox(p, 0u, replicate, 0u, k0, k1, w);
    part[DP_EDGES] += a;
    return (float)dp_add(a ? 1.0 : 0.0, dp_laplace(w[0], w[1], beta));
  });
  dp_merge(part, f, st);
}

// mark == NULL: no pair is kept (target 0)
__global__ __launch_bounds__(AUC_THREADS) void k_dp_lap_write(int n, const float* __restrict__ adj, int64_t lda,
                                                              const uint8_t* __restrict__ mark, float* __restrict__ out, int64_t ldo,
                                                              DpState* __restrict__ st) {
  __shared__ float tile[DP_TILE][DP_TILE + 1];
  uint64_t part[DP_COUNTS] = {0, 0, 0, 0};
  dp_tile_pass(n, adj, lda, out, ldo, tile, [&](int, int, uint32_t p, bool a) {
    const bool o = mark && mark[p];
    part[DP_KEPT] += a && o;
    part[DP_ADDED] += !a && o;
    part[DP_REMOVED] += a && !o;
    return o ? 1.f : 0.f;
  });
  dp_merge(part, 0, st);                                          // (the labels were checked by k_dp_lap_noise, which counted the edges)
}

int dp_fetch(hipStream_t st, const DpState* dev, DpState& h) {
  MCGRA_HIP(hipMemcpyAsync(&h, dev, sizeof(DpState), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  return 0;
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_dp_perturb_graph(void* stream, int n, const float* adj, int ld_adj, int mechanism, double eps, uint64_t seed,
                                      uint32_t replicate, float* out, int ld_out, float* noisy, int ld_noisy, int64_t* counts,
                                      double* realised) {
  const char* who = "dp_perturb_graph";
  const bool lap = mechanism == MCGRA_DP_LAPGRAPH;
  if (n < 2 || n > DP_MAX_N || !adj || ld_adj < n || !out || ld_out < n || !counts || (mechanism != MCGRA_DP_EDGERAND && !lap) ||
      !(eps > 0.0) || !std::isfinite(eps) || (noisy && (!lap || ld_noisy < n))) {
    set_error("%s: bad argument (2 <= n <= %d, adj, out and counts not NULL, every ld >= n, mechanism 0 or 1, a finite eps > 0, "
              "noisy with LapGraph only)", who, DP_MAX_N);
    return MCGRA_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const uint64_t m = (uint64_t)n * (n - 1) / 2;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int nt = (n + DP_TILE - 1) / DP_TILE;
  const unsigned tiles = (unsigned)nt * (nt + 1) / 2;             // <= 524 800
  AucBufs b;
  DpState* state = b.get<DpState>(1);
  if (!state) { set_error("%s: hipMalloc failed", who); return MCGRA_ENOMEM; }
  MCGRA_HIP(hipMemsetAsync(state, 0, sizeof(DpState), st));
  DpState h{};
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (!lap) {
    const double t = floor(4294967296.0 / (1.0 + exp(eps)) + 0.5);        // <= 2^31: e^eps >= 1
    const uint32_t T = (uint32_t)t;
    k_dp_edgerand<<<tiles, AUC_THREADS, 0, st>>>(n, adj, ld_adj, T, k0, k1, replicate, out, ld_out, state);
    MCGRA_KERNEL_CHECK();
    if (int rc = dp_fetch(st, state, h)) return rc;
    if (int rc = rank_flag_error(who, h.flags)) return rc;
    counts[2] = -1;
    if (realised) {
      const double q = t / 4294967296.0;
      realised[0] = q;
      realised[1] = T ? log((1.0 - q) / q) : std::numeric_limits<double>::infinity();
    }
  } else {
    const double eps1 = 0.01 * eps, eps2 = 0.99 * eps;
    float* v = noisy;
    int ldv = ld_noisy;
    if (!v) {
      v = b.get<float>((size_t)n * n);
      ldv = n;
      if (!v) { set_error("%s: hipMalloc of the %d x %d noisy cells failed", who, n, n); return MCGRA_ENOMEM; }
    }
    uint8_t* mark = b.get<uint8_t>(m);
    if (!mark) { set_error("%s: hipMalloc of %llu bytes failed", who, (unsigned long long)m); return MCGRA_ENOMEM; }
    k_dp_lap_noise<<<tiles, AUC_THREADS, 0, st>>>(n, adj, ld_adj, 1.0 / eps2, k0, k1, replicate, v, ldv, state);
    MCGRA_KERNEL_CHECK();
    if (int rc = dp_fetch(st, state, h)) return rc;
    if (int rc = rank_flag_error(who, h.flags)) return rc;
    uint32_t w[4];
    dp_philox((uint32_t)m, 0u, replicate, 0u, k0, k1, w);
    const double noise = dp_laplace(w[0], w[1], 1.0 / eps1);
    const double want = rint(dp_add((double)h.c[DP_EDGES], noise));
    const uint64_t target = want <= 0.0 ? 0 : want >= (double)m ? m : (uint64_t)want;
    if (target)
      if (int rc = topk_mark(who, st, n, v, ldv, target, mark)) return rc;
    k_dp_lap_write<<<tiles, AUC_THREADS, 0, st>>>(n, adj, ld_adj, target ? mark : nullptr, out, ld_out, state);
    MCGRA_KERNEL_CHECK();
    if (int rc = dp_fetch(st, state, h)) return rc;
    counts[2] = (int64_t)target;
    if (realised) { realised[0] = noise; realised[1] = nan; }
  }
  counts[0] = (int64_t)m;
  counts[1] = (int64_t)h.c[DP_EDGES];
  counts[3] = (int64_t)h.c[DP_KEPT];
  counts[4] = (int64_t)h.c[DP_ADDED];
  counts[5] = (int64_t)h.c[DP_REMOVED];
  return 0;
}
