// Exact binary ROC-AUC of a scored square matrix restricted to idx x idx: main.metric_pool (main.py:66-75), i.e.
// sklearn.metrics.roc_curve + auc on ori_adj[idx][:, idx] against inference_adj[idx][:, idx], without gathering the
// submatrix.  AUC = U / (P N) with 2U = sum over positives of (2 #negatives with a lower score + #negatives with an equal
// score) (Mann-Whitney, ties counted 1/2), which is exactly the area under the step curve roc_curve draws.
//
// Passes (DESIGN.md "Recovered-adjacency AUC"; the idx check and the sort are rank_common.hip's, shared with the whole family):
//   rank_check_idx     idx only: range check, repeats; a repeat-free idx of all n nodes is the whole matrix in another
//                      order (the AUC depends on the multiset of (label, score) pairs only) and runs as idx = NULL
//   k_auc_classify     one read of the selected scores and labels: argument checks, per-block positive / negative counts
//   k_auc_emit         a second read: each entry's order-preserving 32-bit key, positives to one region of the
//                      scratch, negatives to another, at per-block offsets (the host's scan of the counts)
//   auc_sort           per region, a stable LSD radix sort of the keys: 4 passes of 8 bits, each a per-block digit
//                      count, one scan of the (digit, block) counts and a stable scatter
//   k_auc_pairs        each key of the smaller class looks up its lower and upper bound in the sorted larger class;
//                      the sum of the two is that key's share of 2U
//   k_ap_terms         (average precision, mcgra_rank_metrics) each positive key x: its lower bound in the sorted
//                      positives and in the sorted negatives give TP = #positives >= x, FP = #negatives >= x and the term
//                      TP / (TP + FP); one float64 partial per block.  k_ap_sum adds the partials and divides by P
//   rank_curves_sorted (mcgra_rank_curves: the ROC and precision-recall curves) the third consumer of the two sorted regions;
//                      its passes are in curves.hip
// mcgra_decode_auc ranks scores that are never stored, s_ij = dot_product_decode2(Z)_ij of a thin factor Z [n x d]:
//   k_dec_rows         every row of Z: NaN / inf check, the L2-normalised copy of modes 1 and 4
//   k_dec_classify     k_auc_classify's body (auc_classify_one) on the scores dec_for_each decodes, a block owning 64 x 64
//                      tiles of idx x idx
//   k_dec_emit         k_auc_emit's body (auc_emit_one) on the same scores; the sort and k_auc_pairs follow unchanged
//   k_dec_scores       the same scores written out (mcgra_decode_scores: the materialised route)
// Counts and 2U are 64-bit integers merged with global integer atomics, so the result does not depend on the order in
// which blocks run; the one rounding is the final division (host, exact integer long division, nearest even).
//
// Average precision, AP = (1 / P) sum over selected positives of TP / (TP + FP) at that positive's score (ties included:
// sklearn.metrics.average_precision_score), is a sum of float64 terms, so its summation order is fixed instead: no
// floating-point atomics, a grid that is a function of P alone (min(4096, ceil(P / 256)) blocks of 256 lanes), each lane adds
// its strided terms in index order, the 64 lanes of a wave are added in a fixed xor-shuffle tree (6 levels), the four waves
// as (w0 + w1) + (w2 + w3) through LDS, and one block adds the per-block partials the same way (at most 16 per lane, then
// the same 8 levels).  The sorted regions do not depend on the order of a repeat-free idx, so neither do the bits of AP.
// Rounding: TP + FP < 2^33 is exact in float64, so a term is one correctly rounded division; with T = ceil(P / (256 x blocks))
// serial terms per lane the result passes through at most 1 + (T - 1) + 8 + 15 + 8 + 1 = T + 32 roundings, and all terms are
// positive, so the relative error is at most (T + 32) 2^-53 (1 + o(1)): 3.7e-15 up to P = 2^20, and with n_idx <= 65 535
// (P < 2^32, T <= 4096) at most 4128 * 2^-53 = 4.6e-13.
// P = 0: AP is a mean over no positives, NaN as the AUC of an absent class is (sklearn 1.7 returns 0.0 with a "No positive
// class found" warning, older versions NaN).  N = 0: every term is 1 and AP is exactly 1.0, as sklearn's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/mcgra.h"
#include "common.h"
#include "rank_common.h"      // the keys, the checks, the block sums, the bound and the radix sort
#include "curves.h"           // the third consumer of the sorted regions (curves.hip: mcgra_rank_curves)
#include "auc_run.h"          // AucRun and the bodies of the classify and emit passes (shared with pair_distance.hip)

namespace mcgra {

namespace {
constexpr int AP_BLOCKS = 4096;            // at most this many blocks (and float64 partials) of k_ap_terms
static_assert(AUC_THREADS == 256, "block_sum_f64 adds four waves as (w0 + w1) + (w2 + w3)");

// scores decoded pair by pair from a thin factor Z (mcgra_decode_auc, mcgra_decode_scores)
constexpr int DEC_TILE = 64;               // a block's tile: 64 x 64 selected pairs, 4 x 4 per lane
constexpr int DEC_KC = 32;                 // columns of Z staged per step
constexpr int DEC_MAX_D = 128;             // widest factor mcgra_decode_auc takes
constexpr int DEC_SCORE_BLOCKS = 4096;     // blocks of k_dec_scores (grid-stride over the tiles)

// f(score, label) for every selected entry this block owns: rows r = blockIdx.x, + gridDim.x, ... of the selection.
// idx == NULL: rows and columns 0 .. n-1, 16-byte loads when a row's scores and labels share their alignment;
// otherwise row idx[r], columns idx[0 .. rows).
template <class F>
__device__ __forceinline__ void auc_for_each(int rows, const float* __restrict__ S, int64_t lds, const float* __restrict__ L,
                                             int64_t ldl, const int64_t* __restrict__ idx, F&& f) {
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const int64_t i = idx ? idx[r] : r;
    const float* srow = S + i * lds;
    const float* lrow = L + i * ldl;
    if (idx) {
      for (int c = threadIdx.x; c < rows; c += blockDim.x) {
        const int64_t j = idx[c];
        f(srow[j], lrow[j]);
      }
      continue;
    }
    const uintptr_t as = (uintptr_t)srow, al = (uintptr_t)lrow;
    int head = rows;                                    // scalar prefix; the whole row when the alignments differ
    if (((as ^ al) & 15) == 0) head = min(rows, (int)(((16 - (as & 15)) & 15) >> 2));
    for (int c = threadIdx.x; c < head; c += blockDim.x) f(srow[c], lrow[c]);
    const int nv = (rows - head) >> 2;
    const float4* s4 = (const float4*)(srow + head);
    const float4* l4 = (const float4*)(lrow + head);
    for (int v = threadIdx.x; v < nv; v += blockDim.x) {
      const float4 a = s4[v], b = l4[v];
      f(a.x, b.x); f(a.y, b.y); f(a.z, b.z); f(a.w, b.w);
    }
    for (int c = head + 4 * nv + threadIdx.x; c < rows; c += blockDim.x) f(srow[c], lrow[c]);
  }
}

// float64 sum over the block in one fixed tree: xor butterfly over the 64 lanes of a wave (a + b == b + a, so every lane
// holds the same bits), then (w0 + w1) + (w2 + w3); valid in every thread
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

}  // namespace

// counts[2 b] / counts[2 b + 1] = positives / negatives block b selects; flags |= the argument errors it meets
__global__ __launch_bounds__(AUC_THREADS) void k_auc_classify(int rows, const float* __restrict__ S, int64_t lds,
                                                              const float* __restrict__ L, int64_t ldl,
                                                              const int64_t* __restrict__ idx, uint64_t* __restrict__ counts,
                                                              int* __restrict__ flags) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  uint32_t pos = 0, tot = 0;
  int f = 0;
  auc_for_each(rows, S, lds, L, ldl, idx, [&](float s, float l) { auc_classify_one(s, l, pos, tot, f); });
  auc_classify_end(pos, tot, f, sh, counts, flags);
}

// keys of block b's positives to keys[offs[2 b] ..), of its negatives to keys[offs[2 b + 1] ..) (any order inside a block)
__global__ __launch_bounds__(AUC_THREADS) void k_auc_emit(int rows, const float* __restrict__ S, int64_t lds,
                                                          const float* __restrict__ L, int64_t ldl,
                                                          const int64_t* __restrict__ idx, const uint64_t* __restrict__ offs,
                                                          uint32_t* __restrict__ keys) {
  __shared__ uint32_t cur[2];
  if (threadIdx.x < 2) cur[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t o_pos = offs[2 * blockIdx.x], o_neg = offs[2 * blockIdx.x + 1];
  auc_for_each(rows, S, lds, L, ldl, idx, [&](float s, float l) { auc_emit_one(s, l, o_pos, o_neg, cur, keys); });
}

// acc += for each key x of A: lower_bound(B, x) + upper_bound(B, x) (a_pos: A holds the positives), or, A holding the
// negatives, (|B| - upper_bound) + (|B| - lower_bound): the positives above x twice and those equal to x once
__global__ __launch_bounds__(AUC_THREADS) void k_auc_pairs(const uint32_t* __restrict__ A, uint64_t na,
                                                           const uint32_t* __restrict__ B, uint64_t nbk, int a_pos,
                                                           unsigned long long* __restrict__ acc) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  uint64_t s = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * AUC_THREADS + threadIdx.x; i < na; i += (uint64_t)gridDim.x * AUC_THREADS) {
    const uint32_t x = A[i];
    const uint64_t lt = rank_bound<false>(B, (uint64_t)0, nbk, x);       // first key >= x
    const uint64_t le = rank_bound<true>(B, lt, nbk, x);                 // first key > x
    s += a_pos ? lt + le : (nbk - le) + (nbk - lt);
  }
  const uint64_t tot = block_sum_u64(s, sh);
  if (threadIdx.x == 0 && tot) atomicAdd(acc, (unsigned long long)tot);
}

// part[b] = block b's sum of TP / (TP + FP) over the sorted positives Pk[0, np) it owns (index i = global lane, + lanes of
// the grid, ...; a lane adds its terms in that order), TP = np - lower_bound(Pk, x), FP = nn - lower_bound(Nk, x).  Always
// walks the positives; the grid is a function of np alone (header comment).
__global__ __launch_bounds__(AUC_THREADS) void k_ap_terms(const uint32_t* __restrict__ Pk, uint64_t np,
                                                          const uint32_t* __restrict__ Nk, uint64_t nn,
                                                          double* __restrict__ part) {
  __shared__ double sh[AUC_THREADS / 64];
  double s = 0.0;
  for (uint64_t i = (uint64_t)blockIdx.x * AUC_THREADS + threadIdx.x; i < np; i += (uint64_t)gridDim.x * AUC_THREADS) {
    const uint32_t x = Pk[i];
    const uint64_t tp = np - rank_bound<false>(Pk, (uint64_t)0, i, x);    // first positive >= x: Pk[i] == x, so at or before i
    const uint64_t fp = nn - rank_bound<false>(Nk, (uint64_t)0, nn, x);   // first negative >= x
    s += (double)tp / (double)(tp + fp);            // tp + fp < 2^33: both conversions exact, one rounding
  }
  const double tot = block_sum_f64(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// one block: *out = (part[0] + ... + part[nb - 1]) / np, lane t adding part[t], part[t + 256], ... then the same tree
__global__ __launch_bounds__(AUC_THREADS) void k_ap_sum(const double* __restrict__ part, int nb, uint64_t np,
                                                        double* __restrict__ out) {
  __shared__ double sh[AUC_THREADS / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += AUC_THREADS) s += part[i];
  const double tot = block_sum_f64(s, sh);
  if (threadIdx.x == 0) *out = tot / (double)np;
}

// ---- scores decoded from a thin factor: s_ij = dot_product_decode2(Z)_ij, modes 0, 1, 2, 4, pair by pair ----
namespace {
struct DecShared {
  float a[DEC_TILE][DEC_KC + 1];           // the row panel and the column panel of Z, one step of DEC_KC columns
  float b[DEC_TILE][DEC_KC + 1];
  int64_t ia[DEC_TILE], ib[DEC_TILE];      // their node ids; -1 past the selection
};

// THE score of a pair: f(i, j, s_ij, L_ij) for every selected pair (i, j) of the tiles this block owns (tile t = blockIdx.x,
// + gridDim.x, ... of the ts x ts tiles of idx x idx; idx == NULL: all nodes).  s_ij = <z_i, z_j> accumulated k ascending
// in fp32 (one fma per k), - 1 where i == j, relu, sigmoid when sig.  The products commute, so s_ij and s_ji are the same
// bits, and every kernel below takes its scores from here.
template <class F>
__device__ __forceinline__ void dec_for_each(int rows, int d, const float* __restrict__ Z, int64_t ldz, bool sig,
                                             const float* __restrict__ L, int64_t ldl, const int64_t* __restrict__ idx,
                                             DecShared& sh, F&& f) {
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int ts = (rows + DEC_TILE - 1) / DEC_TILE;
  for (int64_t tile = blockIdx.x; tile < (int64_t)ts * ts; tile += gridDim.x) {
    const int a0 = (int)(tile / ts) * DEC_TILE, b0 = (int)(tile % ts) * DEC_TILE;
    __syncthreads();                                  // the previous tile's epilogue has read ia / ib
    if (t < 2 * DEC_TILE) {
      const int r = t % DEC_TILE, q = (t < DEC_TILE ? a0 : b0) + r;
      (t < DEC_TILE ? sh.ia : sh.ib)[r] = q < rows ? (idx ? idx[q] : (int64_t)q) : -1;
    }
    __syncthreads();
    // the pairs' labels (L != NULL) are asked for first: their latency runs beside the panels' loads and the products
    float lab[4][4] = {};
    if (L) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int64_t i = sh.ia[ty + 16 * r], j = sh.ib[tx + 16 * c];
          if (i >= 0 && j >= 0) lab[r][c] = L[i * ldl + j];
        }
    }
    float acc[4][4] = {};
    for (int k0 = 0; k0 < d; k0 += DEC_KC) {
      if (k0) __syncthreads();
      for (int e = t; e < DEC_TILE * DEC_KC; e += AUC_THREADS) {
        const int r = e / DEC_KC, k = k0 + e % DEC_KC;
        const int64_t i = sh.ia[r], j = sh.ib[r];
        sh.a[r][e % DEC_KC] = (i >= 0 && k < d) ? Z[i * ldz + k] : 0.f;
        sh.b[r][e % DEC_KC] = (j >= 0 && k < d) ? Z[j * ldz + k] : 0.f;
      }
      __syncthreads();
      const int kn = min(DEC_KC, d - k0);
      for (int k = 0; k < kn; ++k) {
        float a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] = sh.a[ty + 16 * q][k]; b[q] = sh.b[tx + 16 * q][k]; }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(a[r], b[c], acc[r][c]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t i = sh.ia[ty + 16 * r], j = sh.ib[tx + 16 * c];
        if (i < 0 || j < 0) continue;
        float s = acc[r][c];
        if (i == j) s -= 1.f;
        s = s <= 0.f ? 0.f : s;                       // relu; a NaN stays one (torch.relu)
        if (sig) s = 1.f / (1.f + expf(-s));
        f(i, j, s, lab[r][c]);
      }
  }
}
}  // namespace

// One wave per row of Z: flags |= AUC_BAD_FACTOR for a NaN / inf entry; Zn != NULL: Zn[row] = z / max(|z|_2, 1e-12)
// (F.normalize(Z, p=2, dim=1)), leading dimension d.
__global__ __launch_bounds__(AUC_THREADS) void k_dec_rows(int n, int d, const float* __restrict__ Z, int64_t ldz,
                                                          float* __restrict__ Zn, int* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  bool bad = false;
  for (int row = blockIdx.x * (AUC_THREADS / 64) + (threadIdx.x >> 6); row < n; row += gridDim.x * (AUC_THREADS / 64)) {
    const float* z = Z + row * ldz;
    float ss = 0.f;
    for (int k = lane; k < d; k += 64) {
      const float v = z[k];
      bad |= !auc_finite(v);
      ss = fmaf(v, v, ss);
    }
    if (!Zn) continue;
    const float den = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
    for (int k = lane; k < d; k += 64) Zn[(int64_t)row * d + k] = z[k] / den;
  }
  if (bad) atomicOr(flags, AUC_BAD_FACTOR);
}

// k_auc_classify / k_auc_emit with the scores of dec_for_each
__global__ __launch_bounds__(AUC_THREADS) void k_dec_classify(int rows, int d, const float* __restrict__ Z, int64_t ldz, int sig,
                                                              const float* __restrict__ L, int64_t ldl,
                                                              const int64_t* __restrict__ idx, uint64_t* __restrict__ counts,
                                                              int* __restrict__ flags) {
  __shared__ DecShared sh;
  __shared__ uint64_t red[AUC_THREADS / 64];
  uint32_t pos = 0, tot = 0;
  int f = 0;
  dec_for_each(rows, d, Z, ldz, sig != 0, L, ldl, idx, sh,
               [&](int64_t, int64_t, float s, float l) { auc_classify_one(s, l, pos, tot, f); });
  auc_classify_end(pos, tot, f, red, counts, flags);
}

__global__ __launch_bounds__(AUC_THREADS) void k_dec_emit(int rows, int d, const float* __restrict__ Z, int64_t ldz, int sig,
                                                          const float* __restrict__ L, int64_t ldl,
                                                          const int64_t* __restrict__ idx, const uint64_t* __restrict__ offs,
                                                          uint32_t* __restrict__ keys) {
  __shared__ DecShared sh;
  __shared__ uint32_t cur[2];
  if (threadIdx.x < 2) cur[threadIdx.x] = 0;
  const uint64_t o_pos = offs[2 * blockIdx.x], o_neg = offs[2 * blockIdx.x + 1];
  dec_for_each(rows, d, Z, ldz, sig != 0, L, ldl, idx, sh,
               [&](int64_t, int64_t, float s, float l) { auc_emit_one(s, l, o_pos, o_neg, cur, keys); });
}

// out[i][j] = s_ij for all nodes: the materialised route
__global__ __launch_bounds__(AUC_THREADS) void k_dec_scores(int n, int d, const float* __restrict__ Z, int64_t ldz, int sig,
                                                            float* __restrict__ out, int64_t ldo) {
  __shared__ DecShared sh;
  dec_for_each(n, d, Z, ldz, sig != 0, nullptr, 0, nullptr, sh, [&](int64_t i, int64_t j, float s, float) { out[i * ldo + j] = s; });
}

namespace {
// num / den rounded to the nearest double (ties to even), 0 < num <= den < 2^63
double auc_divide(uint64_t num, uint64_t den) {
  if (num == 0) return 0.0;
  typedef unsigned __int128 u128;
  const u128 N = num, D = den;
  int sh = 0;
  while ((N << sh) < (D << 53)) ++sh;               // 2^53 <= N 2^sh / D < 2^54 (N 2^sh < 2^117)
  const u128 x = N << sh;
  uint64_t q = (uint64_t)(x / D);
  const bool rest = (x % D) != 0;
  const bool half = q & 1u;
  q >>= 1;                                          // 53 bits; the dropped bit and the remainder decide the rounding
  if (half && (rest || (q & 1u))) ++q;
  return ldexp((double)q, 1 - sh);
}

}  // namespace

// AucRun (auc_run.h): what mcgra_roc_auc / mcgra_rank_metrics, mcgra_decode_auc / mcgra_decode_rank_metrics and
// mcgra_pair_distance_rank_metrics share around their two passes over the selected pairs.
int AucRun::begin() {
  flags = b.get<int>(1);
  counts = b.get<uint64_t>(2 * AUC_ROW_BLOCKS);
  acc = b.get<unsigned long long>(1);
  if (!flags || !counts || !acc) { set_error("%s: hipMalloc failed", who); return MCGRA_ENOMEM; }
  MCGRA_HIP(hipMemsetAsync(flags, 0, sizeof(int), st));
  MCGRA_HIP(hipMemsetAsync(acc, 0, sizeof(unsigned long long), st));
  return 0;
}
int AucRun::select(int n, const int64_t*& idx, int64_t n_idx) {
  bool repeated = false;
  if (int rc = rank_check_idx(who, st, b, n, idx, n_idx, flags, true, &repeated)) return rc;
  if (!repeated && n_idx == n) idx = nullptr;
  return 0;
}
int AucRun::finish(int g, const AucEmit& emit, double* auc, double* ap, const CurveRequest* cv, uint64_t* pnt) {
  std::vector<uint64_t> h(2 * (size_t)g);
  MCGRA_HIP(hipMemcpyAsync(h.data(), counts, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (int rc = rank_flag_error(who, h_flags)) return rc;     // (sklearn raises ValueError for each of them)
  uint64_t P = 0, N = 0;
  for (int i = 0; i < g; ++i) { P += h[2 * i]; N += h[2 * i + 1]; }
  if ((P == 0 || N == 0) && !cv) {
    if (auc) *auc = NAN;                              // roc_curve: tpr or fpr is 0 / 0 (sklearn warns), auc is NaN
    if (ap) *ap = P == 0 ? NAN : 1.0;                 // a mean over no positives; no negatives: every term is TP / TP
    if (pnt) { pnt[0] = P; pnt[1] = N; pnt[2] = 0; }
    return 0;
  }
  // positives at [0, P), negatives at [nbase, nbase + N): each region starts on a 16-byte boundary
  const uint64_t nbase = (P + 3) / 4 * 4;
  for (uint64_t op = 0, on = nbase, i = 0; i < (uint64_t)g; ++i) {
    const uint64_t p = h[2 * i], q = h[2 * i + 1];
    h[2 * i] = op; h[2 * i + 1] = on;
    op += p; on += q;
  }
  uint32_t* keys = b.get<uint32_t>(nbase + N);
  uint32_t* tmp = b.get<uint32_t>(nbase + N);
  const SortScratch ss(b);
  double* part = ap ? b.get<double>(AP_BLOCKS + 1) : nullptr;      // the per-block partials, then the result
  if (!keys || !tmp || !ss.cnt || (ap && !part)) { set_error("%s: hipMalloc of 2 x %llu keys failed", who, (unsigned long long)(nbase + N)); return MCGRA_ENOMEM; }
  MCGRA_HIP(hipMemcpyAsync(counts, h.data(), sizeof(uint64_t) * h.size(), hipMemcpyHostToDevice, st));
  emit(counts, keys);
  MCGRA_KERNEL_CHECK();
  if (int rc = auc_sort(st, keys, tmp, P, ss)) return rc;
  if (int rc = auc_sort(st, keys + nbase, tmp + nbase, N, ss)) return rc;
  if (cv) return rank_curves_sorted(who, st, keys, tmp, P, nbase, N, *cv);
  unsigned long long u2 = 0;
  if (auc) {
    const bool a_pos = P <= N;                      // look the smaller class up in the larger one
    const uint32_t* A = a_pos ? keys : keys + nbase;
    const uint32_t* B = a_pos ? keys + nbase : keys;
    const uint64_t na = a_pos ? P : N, nbk = a_pos ? N : P;
    const int gp = (int)std::min<uint64_t>(4096, (na + AUC_THREADS - 1) / AUC_THREADS);
    k_auc_pairs<<<gp, AUC_THREADS, 0, st>>>(A, na, B, nbk, a_pos ? 1 : 0, acc);
    MCGRA_KERNEL_CHECK();
    MCGRA_HIP(hipMemcpyAsync(&u2, acc, sizeof(u2), hipMemcpyDeviceToHost, st));
  }
  double h_ap = 0.0;
  if (ap) {
    const int ga = (int)std::min<uint64_t>(AP_BLOCKS, (P + AUC_THREADS - 1) / AUC_THREADS);
    k_ap_terms<<<ga, AUC_THREADS, 0, st>>>(keys, P, keys + nbase, N, part);
    k_ap_sum<<<1, AUC_THREADS, 0, st>>>(part, ga, P, part + AP_BLOCKS);
    MCGRA_KERNEL_CHECK();
    MCGRA_HIP(hipMemcpyAsync(&h_ap, part + AP_BLOCKS, sizeof(double), hipMemcpyDeviceToHost, st));
  }
  MCGRA_HIP(hipStreamSynchronize(st));
  if (auc) *auc = auc_divide((uint64_t)u2, 2 * P * N);
  if (ap) *ap = h_ap;
  if (pnt) { pnt[0] = P; pnt[1] = N; pnt[2] = (uint64_t)u2; }
  return 0;
}

}  // namespace mcgra

using namespace mcgra;

namespace mcgra {
namespace {
// mcgra_roc_auc (ap == NULL), mcgra_rank_metrics and mcgra_rank_curves (cv != NULL): one classify, one emit and the two sorts
// for whatever is asked for
int rank_matrix(const char* who, void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                const int64_t* idx, int64_t n_idx, double* auc, double* ap, const CurveRequest* cv = nullptr) {
  if (!auc && !ap && !cv) { set_error("%s: bad argument (nothing to compute)", who); return MCGRA_EINVAL; }
  if (int rc = rank_check_args(who, n, {{labels, ld_labels, true}, {scores, ld_scores, true}}, idx, n_idx, 1)) return rc;
  AucRun run{who, (hipStream_t)stream};
  hipStream_t st = run.st;
  if (int rc = run.begin()) return rc;
  if (int rc = run.select(n, idx, n_idx)) return rc;
  const int rows = (int)n_idx;
  const int g = std::min(rows, AUC_ROW_BLOCKS);
  k_auc_classify<<<g, AUC_THREADS, 0, st>>>(rows, scores, ld_scores, labels, ld_labels, idx, run.counts, run.flags);
  MCGRA_KERNEL_CHECK();
  return run.finish(g, [&](const uint64_t* offs, uint32_t* keys) {
    k_auc_emit<<<g, AUC_THREADS, 0, st>>>(rows, scores, ld_scores, labels, ld_labels, idx, offs, keys);
  }, auc, ap, cv);
}
}  // namespace
}  // namespace mcgra

extern "C" int mcgra_roc_auc(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                             const int64_t* idx, int64_t n_idx, double* out) {
  return rank_matrix("roc_auc", stream, n, labels, ld_labels, scores, ld_scores, idx, n_idx, out, nullptr);
}

extern "C" int mcgra_rank_metrics(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                                  const int64_t* idx, int64_t n_idx, double* auc, double* ap) {
  return rank_matrix("rank_metrics", stream, n, labels, ld_labels, scores, ld_scores, idx, n_idx, auc, ap);
}

extern "C" int mcgra_rank_curves(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                                 const int64_t* idx, int64_t n_idx, int drop_intermediate, int64_t cap, int64_t* roc_tps,
                                 int64_t* roc_fps, float* roc_thr, int64_t* pr_tps, int64_t* pr_fps, float* pr_thr,
                                 int64_t* counts, int64_t* best, float* best_thr) {
  const int roc = (roc_tps != nullptr) + (roc_fps != nullptr) + (roc_thr != nullptr);
  const int pr = (pr_tps != nullptr) + (pr_fps != nullptr) + (pr_thr != nullptr);
  if (!counts || cap < 0 || roc % 3 || pr % 3 || (!roc && !pr && !best)) {
    set_error("rank_curves: bad argument (counts, cap >= 0, each curve's three buffers together, something to compute)");
    return MCGRA_EINVAL;
  }
  const CurveRequest rq{drop_intermediate, cap, roc_tps, roc_fps, roc_thr, pr_tps, pr_fps, pr_thr, counts, best, best_thr};
  return rank_matrix("rank_curves", stream, n, labels, ld_labels, scores, ld_scores, idx, n_idx, nullptr, nullptr, &rq);
}

namespace mcgra {
namespace {
// argument checks of the two decode entries; the factor the tile kernels read: Z, or (modes 1, 4) its normalised copy
int dec_prepare(const char* who, AucRun& run, int n, int d, const float*& Z, int& ldz, int mode) {
  if (mode < 0 || mode > 6) { set_error("%s: decode_mode %d", who, mode); return MCGRA_EINVAL; }
  if (mode == 3 || mode > 4) {
    set_error("%s: decode_mode %d is not a function of <z_i, z_j> alone (modes 0, 1, 2, 4)", who, mode);
    return MCGRA_ENOSUP;
  }
  if (int rc = run.begin()) return rc;
  float* Zn = nullptr;
  if (mode == 1 || mode == 4) {
    Zn = run.b.get<float>((size_t)n * d);
    if (!Zn) { set_error("%s: hipMalloc failed", who); return MCGRA_ENOMEM; }
  }
  k_dec_rows<<<std::min((n + 3) / 4, 1024), AUC_THREADS, 0, run.st>>>(n, d, Z, ldz, Zn, run.flags);
  MCGRA_KERNEL_CHECK();
  if (Zn) { Z = Zn; ldz = d; }
  return 0;
}
}  // namespace
}  // namespace mcgra

namespace mcgra {
namespace {
// mcgra_decode_auc (ap == NULL) and mcgra_decode_rank_metrics
int rank_decoded(const char* who, void* stream, int n, int d, const float* Z, int ldz, int mode, const float* labels,
                 int ld_labels, const int64_t* idx, int64_t n_idx, double* auc, double* ap) {
  if (d < 1 || !Z || ldz < d || (!auc && !ap)) {
    set_error("%s: bad argument (Z [n x d], ldz >= d, something to compute)", who);
    return MCGRA_EINVAL;
  }
  if (int rc = rank_check_args(who, n, {{labels, ld_labels, true}}, idx, n_idx, 1)) return rc;
  if (d > DEC_MAX_D) {
    set_error("%s: a factor of %d columns (at most %d; mcgra_decode_scores + mcgra_roc_auc / mcgra_rank_metrics take any width)",
              who, d, DEC_MAX_D);
    return MCGRA_ENOSUP;
  }
  AucRun run{who, (hipStream_t)stream};
  hipStream_t st = run.st;
  if (int rc = dec_prepare(run.who, run, n, d, Z, ldz, mode)) return rc;
  if (int rc = run.select(n, idx, n_idx)) return rc;
  const int rows = (int)n_idx, sig = mode < 2;
  const int ts = (rows + DEC_TILE - 1) / DEC_TILE;
  const int g = (int)std::min<int64_t>((int64_t)ts * ts, AUC_ROW_BLOCKS);
  k_dec_classify<<<g, AUC_THREADS, 0, st>>>(rows, d, Z, ldz, sig, labels, ld_labels, idx, run.counts, run.flags);
  MCGRA_KERNEL_CHECK();
  return run.finish(g, [&](const uint64_t* offs, uint32_t* keys) {
    k_dec_emit<<<g, AUC_THREADS, 0, st>>>(rows, d, Z, ldz, sig, labels, ld_labels, idx, offs, keys);
  }, auc, ap);
}
}  // namespace
}  // namespace mcgra

extern "C" int mcgra_decode_auc(void* stream, int n, int d, const float* Z, int ldz, int mode, const float* labels,
                                int ld_labels, const int64_t* idx, int64_t n_idx, double* out) {
  return rank_decoded("decode_auc", stream, n, d, Z, ldz, mode, labels, ld_labels, idx, n_idx, out, nullptr);
}

extern "C" int mcgra_decode_rank_metrics(void* stream, int n, int d, const float* Z, int ldz, int mode, const float* labels,
                                         int ld_labels, const int64_t* idx, int64_t n_idx, double* auc, double* ap) {
  return rank_decoded("decode_rank_metrics", stream, n, d, Z, ldz, mode, labels, ld_labels, idx, n_idx, auc, ap);
}

extern "C" int mcgra_decode_scores(void* stream, int n, int d, const float* Z, int ldz, int mode, float* out, int ld_out) {
  if (n < 1 || d < 1 || !Z || ldz < d || !out || ld_out < n) { set_error("decode_scores: bad argument"); return MCGRA_EINVAL; }
  AucRun run{"decode_scores", (hipStream_t)stream};
  hipStream_t st = run.st;
  if (int rc = dec_prepare(run.who, run, n, d, Z, ldz, mode)) return rc;
  const int ts = (n + DEC_TILE - 1) / DEC_TILE;
  const int g = (int)std::min<int64_t>((int64_t)ts * ts, DEC_SCORE_BLOCKS);
  k_dec_scores<<<g, AUC_THREADS, 0, st>>>(n, d, Z, ldz, mode < 2, out, ld_out);
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipMemcpyAsync(&run.h_flags, run.flags, sizeof(int), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));     // also: the normalised copy is freed on return
  return rank_flag_error(run.who, run.h_flags);
}
