// Link-stealing distance baselines (He et al., "Stealing Links from Graph Neural Networks", USENIX Security 2021, Attack-0):
// a node pair is scored by a distance between the two nodes' rows of a thin matrix Z [n x d] (posteriors, embeddings or
// features), s_ij = 0.0f - dist(z_i, z_j), so that a higher score means "more like an edge".  Eight metrics, the ids of
// MCGRA_PAIR_* (include/mcgra.h), scipy.spatial.distance's definitions; DESIGN.md "Pair distances" holds the error bounds.
//   k_pd_rows          one wave per row of Z: NaN / inf check; cosine: the row over max(|z|_2, 1e-12); correlation: the same
//                      of the row minus its own mean (a row of equal entries is centred to exact zeros)
//   pd_for_each<M>     THE score of a pair, 64 x 64 tiles of the selected positions, 4 x 4 pairs per lane, K panels in LDS
//   k_pd_classify      auc_classify_one on those scores: per-block counts of positives and negatives, the argument checks
//   k_pd_emit          auc_emit_one on the same scores: the sort keys; AucRun::finish (auc.hip) does the rest unchanged
//   k_pd_scores        the same scores written out (mcgra_pair_distance_scores)
// Every distance is accumulated k ascending in fp32 with one defined operation chain per k (pd_step); |a - b|, |a + b|,
// |a| + |b|, (a - b)^2 and a b give the same bits with a and b swapped, so s_ij and s_ji are the same bits and the ranking
// entry, which walks the tiles on or below the diagonal only, ranks exactly what the materialising entry writes.  The
// arithmetic is VALU work on differences by design: a matrix-core product of norms and inner products would lose both the
// symmetric bits and the defined order.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "../../include/mcgra.h"
#include "common.h"
#include "rank_common.h"
#include "auc_run.h"

namespace mcgra {
namespace {
constexpr int PD_TILE = 64;                // a block's tile: 64 x 64 selected positions, 4 x 4 per lane
constexpr int PD_KC = 32;                  // columns of Z staged per step
constexpr int PD_BLOCKS = AUC_ROW_BLOCKS;  // at most this many blocks (grid-stride over the tiles)
constexpr int PD_NORM_OVERFLOW = 64;       // beside the AUC_BAD_* bits: a row's sum of squares is not finite
static_assert(AUC_THREADS == 256 && PD_TILE == 64, "16 x 16 lanes own 4 x 4 pairs each");

enum { M_COSINE = MCGRA_PAIR_COSINE, M_EUCLIDEAN = MCGRA_PAIR_EUCLIDEAN, M_CORRELATION = MCGRA_PAIR_CORRELATION,
       M_CHEBYSHEV = MCGRA_PAIR_CHEBYSHEV, M_BRAYCURTIS = MCGRA_PAIR_BRAYCURTIS, M_CANBERRA = MCGRA_PAIR_CANBERRA,
       M_CITYBLOCK = MCGRA_PAIR_CITYBLOCK, M_SQEUCLIDEAN = MCGRA_PAIR_SQEUCLIDEAN };

struct PdShared {
  float a[PD_TILE][PD_KC + 1];             // the row panel and the column panel, one step of PD_KC columns; the odd row
  float b[PD_TILE][PD_KC + 1];             // length keeps the 16 rows a wave reads at one k on 16 different banks
  int64_t ia[PD_TILE], ib[PD_TILE];        // their node ids; -1 past the selection
};

// one k of one pair: s (and t, braycurtis' denominator) after coordinate values a and b
template <int M>
__device__ __forceinline__ void pd_step(float a, float b, float& s, float& t) {
  if (M == M_COSINE || M == M_CORRELATION) {
    s = fmaf(a, b, s);
  } else if (M == M_EUCLIDEAN || M == M_SQEUCLIDEAN) {
    const float e = a - b;
    s = fmaf(e, e, s);
  } else if (M == M_CHEBYSHEV) {
    s = fmaxf(s, fabsf(a - b));
  } else if (M == M_BRAYCURTIS) {
    s = s + fabsf(a - b);
    t = t + fabsf(a + b);
  } else if (M == M_CANBERRA) {
    const float den = fabsf(a) + fabsf(b);
    s = s + (den == 0.f ? 0.f : fabsf(a - b) / den);
  } else {
    s = s + fabsf(a - b);
  }
}
// the distance behind the last k
template <int M>
__device__ __forceinline__ float pd_dist(float s, float t) {
  if (M == M_COSINE || M == M_CORRELATION) return fmaxf(0.f, 1.f - s);
  if (M == M_EUCLIDEAN) return sqrtf(s);
  if (M == M_BRAYCURTIS) return t == 0.f ? 0.f : s / t;
  return s;
}

// pair (ta, tb), ta >= tb >= 0, of the tile index p = ta (ta + 1) / 2 + tb
__device__ __forceinline__ void pd_tile_of(uint32_t p, int& ta, int& tb) {
  uint32_t a, b;
  topk_unpack(p, a, b);                     // a > b, p = a (a - 1) / 2 + b
  ta = (int)a - 1;
  tb = (int)b;
}

// f(a, b, i, j, s, L_ij) for every selected pair of positions (a, b) -- nodes i = idx[a], j = idx[b], idx == NULL: the
// positions themselves -- of the tiles this block owns (tile = blockIdx.x, + gridDim.x, ...).  TRI: the tiles with a0 >= b0
// and in them the pairs a > b (the candidates of mcgra_auc_delong); otherwise all ts x ts tiles and every pair.
template <int M, bool TRI, class F>
__device__ __forceinline__ void pd_for_each(int rows, int d, const float* __restrict__ Z, int64_t ldz,
                                            const float* __restrict__ L, int64_t ldl, const int64_t* __restrict__ idx,
                                            PdShared& sh, F&& f) {
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int ts = (rows + PD_TILE - 1) / PD_TILE;
  const int64_t tiles = TRI ? (int64_t)ts * (ts + 1) / 2 : (int64_t)ts * ts;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int ta, tb;
    if (TRI) pd_tile_of((uint32_t)tile, ta, tb);
    else { ta = (int)(tile / ts); tb = (int)(tile % ts); }
    const int a0 = ta * PD_TILE, b0 = tb * PD_TILE;
    __syncthreads();                                  // the previous tile's epilogue has read ia / ib
    if (t < 2 * PD_TILE) {
      const int r = t % PD_TILE, q = (t < PD_TILE ? a0 : b0) + r;
      (t < PD_TILE ? sh.ia : sh.ib)[r] = q < rows ? (idx ? idx[q] : (int64_t)q) : -1;
    }
    __syncthreads();
    // the pairs' labels (L != NULL) are asked for first: their latency runs beside the panels' loads and the chains
    float lab[4][4] = {};
    if (L) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int64_t i = sh.ia[ty + 16 * r], j = sh.ib[tx + 16 * c];
          if (i >= 0 && j >= 0 && (!TRI || a0 + ty + 16 * r > b0 + tx + 16 * c)) lab[r][c] = L[i * ldl + j];
        }
    }
    float acc[4][4] = {}, den[4][4] = {};
    for (int k0 = 0; k0 < d; k0 += PD_KC) {
      if (k0) __syncthreads();
      for (int e = t; e < PD_TILE * PD_KC; e += AUC_THREADS) {
        const int r = e / PD_KC, k = k0 + e % PD_KC;
        const int64_t i = sh.ia[r], j = sh.ib[r];
        sh.a[r][e % PD_KC] = (i >= 0 && k < d) ? Z[i * ldz + k] : 0.f;
        sh.b[r][e % PD_KC] = (j >= 0 && k < d) ? Z[j * ldz + k] : 0.f;
      }
      __syncthreads();
      const int kn = min(PD_KC, d - k0);
      for (int k = 0; k < kn; ++k) {
        float a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] = sh.a[ty + 16 * q][k]; b[q] = sh.b[tx + 16 * q][k]; }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) pd_step<M>(a[r], b[c], acc[r][c], den[r][c]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int pa = a0 + ty + 16 * r, pb = b0 + tx + 16 * c;
        const int64_t i = sh.ia[ty + 16 * r], j = sh.ib[tx + 16 * c];
        if (i < 0 || j < 0 || (TRI && pa <= pb)) continue;
        f(pa, pb, i, j, 0.0f - pd_dist<M>(acc[r][c], den[r][c]), lab[r][c]);
      }
  }
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
}  // namespace

// One wave per row of Z: flags |= AUC_BAD_FACTOR for a NaN / inf entry.  Zn != NULL (leading dimension d):
//   Zn[row] = c / max(|c|_2, 1e-12), c = z (centre == 0) or z - mean(z) (centre != 0; a row whose entries are all equal has
//   c = 0 exactly, whatever its sum rounds to).  Every sum is lane l's entries l, l + 64, ... in that order, then the xor tree
//   over the 64 lanes: the same bits on every call.  flags |= PD_NORM_OVERFLOW when a finite row's sum of squares is not.
__global__ __launch_bounds__(AUC_THREADS) void k_pd_rows(int n, int d, const float* __restrict__ Z, int64_t ldz, int centre,
                                                         float* __restrict__ Zn, int* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  int f = 0;
  for (int row = blockIdx.x * (AUC_THREADS / 64) + (threadIdx.x >> 6); row < n; row += gridDim.x * (AUC_THREADS / 64)) {
    const float* z = Z + row * ldz;
    bool bad = false;
    float sum = 0.f, lo = INFINITY, hi = -INFINITY;
    for (int k = lane; k < d; k += 64) {
      const float v = z[k];
      bad |= !auc_finite(v);
      sum = sum + v;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
    if (__ballot(bad)) { f |= AUC_BAD_FACTOR; continue; }      // wave-uniform
    if (!Zn) continue;
    float mean = 0.f;
    bool flat = false;
    if (centre) {
      mean = wave_sum(sum) / (float)d;
      flat = wave_min(lo) == wave_max(hi);
    }
    float ss = 0.f;
    for (int k = lane; k < d; k += 64) {
      const float c = flat ? 0.f : z[k] - mean;
      ss = fmaf(c, c, ss);
    }
    ss = wave_sum(ss);
    if (!auc_finite(ss)) f |= PD_NORM_OVERFLOW;
    const float den = fmaxf(sqrtf(ss), 1e-12f);
    for (int k = lane; k < d; k += 64) Zn[(int64_t)row * d + k] = (flat ? 0.f : z[k] - mean) / den;
  }
  if (f) atomicOr(flags, f);
}

// k_auc_classify / k_auc_emit with the scores of pd_for_each over the selected strict lower triangle
template <int M>
__global__ __launch_bounds__(AUC_THREADS) void k_pd_classify(int rows, int d, const float* __restrict__ Z, int64_t ldz,
                                                             const float* __restrict__ L, int64_t ldl,
                                                             const int64_t* __restrict__ idx, uint64_t* __restrict__ counts,
                                                             int* __restrict__ flags) {
  __shared__ PdShared sh;
  __shared__ uint64_t red[AUC_THREADS / 64];
  uint32_t pos = 0, tot = 0;
  int f = 0;
  pd_for_each<M, true>(rows, d, Z, ldz, L, ldl, idx, sh,
                       [&](int, int, int64_t, int64_t, float s, float l) { auc_classify_one(s, l, pos, tot, f); });
  auc_classify_end(pos, tot, f, red, counts, flags);
}

template <int M>
__global__ __launch_bounds__(AUC_THREADS) void k_pd_emit(int rows, int d, const float* __restrict__ Z, int64_t ldz,
                                                         const float* __restrict__ L, int64_t ldl,
                                                         const int64_t* __restrict__ idx, const uint64_t* __restrict__ offs,
                                                         uint32_t* __restrict__ keys) {
  __shared__ PdShared sh;
  __shared__ uint32_t cur[2];
  if (threadIdx.x < 2) cur[threadIdx.x] = 0;
  const uint64_t o_pos = offs[2 * blockIdx.x], o_neg = offs[2 * blockIdx.x + 1];
  pd_for_each<M, true>(rows, d, Z, ldz, L, ldl, idx, sh,
                       [&](int, int, int64_t, int64_t, float s, float l) { auc_emit_one(s, l, o_pos, o_neg, cur, keys); });
}

// out[i][j] = s_ij for all nodes, the diagonal included: every tile is computed where it is written (s_ij and s_ji are the
// same chain on swapped operands, hence the same bits), so that each store is a run of 16 consecutive floats
template <int M>
__global__ __launch_bounds__(AUC_THREADS) void k_pd_scores(int n, int d, const float* __restrict__ Z, int64_t ldz,
                                                           float* __restrict__ out, int64_t ldo) {
  __shared__ PdShared sh;
  pd_for_each<M, false>(n, d, Z, ldz, nullptr, 0, nullptr, sh,
                        [&](int, int, int64_t i, int64_t j, float s, float) { out[i * ldo + j] = s; });
}

namespace {
const char* const PD_NAMES[MCGRA_PAIR_METRICS] = {"cosine", "euclidean", "correlation", "chebyshev",
                                                   "braycurtis", "canberra", "cityblock", "sqeuclidean"};

// f.template operator()<M>() for the metric id
template <class F>
void pd_dispatch(int metric, F&& f) {
  switch (metric) {
    case M_COSINE: f.template operator()<M_COSINE>(); break;
    case M_EUCLIDEAN: f.template operator()<M_EUCLIDEAN>(); break;
    case M_CORRELATION: f.template operator()<M_CORRELATION>(); break;
    case M_CHEBYSHEV: f.template operator()<M_CHEBYSHEV>(); break;
    case M_BRAYCURTIS: f.template operator()<M_BRAYCURTIS>(); break;
    case M_CANBERRA: f.template operator()<M_CANBERRA>(); break;
    case M_CITYBLOCK: f.template operator()<M_CITYBLOCK>(); break;
    default: f.template operator()<M_SQEUCLIDEAN>(); break;
  }
}

struct PdClassify {
  hipStream_t st; int g, rows, d; const float* Z; int ldz; const float* L; int ldl; const int64_t* idx; uint64_t* counts; int* flags;
  template <int M> void operator()() const {
    k_pd_classify<M><<<g, AUC_THREADS, 0, st>>>(rows, d, Z, ldz, L, ldl, idx, counts, flags);
  }
};
struct PdEmit {
  hipStream_t st; int g, rows, d; const float* Z; int ldz; const float* L; int ldl; const int64_t* idx; const uint64_t* offs; uint32_t* keys;
  template <int M> void operator()() const {
    k_pd_emit<M><<<g, AUC_THREADS, 0, st>>>(rows, d, Z, ldz, L, ldl, idx, offs, keys);
  }
};
struct PdScores {
  hipStream_t st; int g, n, d; const float* Z; int ldz; float* out; int ldo;
  template <int M> void operator()() const { k_pd_scores<M><<<g, AUC_THREADS, 0, st>>>(n, d, Z, ldz, out, ldo); }
};

// The checks of Z that need the device, and the matrix the tile kernels read: Z, or (cosine, correlation) its normalised
// copy.  Synchronises: a refusal here comes before anything is ranked or written.
int pd_prepare(AucRun& run, int n, int d, const float*& Z, int& ldz, int metric) {
  if (int rc = run.begin()) return rc;
  float* Zn = nullptr;
  if (metric == M_COSINE || metric == M_CORRELATION) {
    Zn = run.b.get<float>((size_t)n * d);
    if (!Zn) { set_error("%s: hipMalloc of the normalised copy failed", run.who); return MCGRA_ENOMEM; }
  }
  k_pd_rows<<<std::min((n + 3) / 4, 1024), AUC_THREADS, 0, run.st>>>(n, d, Z, ldz, metric == M_CORRELATION, Zn, run.flags);
  MCGRA_KERNEL_CHECK();
  int f = 0;
  MCGRA_HIP(hipMemcpyAsync(&f, run.flags, sizeof(int), hipMemcpyDeviceToHost, run.st));
  MCGRA_HIP(hipStreamSynchronize(run.st));
  if (f & AUC_BAD_FACTOR) { set_error("%s: an entry of Z is NaN or infinite", run.who); return MCGRA_EINVAL; }
  if (f & PD_NORM_OVERFLOW) {
    set_error("%s: a row's sum of squares overflows float32 (%s)", run.who, PD_NAMES[metric]);
    return MCGRA_EINVAL;
  }
  if (Zn) { Z = Zn; ldz = d; }
  return 0;
}

bool pd_bad_factor(const char* who, int n, int d, const float* Z, int ldz, int metric) {
  if (metric < 0 || metric >= MCGRA_PAIR_METRICS) {
    set_error("%s: metric %d (0 .. %d: cosine, euclidean, correlation, chebyshev, braycurtis, canberra, cityblock, sqeuclidean)",
              who, metric, MCGRA_PAIR_METRICS - 1);
    return true;
  }
  if (n < 1 || d < 1 || !Z || ldz < d) { set_error("%s: bad argument (Z [n x d], n >= 1, d >= 1, ldz >= d)", who); return true; }
  return false;
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" const char* mcgra_pair_metric_name(int metric) {
  return metric >= 0 && metric < MCGRA_PAIR_METRICS ? PD_NAMES[metric] : nullptr;
}

extern "C" int mcgra_pair_distance_scores(void* stream, int n, int d, const float* Z, int ldz, int metric, float* out, int ld_out) {
  const char* who = "pair_distance_scores";
  if (pd_bad_factor(who, n, d, Z, ldz, metric)) return MCGRA_EINVAL;
  if (!out || ld_out < n) { set_error("%s: bad argument (out [n x n], ld_out >= n)", who); return MCGRA_EINVAL; }
  AucRun run{who, (hipStream_t)stream};
  if (int rc = pd_prepare(run, n, d, Z, ldz, metric)) return rc;
  const int ts = (n + PD_TILE - 1) / PD_TILE;
  const int g = (int)std::min<int64_t>((int64_t)ts * ts, PD_BLOCKS);
  pd_dispatch(metric, PdScores{run.st, g, n, d, Z, ldz, out, ld_out});
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipStreamSynchronize(run.st));     // the normalised copy is freed on return
  return 0;
}

extern "C" int mcgra_pair_distance_rank_metrics(void* stream, int n, int d, const float* Z, int ldz, int metric,
                                                const float* labels, int ld_labels, const int64_t* idx, int64_t n_idx,
                                                double* auc, double* ap, int64_t* counts) {
  const char* who = "pair_distance_rank_metrics";
  if (pd_bad_factor(who, n, d, Z, ldz, metric)) return MCGRA_EINVAL;
  if ((!auc && !ap) || !counts) { set_error("%s: bad argument (auc or ap, and counts)", who); return MCGRA_EINVAL; }
  if (int rc = rank_check_args(who, n, {{labels, ld_labels, true}}, idx, n_idx, 2)) return rc;
  AucRun run{who, (hipStream_t)stream};
  hipStream_t st = run.st;
  if (int rc = pd_prepare(run, n, d, Z, ldz, metric)) return rc;
  if (int rc = rank_check_idx(who, st, run.b, n, idx, n_idx, run.flags)) return rc;      // no repeats: a pair is two nodes
  const int rows = (int)n_idx;
  const int ts = (rows + PD_TILE - 1) / PD_TILE;
  const int g = (int)std::min<int64_t>((int64_t)ts * (ts + 1) / 2, PD_BLOCKS);
  pd_dispatch(metric, PdClassify{st, g, rows, d, Z, ldz, labels, ld_labels, idx, run.counts, run.flags});
  MCGRA_KERNEL_CHECK();
  double h_auc = 0.0, h_ap = 0.0;
  uint64_t pnt[3] = {0, 0, 0};
  // T is the pair count of the AUC, so that count always runs
  if (int rc = run.finish(g, [&](const uint64_t* offs, uint32_t* keys) {
        pd_dispatch(metric, PdEmit{st, g, rows, d, Z, ldz, labels, ld_labels, idx, offs, keys});
      }, &h_auc, ap ? &h_ap : nullptr, nullptr, pnt)) return rc;
  if (auc) *auc = h_auc;
  if (ap) *ap = h_ap;
  counts[0] = (int64_t)rows * (rows - 1) / 2;
  counts[1] = (int64_t)pnt[0];
  counts[2] = (int64_t)pnt[1];
  counts[3] = (int64_t)pnt[2];
  return 0;
}
