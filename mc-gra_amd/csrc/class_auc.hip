// What the attack knows beyond the node classes: the AUC of the edges against the non-edges of the SAME stratum, a stratum being
// a set of unordered class pairs, and the pairs above a cut per stratum (mcgra_class_auc).
//
// Candidates, selection, comparison and checks: those of mcgra_auc_delong (delong.hip) -- the m = n_idx (n_idx - 1) / 2
// unordered pairs of positions a > b of a repeat-free idx, score scores[idx[a]][idx[b]], label labels[idx[a]][idx[b]]; nothing
// outside the selected strict lower triangle is looked at; scores compare through auc_key (-0.0 == +0.0).
// The class of position a is node_class[idx[a]] in [0, C); the stratum of a candidate is strata[c_a][c_b] in [0, G), strata a
// symmetric host table.  Per stratum g: pairs_g, P_g (label 1), T_g = the sum over its non-edges q of b_q = 2 #{edges OF THE
// STRATUM that score higher} + #{edges of the stratum that score the same}, above_g (score >= threshold,
// mcgra_threshold_pairs' comparison) and hits_g (label 1 among those).
// Passes:
//   DlStage         (delong_common.hip) rank_check_idx; k_dl_classify: one read of the selected strict lower triangle, the
//                   argument checks (NaN / inf score, label other than 0 / 1) and per-block counts of the edges
//   k_ca_classes    the selected nodes' classes, read through idx once: cls[a] = node_class[idx[a]] as a byte by POSITION (what
//                   the two passes over the triangle read, coalesced), a class outside [0, C) flagged in a word of its own
//   k_ca_emit       k_dl_emit with the stratum as what travels with an edge's key
//   auc_sort        by key, the stratum as payload; then ONE more stable pass by the stratum's eight bits, the key as payload:
//                   the edges are stratum-major and ascending inside a stratum
//   k_ca_stream     ONE pass over the selected strict lower triangle.  Every block finds the segments seg[g] .. seg[g + 1] of the
//                   strata by G + 1 searches in the sorted strata (no count pass, no scan) and stages the table, the segment
//                   offsets and DL_STAGE samples of the sorted keys in LDS.  Every candidate counts for pairs, P, above and hits
//                   of its stratum; a non-edge finds its placement INSIDE its stratum's segment (delong_common.h's dl_placement
//                   through the samples, bounded to the segment) and adds it.  The counters
//                   are per block in LDS: the four counts as 32-bit words added once per wave for each of its first
//                   CA_SHARED_BINS distinct strata (ballots, as dl_hist_add: G = 2 puts a whole wave on two strata) and lane by
//                   lane for the strata left (G = 28 .. 136 scatters them); the sums b_q as 64-bit words in CA_TSLOTS copies
//                   per stratum, a lane adding to copy lane % CA_TSLOTS (at most 64 / CA_TSLOTS lanes meet on one address).
//                   At the end one 64-bit integer atomic per non-zero counter and block
// Integer arithmetic only: the same bits on every call, under any permutation of idx and under any renaming of the classes
// with their table.  `out` is written by the host once everything has come back and sum pairs_g = m, sum P_g = P hold.
// Device scratch: 16 bytes per edge (key, stratum and the sort's second buffers), about 3 MB for the sort's counts, 8 bytes
// per block of the row passes, one byte per selected node, and 4 bytes per node of the graph when idx is given.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/mcgra.h"
#include "common.h"
#include "delong_common.h"
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int CA_ROW_BLOCKS = 1024;                  // blocks of the passes over the selected rows (grid-stride)
constexpr int CA_CLASSES = MCGRA_CLASS_MAX;
constexpr int CA_STRATA = MCGRA_CLASS_MAX * (MCGRA_CLASS_MAX + 1) / 2;      // 136: one stratum per unordered class pair
constexpr int CA_SHARED_BINS = 2;                    // distinct strata of a wave whose counts are added once for the wave
constexpr int CA_TSLOTS = 16;                        // copies of a stratum's 64-bit sum in LDS
constexpr int CA_BAD_CLASS = 1;                      // the flag word of k_ca_classes
static_assert(CA_STRATA < 256, "a stratum is one digit of the sort");
static_assert((CA_TSLOTS & (CA_TSLOTS - 1)) == 0 && CA_TSLOTS <= 64, "a lane's copy is lane & (CA_TSLOTS - 1)");

enum { CA_PAIRS = 0, CA_P, CA_ABOVE, CA_HITS, CA_COUNTS };        // the 32-bit counters of a stratum
enum { CA_OUT_PAIRS = 0, CA_OUT_P, CA_OUT_T, CA_OUT_ABOVE, CA_OUT_HITS, CA_COLS };

// what follows the stage's counts on the device, then cls: one byte per selected position
struct CaHead {
  unsigned long long acc[CA_STRATA][CA_COLS];
  int class_flags, pad;
  uint8_t tab[CA_CLASSES * CA_CLASSES];              // strata[c_a][c_b] at c_a * C + c_b
};

// cls[a] = the class of position a; flags |= CA_BAD_CLASS for one outside [0, C) (idx was checked)
__global__ __launch_bounds__(AUC_THREADS) void k_ca_classes(int rows, int C, const int32_t* __restrict__ node_class,
                                                            const int64_t* __restrict__ idx, uint8_t* __restrict__ cls,
                                                            int* __restrict__ flags) {
  int f = 0;
  for (int a = blockIdx.x * AUC_THREADS + threadIdx.x; a < rows; a += gridDim.x * AUC_THREADS) {
    const int32_t c = node_class[idx ? idx[a] : (int64_t)a];
    const bool ok = c >= 0 && c < C;
    if (!ok) f |= CA_BAD_CLASS;
    cls[a] = ok ? (uint8_t)c : (uint8_t)0;
  }
  if (f) atomicOr(flags, f);
}

// k_dl_emit<false> whose second array holds the edge's stratum
__global__ __launch_bounds__(AUC_THREADS) void k_ca_emit(int rows, int C, const float* __restrict__ S, int64_t lds,
                                                         const float* __restrict__ L, int64_t ldl,
                                                         const int64_t* __restrict__ idx, const uint8_t* __restrict__ cls,
                                                         const uint8_t* __restrict__ tab_g, const uint64_t* __restrict__ offs,
                                                         uint32_t* __restrict__ ka, uint32_t* __restrict__ strat) {
  __shared__ uint32_t cur;
  __shared__ uint8_t tab[CA_CLASSES * CA_CLASSES];
  if (threadIdx.x == 0) cur = 0;
  if ((int)threadIdx.x < C * C) tab[threadIdx.x] = tab_g[threadIdx.x];
  __syncthreads();
  const uint64_t o_pos = offs[blockIdx.x];
  tri_for_each(rows, idx, [&](int a, int b, int64_t u, int64_t v) {
    const bool p = auc_pos(L[u * ldl + v]);
    const uint64_t at = o_pos + wave_slot(p, &cur);
    if (!p) return;
    ka[at] = auc_key(S[u * lds + v]);
    strat[at] = tab[cls[a] * C + cls[b]];
  });
}

// cnt[g][CA_PAIRS ..] += this candidate, for every lane that is active in the caller (the loop is the same in all of them).
// The lanes of the wave that share one of its first CA_SHARED_BINS distinct strata add once; the lanes left add on their own.
__device__ __forceinline__ void ca_count(uint32_t* __restrict__ cnt, uint32_t g, bool pos, bool above) {
  const int lane = threadIdx.x & 63;
  uint64_t todo = __ballot(true);
  const uint64_t mp = __ballot(pos), ma = __ballot(above);
  for (int it = 0; it < CA_SHARED_BINS && todo; ++it) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t lg = __shfl(g, leader, 64);
    const uint64_t same = __ballot(g == lg);
    if (lane == leader) {
      uint32_t* c = cnt + lg * CA_COUNTS;
      atomicAdd(&c[CA_PAIRS], (uint32_t)__popcll(same));
      if (same & mp) atomicAdd(&c[CA_P], (uint32_t)__popcll(same & mp));
      if (same & ma) atomicAdd(&c[CA_ABOVE], (uint32_t)__popcll(same & ma));
      if (same & mp & ma) atomicAdd(&c[CA_HITS], (uint32_t)__popcll(same & mp & ma));
    }
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) {
    uint32_t* c = cnt + g * CA_COUNTS;
    atomicAdd(&c[CA_PAIRS], 1u);
    if (pos) atomicAdd(&c[CA_P], 1u);
    if (above) atomicAdd(&c[CA_ABOVE], 1u);
    if (pos && above) atomicAdd(&c[CA_HITS], 1u);
  }
}

// The candidates, streamed: acc[g][CA_OUT_*] over the selected strict lower triangle.  sorted, strat: the np edges' keys and
// strata, stratum-major, the keys ascending inside a stratum; T: the key of the threshold.
__global__ __launch_bounds__(AUC_THREADS) void k_ca_stream(int rows, int C, int G, const float* __restrict__ S, int64_t lds,
                                                           const float* __restrict__ L, int64_t ldl,
                                                           const int64_t* __restrict__ idx, const uint8_t* __restrict__ cls,
                                                           const uint8_t* __restrict__ tab_g, const uint32_t* __restrict__ sorted,
                                                           const uint32_t* __restrict__ strat, uint32_t np, uint32_t T,
                                                           unsigned long long* __restrict__ acc) {
  __shared__ uint32_t smp[DL_STAGE];
  __shared__ unsigned long long tsum[CA_STRATA * CA_TSLOTS];
  __shared__ uint32_t cnt[CA_STRATA * CA_COUNTS];
  __shared__ uint32_t seg[CA_STRATA + 1];
  __shared__ uint8_t tab[CA_CLASSES * CA_CLASSES];
  const uint32_t stride = dl_stage(sorted, np, smp).stride;
  for (int q = threadIdx.x; q < G * CA_TSLOTS; q += AUC_THREADS) tsum[q] = 0;
  for (int q = threadIdx.x; q < G * CA_COUNTS; q += AUC_THREADS) cnt[q] = 0;
  if ((int)threadIdx.x <= G) seg[threadIdx.x] = rank_bound<false>(strat, 0u, np, (uint32_t)threadIdx.x);   // G + 1 <= 137 lanes
  if ((int)threadIdx.x < C * C) tab[threadIdx.x] = tab_g[threadIdx.x];
  __syncthreads();
  tri_for_each(rows, idx, [&](int a, int b, int64_t u, int64_t v) {
    const uint32_t g = tab[cls[a] * C + cls[b]];
    const uint32_t x = auc_key(S[u * lds + v]);
    const bool pos = auc_pos(L[u * ldl + v]);                    // the labels were checked
    if (!pos) {
      const uint32_t lo = seg[g], hi = seg[g + 1];
      if (lo < hi) {
        const uint64_t bq = dl_placement(sorted, smp, stride, dl_segment(lo, hi, stride), x);      // <= 2 P_g < 2^32
        if (bq) atomicAdd(&tsum[g * CA_TSLOTS + (threadIdx.x & (CA_TSLOTS - 1))], (unsigned long long)bq);
      }
    }
    ca_count(cnt, g, pos, x >= T);
  });
  __syncthreads();
  static_assert(CA_OUT_P == CA_P && CA_OUT_ABOVE == CA_ABOVE + 1 && CA_OUT_HITS == CA_HITS + 1, "T sits between P and above");
  for (int q = threadIdx.x; q < G * CA_COUNTS; q += AUC_THREADS) {
    const int c = q % CA_COUNTS;
    if (cnt[q]) atomicAdd(&acc[(q / CA_COUNTS) * CA_COLS + c + (c >= CA_ABOVE ? 1 : 0)], (unsigned long long)cnt[q]);
  }
  for (int g = threadIdx.x; g < G; g += AUC_THREADS) {
    unsigned long long t = 0;
    for (int q = 0; q < CA_TSLOTS; ++q) t += tsum[g * CA_TSLOTS + q];
    if (t) atomicAdd(&acc[g * CA_COLS + CA_OUT_T], t);
  }
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_class_auc(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                               const int64_t* idx, int64_t n_idx, const int32_t* node_class, int n_class, const uint8_t* strata,
                               int n_strata, float threshold, int64_t* out) {
  const char* who = "class_auc";
  if (!out || !node_class || !strata || threshold != threshold) {
    set_error("%s: bad argument%s", who, threshold != threshold ? " (the threshold is NaN)" : " (out, node_class or strata NULL)");
    return MCGRA_EINVAL;
  }
  if (n_class < 1 || n_class > MCGRA_CLASS_MAX || n_strata < 1 || n_strata > CA_STRATA) {
    set_error("%s: bad argument (n_class = %d, n_strata = %d; up to %d classes in [1, %d] strata)", who, n_class, n_strata,
              MCGRA_CLASS_MAX, CA_STRATA);
    return MCGRA_EINVAL;
  }
  const int C = n_class, G = n_strata;
  for (int i = 0; i < C; ++i)
    for (int j = 0; j <= i; ++j)
      if (strata[i * C + j] != strata[j * C + i] || strata[i * C + j] >= G) {
        set_error("%s: bad argument (strata[%d][%d] = %d, strata[%d][%d] = %d; the table is symmetric with entries below %d)",
                  who, i, j, (int)strata[i * C + j], j, i, (int)strata[j * C + i], G);
        return MCGRA_EINVAL;
      }
  if (int rc = rank_check_args(who, n, {{labels, ld_labels, true}, {scores, ld_scores, true}}, idx, n_idx, 2)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int m = (int)n_idx;
  AucBufs b;
  DlStage stage{who, st, b, n, labels, scores, nullptr, ld_labels, ld_scores, 0, idx, m, std::min(m - 1, CA_ROW_BLOCKS)};
  if (int rc = stage.start(sizeof(CaHead) + (size_t)m)) return rc;
  const int g = stage.g;
  CaHead* hd = (CaHead*)stage.extra;
  uint8_t* cls = stage.extra + sizeof(CaHead);
  uint8_t tab[CA_CLASSES * CA_CLASSES] = {};
  memcpy(tab, strata, (size_t)C * C);
  MCGRA_HIP(hipMemcpyAsync(hd->tab, tab, sizeof(tab), hipMemcpyHostToDevice, st));
  k_ca_classes<<<std::min(CA_ROW_BLOCKS, (m + AUC_THREADS - 1) / AUC_THREADS), AUC_THREADS, 0, st>>>(m, C, node_class, idx, cls,
                                                                                                     &hd->class_flags);
  MCGRA_KERNEL_CHECK();
  int class_flags = 0;
  MCGRA_HIP(hipMemcpyAsync(&class_flags, &hd->class_flags, sizeof(int), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (class_flags) {
    set_error("%s: a selected node's class is outside [0, %d)", who, C);
    return MCGRA_EINVAL;
  }
  if (int rc = stage.counted()) return rc;
  const uint64_t P = stage.P, N = stage.N;
  uint32_t *sorted = nullptr, *strat = nullptr;
  if (P) {
    Carver c{};
    if (int rc = stage.pool(4, 0, c, "edges")) return rc;              // the keys, the strata, the sort's second buffers
    uint32_t *ka = c.take<uint32_t>(stage.P4), *kb = c.take<uint32_t>(stage.P4);
    uint32_t *sa = c.take<uint32_t>(stage.P4), *sb = c.take<uint32_t>(stage.P4);
    k_ca_emit<<<g, AUC_THREADS, 0, st>>>(m, C, scores, ld_scores, labels, ld_labels, idx, cls, hd->tab, stage.counts, ka, sa);
    MCGRA_KERNEL_CHECK();
    if (int rc = auc_sort(st, ka, kb, P, stage.sort, sa, sb)) return rc;               // by key: back in ka, sa
    if (int rc = auc_sort(st, sa, sb, P, stage.sort, ka, kb, 8)) return rc;            // one pass by stratum: in sb, kb
    sorted = P > 1 ? kb : ka;                                                          // (fewer than two edges: nothing moved)
    strat = P > 1 ? sb : sa;
  }
  const uint32_t T = auc_key_host(threshold);
  k_ca_stream<<<g, AUC_THREADS, 0, st>>>(m, C, G, scores, ld_scores, labels, ld_labels, idx, cls, hd->tab, sorted, strat,
                                         (uint32_t)P, T, &hd->acc[0][0]);
  MCGRA_KERNEL_CHECK();
  std::vector<unsigned long long> ca((size_t)G * CA_COLS);
  MCGRA_HIP(hipMemcpyAsync(ca.data(), hd->acc, sizeof(unsigned long long) * ca.size(), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));                                  // the scratch is freed on return
  unsigned long long all = 0, pos = 0;
  for (int s = 0; s < G; ++s) { all += ca[s * CA_COLS + CA_OUT_PAIRS]; pos += ca[s * CA_COLS + CA_OUT_P]; }
  if (all != P + N || pos != P) {                                       // the stream and the classify pass read the same labels
    set_error("%s: internal error: the strata hold %llu candidates, %llu of them edges; the selection has %llu and %llu", who, all,
              pos, (unsigned long long)(P + N), (unsigned long long)P);
    return MCGRA_EHIP;
  }
  for (size_t q = 0; q < ca.size(); ++q) out[q] = (int64_t)ca[q];
  return 0;
}
