// Where the attack's errors sit: the AUC of the edges against the non-edges at each distance of the TRUE graph, and the
// false positives of a cut split by that distance (mcgra_hop_auc).
//
// Candidates, selection, comparison and checks: those of mcgra_auc_delong (delong.hip) -- the m = n_idx (n_idx - 1) / 2
// unordered pairs of positions a > b of a repeat-free idx, score scores[idx[a]][idx[b]], label labels[idx[a]][idx[b]]; nothing
// outside the selected strict lower triangle is looked at; scores compare through auc_key (-0.0 == +0.0).
// G is the graph on the selected positions whose edges are the candidates of label 1 (mcgra_graph_structure's G), dist the
// shortest-path length in G: the INDUCED subgraph, a path through an unselected node does not exist.  With H = hops a
// candidate is of class d = dist for d = 1 .. H (class 1: the edges) and of class H + 1, "beyond", when dist > H or there is
// no path.  Per class c: pairs_c, above_c = those with score >= threshold (mcgra_threshold_pairs' comparison) and, for
// c >= 2, T_c = the sum over the class's candidates q of b_q = 2 #{edges that score higher} + #{edges that score the same}.
//
// A graph is a bit matrix (bit_graph.h).  reach_h has bit (a, b) iff a walk of 1 .. h edges joins a and b, so for a != b iff
// dist(a, b) <= h (its diagonal is set from h = 2 on: there and back; no pass reads it).
// Passes:
//   DlStage         (delong_common.hip) rank_check_idx; k_dl_classify: one read of the selected strict lower triangle, the
//                   argument checks (NaN / inf score, label other than 0 / 1) and per-block counts of the positives; later
//                   k_dl_emit: the positives' keys to their slots; auc_sort sorts them in place
//   k_ha_pack       bg_pack_tile with the one bit "label is 1": reach_1 = G
//   k_ha_expand     H - 1 times, from level h's matrix into level h + 1's: one block per row a.  reach_h+1[a] = reach_h[a] |
//                   OR over the neighbours u of a in G of reach_h[u].  The neighbours are the set bits of G's row a (in LDS,
//                   bg_for_each_neighbour); lane t owns the words t, t + 256, .. of the row and ORs the same words of every
//                   neighbour's row in (coalesced).  One writer per word, no atomics, never in place
//   k_ha_stream     ONE pass over the selected strict lower triangle that reads all H levels: the class of a candidate is
//                   H - #{levels whose bit (a, b) is set} (the levels are nested), 0 for an edge; a non-edge finds its
//                   placement among the sorted positives (delong_common.h's dl_placement through samples in LDS).  Per class
//                   pairs, T and above accumulate in registers, then block_add_u64: one 64-bit integer atomic per class,
//                   quantity and block
// Integer arithmetic only: the same bits on every call and under any permutation of idx.  `out` is written by the host once
// everything has come back.
// Device scratch: H bit matrices of 8 m W bytes (all levels are kept for the one stream pass; H = 3: 38 MB at m = 10 000, 1.6 GB
// at m = 65 535), 8 bytes per positive (its key and the sort's second buffer), about 3 MB for the sort's counts, 8 bytes per
// block of the row passes, and 4 bytes per node of the graph when idx is given.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "../../include/mcgra.h"
#include "bit_graph.h"
#include "common.h"
#include "delong_common.h"
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int HA_LANE_WORDS = BG_MAX_W / AUC_THREADS;          // words of a row a lane of the expansion owns, at most
constexpr int HA_ROW_BLOCKS = 1024;                  // blocks of the passes over the selected rows (grid-stride)
constexpr int HA_CLASSES = MCGRA_HOP_MAX + 1;        // distances 1 .. MCGRA_HOP_MAX and beyond
static_assert(HA_LANE_WORDS * AUC_THREADS == BG_MAX_W, "the lanes of one block cover a row of the capacity");

enum { HA_PAIRS = 0, HA_T, HA_ABOVE, HA_COLS };

// Tile (A, B), B <= A, of block p = A (A + 1) / 2 + B: G's words (row a, word B) and (row b, word A).  The labels were checked.
__global__ __launch_bounds__(AUC_THREADS) void k_ha_pack(int m, int W, const float* __restrict__ L, int64_t ldl,
                                                         const int64_t* __restrict__ idx, uint64_t* __restrict__ MG) {
  __shared__ uint64_t tile[1][BG_TILE];
  bg_pack_tile<1>(m, W, idx, tile, [&](int64_t u, int64_t v, bool (&bit)[1]) { bit[0] = auc_pos(L[u * ldl + v]); },
                  [&](size_t at, const uint64_t (&w)[1]) { MG[at] = w[0]; });
}

// Block v: out row v = in row v | the rows of `in` of v's neighbours in G.
__global__ __launch_bounds__(AUC_THREADS) void k_ha_expand(int W, const uint64_t* __restrict__ G, const uint64_t* __restrict__ in,
                                                           uint64_t* __restrict__ out) {
  __shared__ uint64_t row[BG_MAX_W];
  const size_t v = blockIdx.x;
  uint64_t acc[HA_LANE_WORDS];
#pragma unroll
  for (int q = 0; q < HA_LANE_WORDS; ++q) {
    const int k = threadIdx.x + q * AUC_THREADS;
    acc[q] = 0;
    if (k < W) {
      row[k] = G[v * W + k];
      acc[q] = in[v * W + k];
    }
  }
  __syncthreads();
  for (int j = 0; j < W; ++j)
    bg_for_each_neighbour(row[j], j, in, W, [&](auto& pu) {
#pragma unroll
      for (int q = 0; q < HA_LANE_WORDS; ++q) {
        const int k = threadIdx.x + q * AUC_THREADS;
        if (k < W) {
          uint64_t y[BG_BATCH];
#pragma unroll
          for (int s = 0; s < BG_BATCH; ++s) y[s] = pu[s][k];
#pragma unroll
          for (int s = 0; s < BG_BATCH; ++s) acc[q] |= y[s];
        }
      }
    }, [&](const uint64_t* __restrict__ pu) {
#pragma unroll
      for (int q = 0; q < HA_LANE_WORDS; ++q) {
        const int k = threadIdx.x + q * AUC_THREADS;
        if (k < W) acc[q] |= pu[k];
      }
    });
#pragma unroll
  for (int q = 0; q < HA_LANE_WORDS; ++q) {
    const int k = threadIdx.x + q * AUC_THREADS;
    if (k < W) out[v * W + k] = acc[q];
  }
}

// The candidates, streamed: acc[class][HA_PAIRS / HA_T / HA_ABOVE] over the selected strict lower triangle.  M: the H levels,
// `plane` words apart; sorted: the np positives' keys, ascending; T: the key of the threshold.
__global__ __launch_bounds__(AUC_THREADS) void k_ha_stream(int rows, int W, int H, const float* __restrict__ S, int64_t lds,
                                                           const int64_t* __restrict__ idx, const uint64_t* __restrict__ M,
                                                           size_t plane, const uint32_t* __restrict__ sorted, uint32_t np,
                                                           uint32_t T, unsigned long long* __restrict__ acc) {
  __shared__ uint32_t smp[DL_STAGE];
  __shared__ uint64_t sh[AUC_THREADS / 64];
  const DlSamples sm = dl_stage(sorted, np, smp);
  __syncthreads();
  uint32_t cnt[HA_CLASSES] = {}, abv[HA_CLASSES] = {};           // a lane sees fewer than 2^32 candidates
  uint64_t sum[HA_CLASSES] = {};
  tri_for_each(rows, idx, [&](int a, int b, int64_t u, int64_t v) {
    const uint32_t x = auc_key(S[u * lds + v]);
    const size_t at = (size_t)a * W + (b >> 6);
    int cls = H;                                                 // the levels are nested: H - #{levels that hold the pair}
    for (int h = 0; h < H; ++h) cls -= (int)((M[h * plane + at] >> (b & 63)) & 1ull);
    uint64_t bq = 0;
    if (cls > 0 && np) bq = dl_placement(sorted, smp, sm.stride, dl_all(np, sm), x);
    const bool above = x >= T;
#pragma unroll
    for (int c = 0; c < HA_CLASSES; ++c) {
      const bool hit = cls == c;
      cnt[c] += hit ? 1u : 0u;
      abv[c] += (hit && above) ? 1u : 0u;
      sum[c] += hit ? bq : 0ull;
    }
  });
#pragma unroll
  for (int c = 0; c < HA_CLASSES; ++c) {
    if (c <= H) {                                                // the same in every lane
      const uint64_t part[HA_COLS] = {cnt[c], sum[c], abv[c]};
      block_add_u64(part, sh, acc + c * HA_COLS);
    }
  }
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_hop_auc(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                             const int64_t* idx, int64_t n_idx, int hops, float threshold, int64_t* out) {
  const char* who = "hop_auc";
  if (!out || threshold != threshold) {
    set_error("%s: bad argument%s", who, threshold != threshold ? " (the threshold is NaN)" : " (out NULL)");
    return MCGRA_EINVAL;
  }
  if (hops < 1 || hops > MCGRA_HOP_MAX) {
    set_error("%s: bad argument (hops = %d; distances are told apart up to hops in [1, %d])", who, hops, MCGRA_HOP_MAX);
    return MCGRA_EINVAL;
  }
  if (int rc = rank_check_args(who, n, {{labels, ld_labels, true}, {scores, ld_scores, true}}, idx, n_idx, 2)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int m = (int)n_idx, W = (m + 63) / 64, H = hops;
  const size_t plane = (size_t)m * W;
  AucBufs b;
  uint64_t* M = b.get<uint64_t>(plane * H);
  if (!M) {
    set_error("%s: hipMalloc of %d bit matrices of %d x %d words (%llu bytes) failed", who, H, m, W,
              (unsigned long long)(plane * H * sizeof(uint64_t)));
    return MCGRA_ENOMEM;
  }
  DlStage stage{who, st, b, n, labels, scores, nullptr, ld_labels, ld_scores, 0, idx, m, std::min(m - 1, HA_ROW_BLOCKS)};
  typedef unsigned long long Acc[HA_CLASSES][HA_COLS];
  if (int rc = stage.start(sizeof(Acc))) return rc;
  if (int rc = stage.counted()) return rc;
  const uint64_t P = stage.P, N = stage.N;
  const int g = stage.g;
  k_ha_pack<<<bg_tiles(W), AUC_THREADS, 0, st>>>(m, W, labels, ld_labels, idx, M);
  for (int lv = 1; lv < H; ++lv) k_ha_expand<<<m, AUC_THREADS, 0, st>>>(W, M, M + (lv - 1) * plane, M + lv * plane);
  MCGRA_KERNEL_CHECK();
  uint32_t* sorted = nullptr;
  if (P) {
    Carver c{};
    if (int rc = stage.pool(2, 0, c)) return rc;                        // the keys, the sort's second buffer
    sorted = c.take<uint32_t>(stage.P4);
    if (int rc = stage.emit(sorted, nullptr)) return rc;
    if (int rc = auc_sort(st, sorted, c.take<uint32_t>(stage.P4), P, stage.sort)) return rc;
  }
  const uint32_t T = auc_key_host(threshold);
  k_ha_stream<<<g, AUC_THREADS, 0, st>>>(m, W, H, scores, ld_scores, idx, M, plane, sorted, (uint32_t)P, T, (unsigned long long*)stage.extra);
  MCGRA_KERNEL_CHECK();
  Acc ha;
  MCGRA_HIP(hipMemcpyAsync(ha, stage.extra, sizeof(ha), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));                                  // the scratch is freed on return
  unsigned long long all = 0, t1 = 0;
  for (int c = 0; c <= H; ++c) { all += ha[c][HA_PAIRS]; t1 += ha[c][HA_T]; }
  if (ha[0][HA_PAIRS] != P || all != P + N || ha[0][HA_T] != 0) {       // the bit matrix and the classify pass read the same labels
    set_error("%s: internal error: the classes hold %llu candidates, %llu of them edges; the selection has %llu and %llu", who,
              all, ha[0][HA_PAIRS], (unsigned long long)(P + N), (unsigned long long)P);
    return MCGRA_EHIP;
  }
  ha[0][HA_T] = t1;                                                     // T_1 = the sum over the other classes: mcgra_auc_delong's T
  int64_t r[HA_CLASSES * HA_COLS];
  for (int c = 0; c <= H; ++c)
    for (int q = 0; q < HA_COLS; ++q) r[c * HA_COLS + q] = (int64_t)ha[c][q];
  memcpy(out, r, sizeof(int64_t) * HA_COLS * (size_t)(H + 1));
  return 0;
}
