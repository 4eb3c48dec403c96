// Which edges leak: every true edge's own placement among the non-edges, tied to where the edge sits in the TRUE graph -- the
// common neighbours of its two ends and the smaller of their degrees -- reduced per stratum and handed out edge by edge
// (mcgra_edge_exposure).  The positives' side of what hop_auc.hip does for the negatives.
//
// Candidates, selection, comparison and checks: those of mcgra_auc_delong (delong.hip) -- the m = n_idx (n_idx - 1) / 2
// unordered pairs of positions a > b of a repeat-free idx, score scores[idx[a]][idx[b]], label labels[idx[a]][idx[b]]; nothing
// outside the selected strict lower triangle is looked at; scores compare through auc_key (-0.0 == +0.0).
// G is the graph on the selected positions whose edges are the candidates of label 1 (mcgra_graph_structure's G): the INDUCED
// subgraph, a neighbour that is not selected does not exist.  For every edge e = {a, b} of G:
//   a_e = 2 #{non-edges that score lower} + #{non-edges that score the same}, mcgra_auc_delong's placement of a positive
//   c_e = |N(a) & N(b)| in G, the triangles through the edge; its class ec = min(c_e, 15)
//   d_e = min(deg(a), deg(b)) in G; its class dc = min(15, bit_length(d_e)) >= 1
// table[ec][dc] = {edges, sum of a_e, edges with score >= threshold}.
//
// Passes:
//   DlStage         (delong_common.hip) rank_check_idx; k_dl_classify: one read of the selected strict lower triangle, the
//                   argument checks, the positives per block and per position: the degrees in G
//   k_ee_pack       bg_pack_tile with the one bit "label is 1": G as a bit matrix (bit_graph.h)
//   k_dl_emit       (DlStage) a second read of the labels: each positive's key and its ends a << 16 | b to a slot of its
//                   block's range (any order inside a block).  a << 16 | b orders as the packed position a (a - 1) / 2 + b does
//   auc_sort        twice: the keys, ascending (the placements are searched there), and the ends, ascending -- THE ORDER OF THE
//                   EDGE LIST, decided by this sort and never by an atomic
//   k_ee_negatives  a third read: every non-edge finds its place among the sorted keys (delong_common.h: samples in LDS) and
//                   counts itself into hist / ties; the candidates at or above the threshold are counted per label
//   rank_scan       the running sum of hist
//   k_ee_edges      one WAVE per edge of the sorted list: the lanes stride the W words of the two rows, popcounts of the AND, one
//                   wave sum: c_e.  Lane 0 reads the two degrees and the edge's score, finds its key among the sorted keys,
//                   forms a_e = 2 cum - ties, writes the edge's columns and adds to its cell of the block's table in LDS
//                   (6 KB); the block then merges its non-zero cells: one 64-bit integer atomic per cell and block
// Integer arithmetic only: the same bits on every call, the header and the table the same under any permutation of idx.  The
// host writes header and table once everything has come back.
// Device scratch: one bit matrix of 8 m W bytes (W = ceil(m / 64): 13 MB at m = 10 000, 537 MB at m = 65 535), 28 bytes per
// positive (its key, the sort's second buffer, hist, ties, the 8-byte running sum, its ends), about 3 MB for the sort's counts,
// 8 bytes per block of the row passes, 4 bytes per selected node, 6 KB of accumulators, and 4 bytes per node of the graph when idx
// is given.
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
constexpr int EE_ROW_BLOCKS = 1024;                  // blocks of the passes over the selected rows (grid-stride)
constexpr int EE_EDGE_BLOCKS = 1024;                 // at most this many blocks of the pass over the edges (grid-stride), a wave an edge
constexpr int EE_CLASSES = MCGRA_EXPOSURE_CLASSES;   // classes of either axis of the table
constexpr int EE_COLS = 3;                           // edges, sum of placements, edges at or above the threshold
constexpr int EE_CELLS = EE_CLASSES * EE_CLASSES * EE_COLS;
static_assert(AUC_MAX_NIDX < (1 << 16), "a position fits 16 bits: the ends of an edge travel as a << 16 | b");

enum { EE_T_NEG = 0, EE_ABOVE_POS, EE_ABOVE_NEG, EE_ACC };

// Tile (A, B), B <= A, of block p = A (A + 1) / 2 + B: G's words (row a, word B) and (row b, word A).  The labels were checked.
__global__ __launch_bounds__(AUC_THREADS) void k_ee_pack(int m, int W, const float* __restrict__ L, int64_t ldl,
                                                         const int64_t* __restrict__ idx, uint64_t* __restrict__ MG) {
  __shared__ uint64_t tile[1][BG_TILE];
  bg_pack_tile<1>(m, W, idx, tile, [&](int64_t u, int64_t v, bool (&bit)[1]) { bit[0] = auc_pos(L[u * ldl + v]); },
                  [&](size_t at, const uint64_t (&w)[1]) { MG[at] = w[0]; });
}

// The non-edges, streamed: hist / ties of s over the np sorted keys, acc[EE_T_NEG] += their placements (the edges' placements
// must sum to the same), acc[EE_ABOVE_*] += the candidates of either label whose key is at or above T.
__global__ __launch_bounds__(AUC_THREADS) void k_ee_negatives(int rows, DlSide s, const float* __restrict__ L, int64_t ldl,
                                                              const int64_t* __restrict__ idx, uint32_t np, uint32_t T,
                                                              unsigned long long* __restrict__ acc) {
  __shared__ uint32_t smp[DL_STAGE];
  __shared__ uint64_t sh[AUC_THREADS / 64];
  const DlSamples sm = dl_stage(s.sorted, np, smp);
  __syncthreads();
  uint64_t part[EE_ACC] = {};
  tri_for_each(rows, idx, [&](int, int, int64_t u, int64_t v) {
    const float x = s.S[u * s.ld + v];
    const bool neg = !auc_pos(L[u * ldl + v]);                 // the labels were checked: 0 or 1
    const uint64_t b = dl_negative(s, np, smp, sm, x, neg);
    const uint64_t above = auc_key(x) >= T ? 1u : 0u;
    part[EE_T_NEG] += neg ? b : 0ull;
    part[EE_ABOVE_POS] += neg ? 0ull : above;
    part[EE_ABOVE_NEG] += neg ? above : 0ull;
  });
  block_add_u64(part, sh, acc);
}

// the per-edge columns (all NULL: the table alone; pairs != NULL: each of the others may still be NULL)
struct EeColumns {
  int64_t* pairs;
  float* scores;
  int64_t* placement;
  int32_t* common;
  int32_t* deg;
};

// Edge e of the np sorted ends, one wave each: its row of the columns and its share of table[ec][dc][EE_COLS].
__global__ __launch_bounds__(AUC_THREADS) void k_ee_edges(int W, const uint64_t* __restrict__ MG, const uint32_t* __restrict__ degree,
                                                          DlSide s, const uint32_t* __restrict__ ends, uint32_t np,
                                                          const int64_t* __restrict__ idx, uint32_t T, EeColumns out,
                                                          unsigned long long* __restrict__ table) {
  __shared__ unsigned long long cell[EE_CELLS];
  for (int i = threadIdx.x; i < EE_CELLS; i += AUC_THREADS) cell[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (uint64_t e = (uint64_t)blockIdx.x * BG_WAVES + wv; e < np; e += (uint64_t)gridDim.x * BG_WAVES) {
    const uint32_t ab = ends[e], a = ab >> 16, b = ab & 0xffffu;                  // the same in every lane of the wave
    const uint64_t* __restrict__ ra = MG + (size_t)a * W;
    const uint64_t* __restrict__ rb = MG + (size_t)b * W;
    uint64_t cnt = 0;
    for (int k = lane; k < W; k += 64) cnt += (uint64_t)__popcll(ra[k] & rb[k]);
    cnt = wave_sum_u64(cnt);
    if (lane == 0) {                                                              // the wave's one writer
      const uint32_t c = (uint32_t)cnt, da = degree[a], db = degree[b];
      const int64_t u = idx ? idx[a] : (int64_t)a, v = idx ? idx[b] : (int64_t)b;
      const float score = s.S[u * s.ld + v];
      const uint32_t x = auc_key(score);
      const uint32_t l = rank_bound<false>(s.sorted, 0u, np, x);                    // its own key is there: l < np
      const uint64_t place = 2 * (s.cum[l] + s.hist[l]) - s.ties[l];                // dl_positive's a, <= 2 N
      const uint32_t d = min(da, db);                                               // >= 1: the edge itself
      const int ec = (int)min(c, (uint32_t)(EE_CLASSES - 1)), dc = min(EE_CLASSES - 1, 32 - __clz((int)d));
      unsigned long long* q = cell + (ec * EE_CLASSES + dc) * EE_COLS;
      atomicAdd(q, 1ull);
      if (place) atomicAdd(q + 1, (unsigned long long)place);
      if (x >= T) atomicAdd(q + 2, 1ull);
      if (out.pairs) {
        out.pairs[2 * e] = u;
        out.pairs[2 * e + 1] = v;
        if (out.scores) out.scores[e] = score;
        if (out.placement) out.placement[e] = (int64_t)place;
        if (out.common) out.common[e] = (int32_t)c;
        if (out.deg) { out.deg[2 * e] = (int32_t)da; out.deg[2 * e + 1] = (int32_t)db; }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < EE_CELLS; i += AUC_THREADS)
    if (cell[i]) atomicAdd(&table[i], cell[i]);
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_edge_exposure(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                                   const int64_t* idx, int64_t n_idx, float threshold, int64_t cap, int64_t* pairs,
                                   float* pair_scores, int64_t* placement, int32_t* common, int32_t* deg, int64_t* header,
                                   int64_t* table) {
  const char* who = "edge_exposure";
  if (!header || !table || threshold != threshold) {
    set_error("%s: bad argument%s", who, threshold != threshold ? " (the threshold is NaN)" : " (header or table NULL)");
    return MCGRA_EINVAL;
  }
  if (cap < 0 || (cap > 0 && !pairs) || (cap == 0 && (pairs || pair_scores || placement || common || deg))) {
    set_error("%s: bad argument (cap = %lld%s)", who, (long long)cap,
              cap < 0 ? "" : cap > 0 ? " with pairs NULL" : " with a column given");
    return MCGRA_EINVAL;
  }
  if (int rc = rank_check_args(who, n, {{labels, ld_labels, true}, {scores, ld_scores, true}}, idx, n_idx, 2)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int m = (int)n_idx, W = (m + 63) / 64;
  AucBufs b;
  uint64_t* MG = b.get<uint64_t>((size_t)m * W);
  if (!MG) {
    set_error("%s: hipMalloc of the bit matrix of %d x %d words (%llu bytes) failed", who, m, W,
              (unsigned long long)((size_t)m * W * sizeof(uint64_t)));
    return MCGRA_ENOMEM;
  }
  DlStage stage{who, st, b, n, labels, scores, nullptr, ld_labels, ld_scores, 0, idx, m, std::min(m - 1, EE_ROW_BLOCKS)};
  typedef unsigned long long Acc[EE_CELLS + EE_ACC];                    // the table, then the stream's three counters
  if (int rc = stage.start(sizeof(Acc) + sizeof(uint32_t) * (size_t)m, sizeof(Acc))) return rc;      // and the degrees in G
  if (int rc = stage.counted()) return rc;
  const uint64_t P = stage.P, N = stage.N;
  const bool rows_out = cap > 0 && (uint64_t)cap >= P;                  // cap < P: the integers alone, then MCGRA_ENOMEM
  unsigned long long* acc = (unsigned long long*)stage.extra;
  k_ee_pack<<<bg_tiles(W), AUC_THREADS, 0, st>>>(m, W, labels, ld_labels, idx, MG);
  MCGRA_KERNEL_CHECK();
  Carver c{};
  if (int rc = stage.pool(3, 4, c)) return rc;                          // the keys, the sort's second buffer, the ends | cum, hist, ties
  DlSide side{};
  side.S = scores;
  side.ld = ld_scores;
  side.cum = c.take<uint64_t>(stage.H4);
  side.sorted = c.take<uint32_t>(stage.P4);
  side.hist = c.take<uint32_t>(stage.H4);
  side.ties = c.take<uint32_t>(stage.H4);
  uint32_t* tmp = c.take<uint32_t>(stage.P4);
  uint32_t* ends = c.take<uint32_t>(stage.P4);
  MCGRA_HIP(hipMemsetAsync(side.hist, 0, sizeof(uint32_t) * 2 * stage.H4, st));       // hist and ties are adjacent
  if (P) {
    if (int rc = stage.emit(side.sorted, ends)) return rc;             // the keys, and the ends a << 16 | b
    if (int rc = auc_sort(st, side.sorted, tmp, P, stage.sort)) return rc;
    if (int rc = auc_sort(st, ends, tmp, P, stage.sort)) return rc;
  }
  const uint32_t T = auc_key_host(threshold);
  k_ee_negatives<<<stage.g, AUC_THREADS, 0, st>>>(m, side, labels, ld_labels, idx, (uint32_t)P, T, acc + EE_CELLS);
  MCGRA_KERNEL_CHECK();
  if (P) {
    rank_scan(st, side.hist, (int)P, side.cum);
    const EeColumns out = rows_out ? EeColumns{pairs, pair_scores, placement, common, deg} : EeColumns{};
    const int gp = (int)std::min<uint64_t>(EE_EDGE_BLOCKS, (P + BG_WAVES - 1) / BG_WAVES);
    k_ee_edges<<<gp, AUC_THREADS, 0, st>>>(W, MG, stage.deg, side, ends, (uint32_t)P, idx, T, out, acc);
    MCGRA_KERNEL_CHECK();
  }
  Acc ha;
  MCGRA_HIP(hipMemcpyAsync(ha, acc, sizeof(Acc), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));                                  // the scratch is freed on return
  unsigned long long cells = 0, t = 0, above = 0;
  for (int q = 0; q < EE_CELLS; q += EE_COLS) { cells += ha[q]; t += ha[q + 1]; above += ha[q + 2]; }
  const unsigned long long* tail = ha + EE_CELLS;
  if (cells != P || t != tail[EE_T_NEG] || above != tail[EE_ABOVE_POS]) {     // the two sides of the placements, the two reads of the labels
    set_error("%s: internal error: the table holds %llu edges, T = %llu, %llu above; the stream has %llu, %llu and %llu", who, cells,
              t, above, (unsigned long long)P, tail[EE_T_NEG], tail[EE_ABOVE_POS]);
    return MCGRA_EHIP;
  }
  const int64_t hd[6] = {(int64_t)(P + N), (int64_t)P, (int64_t)N, (int64_t)t, (int64_t)above, (int64_t)tail[EE_ABOVE_NEG]};
  int64_t tb[EE_CELLS];
  for (int q = 0; q < EE_CELLS; ++q) tb[q] = (int64_t)ha[q];
  memcpy(header, hd, sizeof(hd));
  memcpy(table, tb, sizeof(tb));
  if (cap > 0 && !rows_out) {
    set_error("%s: %llu edges, the columns hold cap = %lld rows (header[1] says what is needed)", who, (unsigned long long)P,
              (long long)cap);
    return MCGRA_ENOMEM;
  }
  return 0;
}
