// Whether the recovered graph LOOKS like the real one: degree, triangle and wedge counts of the graph that a threshold cuts
// out of a scored square matrix, of the true graph and of their intersection (mcgra_graph_structure).
//
// Candidates, selection and checks: those of mcgra_threshold_pairs (two_means.hip) -- the pairs of positions a > b of a
// repeat-free idx of m nodes, score scores[idx[a]][idx[b]], label labels[idx[a]][idx[b]].  R has the edge {a, b} iff the score
// is >= threshold as float32 values (auc_key: -0.0 == +0.0, +-inf thresholds allowed); G iff the label is 1; C = R & G.
// For a graph X, d_X(v) is the degree of position v and t_X(v) the unordered {u, w} with vu, vw, uw all in X.
//
// The three graphs are bit matrices (bit_graph.h: the layout, the pack of a tile, the walk over a row's neighbours).
// Passes:
//   rank_check_idx  idx only: range check, repeats (rank_common.hip)
//   k_gs_pack       bg_pack_tile with the two bits "score >= threshold" (R) and "label is 1" (G) of a pair: the one read of
//                   the selected strict lower triangle.  The same pass does the argument checks (NaN / inf score, label other
//                   than 0 / 1) into the family's flag word and, given labels, writes G's matrix and C = R & G
//   k_gs_count      one block per (position v, graph): row v into LDS, d(v) = its popcount; wave w walks the neighbours u in
//                   the words w, w + 4, ... of row v (bg_for_each_neighbour); the lanes stride over row u's W words
//                   (coalesced) and add popc(row_u[k] & row_v[k]) in 64 bits; the block's sum is 2 t(v).  One writer per
//                   output
//   k_gs_totals     one block: sum d, sum t, sum d (d - 1) / 2 of each graph's columns
// Integer arithmetic only, every output has one writer: the same bits on every call, whatever order the blocks run in.
// `out` is written by k_gs_count alone, which is launched once every check has passed.
// Device scratch: m W 8 bytes per graph, one graph without labels and three with them (38 MB at m = 10 000, 1.6 GB at
// m = 65 535), about 100 bytes, and 4 bytes per node of the graph when idx is given.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "../../include/mcgra.h"
#include "bit_graph.h"
#include "common.h"
#include "rank_common.h"

namespace mcgra {
namespace {
struct GsState {
  unsigned long long tot[9];               // per graph: sum d, sum t, sum d (d - 1) / 2
  int flags;
};

// Tile (A, B), B <= A, of block p = A (A + 1) / 2 + B.  MR, MG, MC: the three bit matrices (MG, MC only with L).
__global__ __launch_bounds__(AUC_THREADS) void k_gs_pack(int m, int W, const float* __restrict__ S, int64_t lds,
                                                         const float* __restrict__ L, int64_t ldl,
                                                         const int64_t* __restrict__ idx, uint32_t T,
                                                         uint64_t* __restrict__ MR, uint64_t* __restrict__ MG,
                                                         uint64_t* __restrict__ MC, int* __restrict__ flags) {
  __shared__ uint64_t tile[2][BG_TILE];
  int f = 0;
  bg_pack_tile<2>(m, W, idx, tile, [&](int64_t u, int64_t v, bool (&bit)[2]) {
    const float s = S[u * lds + v];
    if (!auc_finite(s)) f |= AUC_BAD_SCORE;
    bit[0] = auc_key(s) >= T;
    if (L) {
      const float l = L[u * ldl + v];
      bit[1] = auc_pos(l);
      if (!bit[1] && !auc_neg(l)) f |= AUC_BAD_LABEL;             // also NaN
    }
  }, [&](size_t at, const uint64_t (&w)[2]) {
    MR[at] = w[0];
    if (L) { MG[at] = w[1]; MC[at] = w[0] & w[1]; }
  });
  if (f) atomicOr(flags, f);
}

// Block (v, g): d and t of position v in graph g (M + g * plane).  out row v = {d_R, t_R, d_G, t_G, d_C, t_C}; with one graph
// the block also writes the four -1.
__global__ __launch_bounds__(AUC_THREADS) void k_gs_count(int W, const uint64_t* __restrict__ M, size_t plane, int graphs,
                                                          int64_t* __restrict__ out) {
  __shared__ uint64_t row[BG_MAX_W];
  __shared__ uint64_t sh[BG_WAVES];
  const int v = blockIdx.x, g = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t* __restrict__ Mg = M + (size_t)g * plane;
  uint64_t deg = 0;
  for (int k = threadIdx.x; k < W; k += AUC_THREADS) {
    const uint64_t x = Mg[(size_t)v * W + k];
    row[k] = x;
    deg += (uint64_t)__popcll(x);
  }
  const uint64_t d = block_sum_u64(deg, sh);                      // (its barrier also publishes row[])
  uint64_t acc = 0;
  for (int j = wv; j < W; j += BG_WAVES)
    bg_for_each_neighbour(row[j], j, Mg, W, [&](auto& pu) {
      for (int k = lane; k < W; k += 64) {
        const uint64_t rv = row[k];
        uint64_t y[BG_BATCH];
#pragma unroll
        for (int q = 0; q < BG_BATCH; ++q) y[q] = pu[q][k];
#pragma unroll
        for (int q = 0; q < BG_BATCH; ++q) acc += (uint64_t)__popcll(y[q] & rv);
      }
    }, [&](const uint64_t* __restrict__ pu) {
      for (int k = lane; k < W; k += 64) acc += (uint64_t)__popcll(pu[k] & row[k]);
    });
  __syncthreads();                                                // sh is reused
  const uint64_t t2 = block_sum_u64(acc, sh);                     // every triangle through v from both of its other corners
  if (threadIdx.x == 0) {
    int64_t* o = out + (size_t)v * 6;
    o[2 * g] = (int64_t)d;
    o[2 * g + 1] = (int64_t)(t2 >> 1);
    if (graphs == 1) { o[2] = -1; o[3] = -1; o[4] = -1; o[5] = -1; }
  }
}

// st->tot[3 g + {0, 1, 2}] = sum d, sum t, sum d (d - 1) / 2 of graph g's two columns (one block)
__global__ __launch_bounds__(AUC_THREADS) void k_gs_totals(int m, int graphs, const int64_t* __restrict__ out,
                                                           GsState* __restrict__ st) {
  __shared__ uint64_t sh[BG_WAVES];
  for (int g = 0; g < graphs; ++g) {
    uint64_t sd = 0, stri = 0, sw = 0;
    for (int v = threadIdx.x; v < m; v += AUC_THREADS) {
      const uint64_t d = (uint64_t)out[(size_t)v * 6 + 2 * g], t = (uint64_t)out[(size_t)v * 6 + 2 * g + 1];
      sd += d;
      stri += t;
      sw += d * (d - (d ? 1 : 0)) / 2;
    }
    const uint64_t a = block_sum_u64(sd, sh);
    __syncthreads();
    const uint64_t b = block_sum_u64(stri, sh);
    __syncthreads();
    const uint64_t c = block_sum_u64(sw, sh);
    __syncthreads();
    if (threadIdx.x == 0) { st->tot[3 * g] = a; st->tot[3 * g + 1] = b; st->tot[3 * g + 2] = c; }
  }
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_graph_structure(void* stream, int n, const float* scores, int ld_scores, const float* labels,
                                     int ld_labels, const int64_t* idx, int64_t n_idx, float threshold, int64_t* header,
                                     int64_t* out) {
  const char* who = "graph_structure";
  if (!header || !out || threshold != threshold) {
    set_error("%s: bad argument%s", who, threshold != threshold ? " (the threshold is NaN)" : "");
    return MCGRA_EINVAL;
  }
  if (int rc = rank_check_args(who, n, {{scores, ld_scores, true}, {labels, ld_labels, false}}, idx, n_idx, 2)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int m = (int)n_idx, W = (m + 63) / 64, graphs = labels ? 3 : 1;
  const size_t plane = (size_t)m * W;
  AucBufs b;
  GsState* state = b.get<GsState>(1);
  uint64_t* M = b.get<uint64_t>(plane * graphs);
  if (!state || !M) {
    set_error("%s: hipMalloc of %d bit matrices of %d x %d words (%llu bytes) failed", who, graphs, m, W,
              (unsigned long long)(plane * graphs * sizeof(uint64_t)));
    return MCGRA_ENOMEM;
  }
  MCGRA_HIP(hipMemsetAsync(state, 0, sizeof(GsState), st));
  if (int rc = rank_check_idx(who, st, b, n, idx, m, &state->flags)) return rc;
  k_gs_pack<<<bg_tiles(W), AUC_THREADS, 0, st>>>(m, W, scores, ld_scores, labels, ld_labels, idx, auc_key_host(threshold), M,
                                                 labels ? M + plane : nullptr, labels ? M + 2 * plane : nullptr, &state->flags);
  MCGRA_KERNEL_CHECK();
  GsState h{};
  MCGRA_HIP(hipMemcpyAsync(&h, state, sizeof(GsState), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (int rc = rank_flag_error(who, h.flags)) return rc;
  k_gs_count<<<dim3((unsigned)m, (unsigned)graphs), AUC_THREADS, 0, st>>>(W, M, plane, graphs, out);
  k_gs_totals<<<1, AUC_THREADS, 0, st>>>(m, graphs, out, state);
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipMemcpyAsync(&h, state, sizeof(GsState), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));                                  // the scratch is freed on return
  int64_t r[9] = {(int64_t)m * (m - 1) / 2, -1, -1, -1, -1, -1, -1, -1, -1};
  for (int g = 0; g < graphs; ++g) {
    const int at = g == 0 ? 1 : g == 1 ? 4 : 7;                         // {E, T, W} of R, G; {E, T} of C
    r[at] = (int64_t)(h.tot[3 * g] / 2);
    r[at + 1] = (int64_t)(h.tot[3 * g + 1] / 3);
    if (g < 2) r[at + 2] = (int64_t)h.tot[3 * g + 2];
  }
  memcpy(header, r, sizeof(r));
  return 0;
}
