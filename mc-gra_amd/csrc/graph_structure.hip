// Whether the recovered graph LOOKS like the real one: degree, triangle and wedge counts of the graph that a threshold cuts
// out of a scored square matrix, of the true graph and of their intersection (mcgra_graph_structure).
//
// Candidates, selection and checks: those of mcgra_threshold_pairs (two_means.hip) -- the pairs of positions a > b of a
// repeat-free idx of m nodes, score scores[idx[a]][idx[b]], label labels[idx[a]][idx[b]].  R has the edge {a, b} iff the score
// is >= threshold as float32 values (auc_key: -0.0 == +0.0, +-inf thresholds allowed); G iff the label is 1; C = R & G.
// For a graph X, d_X(v) is the degree of position v and t_X(v) the unordered {u, w} with vu, vw, uw all in X.
//
// A graph is a row-major BIT matrix: m rows of W = ceil(m / 64) 64-bit words, bit (a, b) at word b / 64 of row a, bit b % 64;
// symmetric, zero diagonal, zero pad bits at positions >= m.  One AND + popcount then tests 64 pairs.
// Passes:
//   rank_check_idx  idx only: range check, repeats (rank_common.hip)
//   k_gs_pack       the one read of the selected strict lower triangle, in 64 x 64 tiles of positions (A, B), B <= A: one block a
//                   tile, a wave 16 of its rows, lane = column.  __ballot of "a > b, a < m, score >= threshold" IS the word (row
//                   a, word B).  The tile's 64 words are parked in LDS; every lane reads the word of ITS row and a second
//                   ballot per column gives the mirrored word (row b, word A).  The diagonal tile ORs both halves before its one
//                   store.  Every word of the matrix has exactly one writer: plain vector stores, no atomics, no memset.  The
//                   same pass does the argument checks (NaN / inf score, label other than 0 / 1) into the family's flag word
//                   and, given labels, writes G's matrix and C = R & G
//   k_gs_count      one block per (position v, graph): row v into LDS, d(v) = its popcount; wave w walks the set bits u of the
//                   words w, w + 4, ... of row v, eight neighbours of a word at a time while it holds as many (their loads in
//                   flight together: a hub's row is one block's work), then one at a time; the lanes stride over row u's W
//                   words (coalesced) and add popc(row_u[k] & row_v[k]) in 64 bits; the block's sum is 2 t(v).  One writer
//                   per output
//   k_gs_totals     one block: sum d, sum t, sum d (d - 1) / 2 of each graph's columns
// Integer arithmetic only, every output has one writer: the same bits on every call, whatever order the blocks run in.
// `out` is written by k_gs_count alone, which is launched once every check has passed.
// Device scratch: m W 8 bytes per graph, one graph without labels and three with them (38 MB at m = 10 000, 1.6 GB at
// m = 65 535), about 100 bytes, and 4 bytes per node of the graph when idx is given.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "../../include/mcgra.h"
#include "common.h"
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int GS_TILE = 64;                         // positions per tile side = bits per word = lanes per wave
constexpr int GS_WAVES = AUC_THREADS / 64;          // waves per block
constexpr int GS_ROWS = GS_TILE / GS_WAVES;         // rows (pack) or columns (mirror) of a tile per wave
constexpr int GS_BATCH = 8;                         // neighbours of one word whose rows a wave of the count reads together
constexpr int GS_MAX_W =(int)((AUC_MAX_NIDX + 63) / 64);   // words per row at the capacity: 8 KiB of LDS
static_assert(GS_ROWS <= 64 && GS_TILE == 64, "a wave parks its words in its first GS_ROWS lanes");

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
  __shared__ uint64_t tR[GS_TILE], tG[GS_TILE];
  uint32_t A1, B;
  topk_unpack(blockIdx.x, A1, B);                                // A1 = A + 1 > B
  const int A = (int)A1 - 1, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = GS_TILE * (int)B + lane;                         // this lane's column
  const int64_t v = b < m ? (idx ? idx[b] : (int64_t)b) : 0;
  int f = 0;
  uint64_t myR = 0, myG = 0;                                     // lane i < GS_ROWS: the words of row wv * GS_ROWS + i
#pragma unroll 4
  for (int i = 0; i < GS_ROWS; ++i) {
    const int a = GS_TILE * A + wv * GS_ROWS + i;                // the same in every lane of the wave
    const bool valid = a < m && b < a;                           // so b < m
    bool r = false, g = false;
    if (valid) {
      const int64_t u = idx ? idx[a] : (int64_t)a;
      const float s = S[u * lds + v];
      if (!auc_finite(s)) f |= AUC_BAD_SCORE;
      r = auc_key(s) >= T;
      if (L) {
        const float l = L[u * ldl + v];
        g = auc_pos(l);
        if (!g && !auc_neg(l)) f |= AUC_BAD_LABEL;               // also NaN
      }
    }
    const uint64_t wR = __ballot(r), wG = __ballot(g);
    if (lane == i) { myR = wR; myG = wG; }
  }
  if (f) atomicOr(flags, f);
  if (lane < GS_ROWS) {
    const int r = wv * GS_ROWS + lane, a = GS_TILE * A + r;
    tR[r] = myR;
    tG[r] = myG;
    if (A != (int)B && a < m) {                                  // word (row a, word B); the diagonal tile stores below
      const size_t at = (size_t)a * W + B;
      MR[at] = myR;
      if (L) { MG[at] = myG; MC[at] = myR & myG; }
    }
  }
  __syncthreads();
  const uint64_t rowR = tR[lane], rowG = tG[lane];               // this lane's ROW of the tile
  myR = 0; myG = 0;
#pragma unroll 4
  for (int i = 0; i < GS_ROWS; ++i) {
    const int c = wv * GS_ROWS + i;                              // column c of the tile: bit r of the mirrored word = bit c of row r
    const uint64_t wR = __ballot((rowR >> c) & 1ull), wG = __ballot((rowG >> c) & 1ull);
    if (lane == i) { myR = wR; myG = wG; }
  }
  if (lane < GS_ROWS) {
    const int c = wv * GS_ROWS + lane, row = GS_TILE * (int)B + c;
    if (A == (int)B) { myR |= tR[c]; myG |= tG[c]; }             // columns below the diagonal | columns above it
    if (row < m) {                                               // word (row b, word A)
      const size_t at = (size_t)row * W + A;
      MR[at] = myR;
      if (L) { MG[at] = myG; MC[at] = myR & myG; }
    }
  }
}

// Block (v, g): d and t of position v in graph g (M + g * plane).  out row v = {d_R, t_R, d_G, t_G, d_C, t_C}; with one graph
// the block also writes the four -1.
__global__ __launch_bounds__(AUC_THREADS) void k_gs_count(int W, const uint64_t* __restrict__ M, size_t plane, int graphs,
                                                          int64_t* __restrict__ out) {
  __shared__ uint64_t row[GS_MAX_W];
  __shared__ uint64_t sh[GS_WAVES];
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
  for (int j = wv; j < W; j += GS_WAVES) {
    const uint64_t x = row[j];
    uint64_t bits = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32) |
                    (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);      // the same in every lane: a scalar loop
    // the set bits are neighbours u = 64 j + bit of v (u < m: the pad bits are 0).  A word of a long row (a hub, a dense graph)
    // holds many: GS_BATCH rows a step, their loads in flight together; what is left, one row a step
    while (__popcll(bits) >= GS_BATCH) {
      const uint64_t* pu[GS_BATCH];
#pragma unroll
      for (int q = 0; q < GS_BATCH; ++q) {
        pu[q] = Mg + (size_t)(GS_TILE * j + __ffsll((unsigned long long)bits) - 1) * W;
        bits &= bits - 1;
      }
      for (int k = lane; k < W; k += 64) {
        const uint64_t rv = row[k];
        uint64_t y[GS_BATCH];
#pragma unroll
        for (int q = 0; q < GS_BATCH; ++q) y[q] = pu[q][k];
#pragma unroll
        for (int q = 0; q < GS_BATCH; ++q) acc += (uint64_t)__popcll(y[q] & rv);
      }
    }
    while (bits) {
      const uint64_t* __restrict__ pu = Mg + (size_t)(GS_TILE * j + __ffsll((unsigned long long)bits) - 1) * W;
      bits &= bits - 1;
      for (int k = lane; k < W; k += 64) acc += (uint64_t)__popcll(pu[k] & row[k]);
    }
  }
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
  __shared__ uint64_t sh[GS_WAVES];
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
    (void)hipGetLastError();                                      // the refusal is reported here, not by the next launch check
    set_error("%s: hipMalloc of %d bit matrices of %d x %d words (%llu bytes) failed", who, graphs, m, W,
              (unsigned long long)(plane * graphs * sizeof(uint64_t)));
    return MCGRA_ENOMEM;
  }
  MCGRA_HIP(hipMemsetAsync(state, 0, sizeof(GsState), st));
  if (int rc = rank_check_idx(who, st, b, n, idx, m, &state->flags)) return rc;
  uint32_t tb;
  memcpy(&tb, &threshold, sizeof(tb));
  if (tb == 0x80000000u) tb = 0u;
  const uint32_t T = (tb & 0x80000000u) ? ~tb : (tb | 0x80000000u);     // auc_key of the threshold (+-inf included)
  const unsigned tiles = (unsigned)W * (unsigned)(W + 1) / 2;           // at most 1024 * 1025 / 2
  k_gs_pack<<<tiles, AUC_THREADS, 0, st>>>(m, W, scores, ld_scores, labels, ld_labels, idx, T, M, labels ? M + plane : nullptr,
                                           labels ? M + 2 * plane : nullptr, &state->flags);
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
