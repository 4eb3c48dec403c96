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
// A graph is mcgra_graph_structure's row-major BIT matrix: m rows of W = ceil(m / 64) 64-bit words, bit (a, b) at word b / 64
// of row a, bit b % 64; zero pad bits at positions >= m.  reach_h has bit (a, b) iff a walk of 1 .. h edges joins a and b, so
// for a != b iff dist(a, b) <= h (its diagonal is set from h = 2 on: there and back; no pass reads it).
// Passes:
//   rank_check_idx  idx only: range check, repeats (rank_common.hip)
//   k_dl_classify   (delong_common.h) one read of the selected strict lower triangle: the argument checks (NaN / inf score,
//                   label other than 0 / 1) and per-block counts of the positives
//   k_ha_pack       a read of the labels in 64 x 64 tiles of positions, graph_structure.hip's tile for one graph: a ballot IS
//                   the word (row a, word B), the tile's words parked in LDS and a second ballot per column give the mirrored
//                   word (row b, word A).  Every word of reach_1 = G has one writer
//   k_ha_expand     H - 1 times, from level h's matrix into level h + 1's: one block per row a.  reach_h+1[a] = reach_h[a] |
//                   OR over the neighbours u of a in G of reach_h[u].  The neighbours are the set bits of G's row a (in LDS,
//                   walked as a scalar loop); lane t owns the words t, t + 256, .. of the row and ORs the same words of every
//                   neighbour's row in (coalesced), HA_BATCH neighbours of one word at a time while it holds as many (a hub's
//                   row is one block's work).  One writer per word, no atomics, never in place
//   k_dl_emit       (delong_common.h) the positives' keys to their slots; auc_sort sorts them in place
//   k_ha_stream     ONE pass over the selected strict lower triangle that reads all H levels: the class of a candidate is
//                   H - #{levels whose bit (a, b) is set} (the levels are nested), 0 for an edge; a non-edge finds lb and ub
//                   among the sorted positives (delong_common.h's dl_find through samples in LDS), b = 2 P - lb - ub.  Per
//                   class pairs, T and above accumulate in registers, then block_sum_u64, then one 64-bit integer atomic per
//                   class, quantity and block
// Integer arithmetic only: the same bits on every call and under any permutation of idx.  `out` is written by the host once
// everything has come back.
// Device scratch: H bit matrices of 8 m W bytes (all levels are kept for the one stream pass; H = 3: 38 MB at m = 10 000, 1.6 GB
// at m = 65 535), 8 bytes per positive (its key and the sort's second buffer), about 3 MB for the sort's counts, 8 bytes per
// block of the row passes, and 4 bytes per node of the graph when idx is given.
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
constexpr int HA_TILE = 64;                          // positions per tile side = bits per word = lanes per wave
constexpr int HA_WAVES = AUC_THREADS / 64;           // waves per block
constexpr int HA_ROWS = HA_TILE / HA_WAVES;          // rows (pack) or columns (mirror) of a tile per wave
constexpr int HA_BATCH = 8;                          // neighbours of one word whose rows a block of the expansion reads together
constexpr int HA_MAX_W = (int)((AUC_MAX_NIDX + 63) / 64);      // words per row at the capacity: 8 KiB of LDS
constexpr int HA_LANE_WORDS = HA_MAX_W / AUC_THREADS;          // words of a row a lane of the expansion owns, at most
constexpr int HA_ROW_BLOCKS = 1024;                  // blocks of the passes over the selected rows (grid-stride)
constexpr int HA_CLASSES = MCGRA_HOP_MAX + 1;        // distances 1 .. MCGRA_HOP_MAX and beyond
static_assert(HA_ROWS <= 64 && HA_TILE == 64, "a wave parks its words in its first HA_ROWS lanes");
static_assert(HA_LANE_WORDS * AUC_THREADS == HA_MAX_W, "the lanes of one block cover a row of the capacity");

enum { HA_PAIRS = 0, HA_T, HA_ABOVE, HA_COLS };

struct HaHead {
  unsigned long long acc[HA_CLASSES][HA_COLS];
  int flags, pad;
};

// Tile (A, B), B <= A, of block p = A (A + 1) / 2 + B: G's words (row a, word B) and (row b, word A).  The labels were checked.
__global__ __launch_bounds__(AUC_THREADS) void k_ha_pack(int m, int W, const float* __restrict__ L, int64_t ldl,
                                                         const int64_t* __restrict__ idx, uint64_t* __restrict__ MG) {
  __shared__ uint64_t tG[HA_TILE];
  uint32_t A1, B;
  topk_unpack(blockIdx.x, A1, B);                                // A1 = A + 1 > B
  const int A = (int)A1 - 1, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = HA_TILE * (int)B + lane;                         // this lane's column
  const int64_t v = b < m ? (idx ? idx[b] : (int64_t)b) : 0;
  uint64_t mine = 0;                                             // lane i < HA_ROWS: the word of row wv * HA_ROWS + i
#pragma unroll 4
  for (int i = 0; i < HA_ROWS; ++i) {
    const int a = HA_TILE * A + wv * HA_ROWS + i;                // the same in every lane of the wave
    bool g = false;
    if (a < m && b < a) {                                        // so b < m
      const int64_t u = idx ? idx[a] : (int64_t)a;
      g = auc_pos(L[u * ldl + v]);
    }
    const uint64_t w = __ballot(g);
    if (lane == i) mine = w;
  }
  if (lane < HA_ROWS) {
    const int r = wv * HA_ROWS + lane, a = HA_TILE * A + r;
    tG[r] = mine;
    if (A != (int)B && a < m) MG[(size_t)a * W + B] = mine;      // the diagonal tile stores below
  }
  __syncthreads();
  const uint64_t row = tG[lane];                                 // this lane's ROW of the tile
  mine = 0;
#pragma unroll 4
  for (int i = 0; i < HA_ROWS; ++i) {
    const int c = wv * HA_ROWS + i;                              // column c of the tile: bit r of the mirrored word = bit c of row r
    const uint64_t w = __ballot((row >> c) & 1ull);
    if (lane == i) mine = w;
  }
  if (lane < HA_ROWS) {
    const int c = wv * HA_ROWS + lane, r = HA_TILE * (int)B + c;
    if (A == (int)B) mine |= tG[c];                              // columns below the diagonal | columns above it
    if (r < m) MG[(size_t)r * W + A] = mine;
  }
}

// Block v: out row v = in row v | the rows of `in` of v's neighbours in G.
__global__ __launch_bounds__(AUC_THREADS) void k_ha_expand(int W, const uint64_t* __restrict__ G, const uint64_t* __restrict__ in,
                                                           uint64_t* __restrict__ out) {
  __shared__ uint64_t row[HA_MAX_W];
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
  for (int j = 0; j < W; ++j) {
    const uint64_t x = row[j];
    uint64_t bits = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32) |
                    (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);      // the same in every lane: a scalar loop
    // the set bits are the neighbours u = 64 j + bit of v (u < m: the pad bits are 0)
    while (__popcll(bits) >= HA_BATCH) {
      const uint64_t* pu[HA_BATCH];
#pragma unroll
      for (int q = 0; q < HA_BATCH; ++q) {
        pu[q] = in + (size_t)(HA_TILE * j + __ffsll((unsigned long long)bits) - 1) * W;
        bits &= bits - 1;
      }
#pragma unroll
      for (int q = 0; q < HA_LANE_WORDS; ++q) {
        const int k = threadIdx.x + q * AUC_THREADS;
        if (k < W) {
          uint64_t y[HA_BATCH];
#pragma unroll
          for (int s = 0; s < HA_BATCH; ++s) y[s] = pu[s][k];
#pragma unroll
          for (int s = 0; s < HA_BATCH; ++s) acc[q] |= y[s];
        }
      }
    }
    while (bits) {
      const uint64_t* __restrict__ pu = in + (size_t)(HA_TILE * j + __ffsll((unsigned long long)bits) - 1) * W;
      bits &= bits - 1;
#pragma unroll
      for (int q = 0; q < HA_LANE_WORDS; ++q) {
        const int k = threadIdx.x + q * AUC_THREADS;
        if (k < W) acc[q] |= pu[k];
      }
    }
  }
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
  uint32_t stride = 1, ns = 0;
  if (np) {
    stride = (np + DL_STAGE - 1) / DL_STAGE;
    ns = (np + stride - 1) / stride;
    for (uint32_t q = threadIdx.x; q < ns; q += AUC_THREADS) smp[q] = sorted[(uint64_t)q * stride];
  }
  __syncthreads();
  uint32_t cnt[HA_CLASSES] = {}, abv[HA_CLASSES] = {};           // a lane sees fewer than 2^32 candidates
  uint64_t sum[HA_CLASSES] = {};
  tri_for_each(rows, idx, [&](int a, int b, int64_t u, int64_t v) {
    const uint32_t x = auc_key(S[u * lds + v]);
    const size_t at = (size_t)a * W + (b >> 6);
    int cls = H;                                                 // the levels are nested: H - #{levels that hold the pair}
    for (int h = 0; h < H; ++h) cls -= (int)((M[h * plane + at] >> (b & 63)) & 1ull);
    uint64_t bq = 0;
    if (cls > 0 && np) {
      const uint32_t lb = dl_find<false>(sorted, np, smp, ns, stride, x);
      const uint32_t ub = (lb < np && sorted[lb] == x) ? dl_find<true>(sorted, np, smp, ns, stride, x) : lb;
      bq = 2ull * np - lb - ub;                                  // <= 2 np < 2^32
    }
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
#pragma unroll
      for (int q = 0; q < HA_COLS; ++q) {
        __syncthreads();
        const uint64_t tot = block_sum_u64(part[q], sh);
        if (threadIdx.x == 0 && tot) atomicAdd(&acc[c * HA_COLS + q], (unsigned long long)tot);
      }
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
  const int g = std::min(m - 1, HA_ROW_BLOCKS);
  AucBufs b;
  uint8_t* head = b.get<uint8_t>(sizeof(HaHead) + sizeof(uint64_t) * (size_t)g);
  uint64_t* M = b.get<uint64_t>(plane * H);
  if (!head || !M) {
    (void)hipGetLastError();                                      // the refusal is reported here, not by the next launch check
    set_error("%s: hipMalloc of %d bit matrices of %d x %d words (%llu bytes) failed", who, H, m, W,
              (unsigned long long)(plane * H * sizeof(uint64_t)));
    return MCGRA_ENOMEM;
  }
  HaHead* hd = (HaHead*)head;
  uint64_t* counts = (uint64_t*)(head + sizeof(HaHead));
  static_assert(sizeof(HaHead) % 8 == 0, "counts is 8-byte aligned");
  MCGRA_HIP(hipMemsetAsync(hd, 0, sizeof(HaHead), st));
  if (int rc = rank_check_idx(who, st, b, n, idx, m, &hd->flags)) return rc;
  k_dl_classify<false><<<g, AUC_THREADS, 0, st>>>(m, scores, ld_scores, nullptr, 0, labels, ld_labels, idx, counts, nullptr,
                                                  &hd->flags);
  MCGRA_KERNEL_CHECK();
  std::vector<uint64_t> h;
  uint64_t P = 0, N = 0;
  if (int rc = dl_counted(who, st, counts, &hd->flags, g, false, m, h, P, N)) return rc;
  const unsigned tiles = (unsigned)W * (unsigned)(W + 1) / 2;           // at most 1024 * 1025 / 2
  k_ha_pack<<<tiles, AUC_THREADS, 0, st>>>(m, W, labels, ld_labels, idx, M);
  for (int lv = 1; lv < H; ++lv) k_ha_expand<<<m, AUC_THREADS, 0, st>>>(W, M, M + (lv - 1) * plane, M + lv * plane);
  MCGRA_KERNEL_CHECK();
  uint32_t* sorted = nullptr;
  if (P) {
    // one allocation for what scales with P: the sort's counts, the keys, the sort's second buffer.  P4 = P rounded up to 4
    // keys: every array starts on 16 bytes
    const size_t P4 = (P + 3) / 4 * 4, sort_cnt = 256 * (size_t)AUC_SORT_BLOCKS;
    uint8_t* pool = b.get<uint8_t>((sizeof(uint64_t) + sizeof(uint32_t)) * sort_cnt + 2 * sizeof(uint32_t) * P4);
    if (!pool) {
      (void)hipGetLastError();
      set_error("%s: hipMalloc of the scratch of %llu positives failed", who, (unsigned long long)P);
      return MCGRA_ENOMEM;
    }
    uint64_t* off = (uint64_t*)pool;
    uint32_t* cnt = (uint32_t*)(off + sort_cnt);
    sorted = cnt + sort_cnt;
    uint32_t* tmp = sorted + P4;
    MCGRA_HIP(hipMemcpyAsync(counts, h.data(), sizeof(uint64_t) * h.size(), hipMemcpyHostToDevice, st));
    k_dl_emit<false><<<g, AUC_THREADS, 0, st>>>(m, scores, ld_scores, nullptr, 0, labels, ld_labels, idx, counts, sorted, nullptr);
    MCGRA_KERNEL_CHECK();
    if (int rc = auc_sort(st, sorted, tmp, P, cnt, off)) return rc;
  }
  uint32_t tb;
  memcpy(&tb, &threshold, sizeof(tb));
  if (tb == 0x80000000u) tb = 0u;
  const uint32_t T = (tb & 0x80000000u) ? ~tb : (tb | 0x80000000u);     // auc_key of the threshold (+-inf included)
  k_ha_stream<<<g, AUC_THREADS, 0, st>>>(m, W, H, scores, ld_scores, idx, M, plane, sorted, (uint32_t)P, T, &hd->acc[0][0]);
  MCGRA_KERNEL_CHECK();
  unsigned long long ha[HA_CLASSES][HA_COLS];
  MCGRA_HIP(hipMemcpyAsync(ha, hd->acc, sizeof(ha), hipMemcpyDeviceToHost, st));
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
