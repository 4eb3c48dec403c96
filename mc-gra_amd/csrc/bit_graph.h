// The bit matrix of a graph on m selected positions, which graph_structure.hip and hop_auc.hip share: its layout, the pack of
// the selected strict lower triangle into it, and the walk over the neighbours of a row.  Device side only, inlined into each
// file's kernels.
//
// A graph is a row-major BIT matrix: m rows of W = ceil(m / 64) 64-bit words, bit (a, b) at word b / 64 of row a, bit b % 64;
// symmetric, zero diagonal, zero pad bits at positions >= m.  One AND + popcount then tests 64 pairs.
#pragma once
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int BG_TILE = 64;                          // positions per tile side = bits per word = lanes per wave
constexpr int BG_WAVES = AUC_THREADS / 64;           // waves per block
constexpr int BG_ROWS = BG_TILE / BG_WAVES;          // rows (pack) or columns (mirror) of a tile per wave
constexpr int BG_BATCH = 8;                          // neighbours of one word whose rows are read together
constexpr int BG_MAX_W = (int)((AUC_MAX_NIDX + 63) / 64);      // words per row at the capacity: 8 KiB of LDS
static_assert(BG_ROWS <= 64 && BG_TILE == 64, "a wave parks its words in its first BG_ROWS lanes");

// blocks of a pack: the tiles (A, B), B <= A, of W x W words (at most 1024 * 1025 / 2)
inline unsigned bg_tiles(int W) { return (unsigned)W * (unsigned)(W + 1) / 2; }

// The pack of NG graphs at once, one block (AUC_THREADS lanes) a tile: the one read of the selected strict lower triangle, in
// 64 x 64 tiles of positions (A, B), B <= A, block p = A (A + 1) / 2 + B; a wave BG_ROWS of the tile's rows, lane = column.
// pair(u, v, bit) sets bit[k] = whether graph k has the edge of the nodes u = idx[a], v = idx[b]; it is called for a < m,
// b < a alone.  __ballot of a bit IS the word (row a, word B).  The tile's 64 words per graph are parked in LDS (tile: NG
// arrays of BG_TILE words); every lane reads the word of ITS row and a second ballot per column gives the mirrored word (row b,
// word A).  The diagonal tile ORs both halves before its one store.  store(at, w): the words w[k] belong at word `at` of graph
// k's matrix; every word of a matrix has exactly one writer: plain vector stores, no atomics, no memset.
template <int NG, class Pair, class Store>
__device__ __forceinline__ void bg_pack_tile(int m, int W, const int64_t* __restrict__ idx, uint64_t (*tile)[BG_TILE], Pair&& pair,
                                             Store&& store) {
  uint32_t A1, B;
  topk_unpack(blockIdx.x, A1, B);                                // A1 = A + 1 > B
  const int A = (int)A1 - 1, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = BG_TILE * (int)B + lane;                         // this lane's column
  const int64_t v = b < m ? (idx ? idx[b] : (int64_t)b) : 0;
  uint64_t mine[NG] = {};                                        // lane i < BG_ROWS: the words of row wv * BG_ROWS + i
#pragma unroll 4
  for (int i = 0; i < BG_ROWS; ++i) {
    const int a = BG_TILE * A + wv * BG_ROWS + i;                // the same in every lane of the wave
    bool bit[NG] = {};
    if (a < m && b < a) pair(idx ? idx[a] : (int64_t)a, v, bit); // so b < m
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      const uint64_t w = __ballot(bit[k]);
      if (lane == i) mine[k] = w;
    }
  }
  if (lane < BG_ROWS) {
    const int r = wv * BG_ROWS + lane, a = BG_TILE * A + r;
#pragma unroll
    for (int k = 0; k < NG; ++k) tile[k][r] = mine[k];
    if (A != (int)B && a < m) store((size_t)a * W + B, mine);    // word (row a, word B); the diagonal tile stores below
  }
  __syncthreads();
  uint64_t row[NG];                                              // this lane's ROW of the tile
#pragma unroll
  for (int k = 0; k < NG; ++k) { row[k] = tile[k][lane]; mine[k] = 0; }
#pragma unroll 4
  for (int i = 0; i < BG_ROWS; ++i) {
    const int c = wv * BG_ROWS + i;                              // column c of the tile: bit r of the mirrored word = bit c of row r
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      const uint64_t w = __ballot((row[k] >> c) & 1ull);
      if (lane == i) mine[k] = w;
    }
  }
  if (lane < BG_ROWS) {
    const int c = wv * BG_ROWS + lane, r = BG_TILE * (int)B + c;
    if (A == (int)B) {                                           // columns below the diagonal | columns above it
#pragma unroll
      for (int k = 0; k < NG; ++k) mine[k] |= tile[k][c];
    }
    if (r < m) store((size_t)r * W + A, mine);                   // word (row b, word A)
  }
}

// The neighbours of a position whose row holds the word x at word j (x may come from LDS: its two halves go through
// readfirstlane, so the walk is a scalar loop, the same in every lane of the wave).  The set bits are the neighbours
// u = 64 j + bit (u < m: the pad bits are 0).  A word of a long row (a hub, a dense graph) holds many: many(pu) gets BG_BATCH
// of their rows in M (W words each) a step while the word holds as many, so that their loads are in flight together; one(pu)
// gets what is left, one row a step.
template <class Many, class One>
__device__ __forceinline__ void bg_for_each_neighbour(uint64_t x, int j, const uint64_t* __restrict__ M, int W, Many&& many,
                                                      One&& one) {
  uint64_t bits = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32) |
                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
  while (__popcll(bits) >= BG_BATCH) {
    const uint64_t* pu[BG_BATCH];
#pragma unroll
    for (int q = 0; q < BG_BATCH; ++q) {
      pu[q] = M + (size_t)(BG_TILE * j + __ffsll((unsigned long long)bits) - 1) * W;
      bits &= bits - 1;
    }
    many(pu);
  }
  while (bits) {
    const uint64_t* __restrict__ pu = M + (size_t)(BG_TILE * j + __ffsll((unsigned long long)bits) - 1) * W;
    bits &= bits - 1;
    one(pu);
  }
}
}  // namespace
}  // namespace mcgra
