// What the ranking entries share (auc.hip, curves.hip, topk.hip, node_rank.hip, two_means.hip, delong.hip, node_jackknife.hip,
// graph_structure.hip, hop_auc.hip, class_auc.hip; dp_graph.hip takes topk.hip's selection through topk_mark).
// Device side, inlined into each file's kernels: the order-preserving key of a float32 score, the label predicates, the pair of
// a packed position, integer block sums, the walk over the selected lower triangle (tri_for_each), the bound of a key in
// ascending keys (rank_bound), a lane's slot behind a wave-shared cursor (wave_slot) and its rank among the flagged lanes of a
// block (block_rank).  Host side, defined once in rank_common.hip: the checks of the arguments and of idx, the table from
// flag bits to refusals, the tile rule, one scan, and the stable LSD radix sort of 32-bit keys (optionally with a 32-bit
// payload); their kernels are compiled there and nowhere else.  Here too: the scratch allocations of a call (AucBufs), the
// carver of one of them into arrays, and the sort's scratch.  Everything here is integer work, so no result depends on the
// order in which blocks run.
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "../../include/mcgra.h"
#include "common.h"

namespace mcgra {
constexpr int AUC_THREADS = 256;
constexpr int AUC_SORT_TILE = 1024;        // keys staged per step of a sort block (256 lanes x one 16-byte load)
constexpr int AUC_SORT_BLOCKS = 1024;      // at most this many tiles of keys per sort pass
constexpr size_t AUC_SORT_COUNTS = 256 * (size_t)AUC_SORT_BLOCKS;      // the (digit, tile) counts of one sort pass
constexpr int64_t AUC_MAX_NIDX = 65535;    // 2 P N <= 2 (n_idx^2 / 2)^2 < 2^63; a packed pair position fits 32 bits

// DL_BAD_SCORE_B: the second score matrix of a paired entry
enum { AUC_BAD_SCORE = 1, AUC_BAD_LABEL = 2, AUC_BAD_INDEX = 4, AUC_REPEAT = 8, AUC_BAD_FACTOR = 16, DL_BAD_SCORE_B = 32 };

// ---- host side (rank_common.hip)
struct AucBufs {
  std::vector<void*> p;
  ~AucBufs() { for (void* q : p) (void)hipFree(q); }
  template <typename T>
  T* get(size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();             // the caller reports the refusal, not the launch check of the next call
      return nullptr;
    }
    p.push_back(q);
    return (T*)q;
  }
};

// One allocation carved into arrays front to back; every array starts on 16 bytes (the sort loads four keys at a time).
// bytes<T>(count) is what take<T>(count) uses up.
struct Carver {
  uint8_t* at;
  size_t left;
  template <typename T>
  static constexpr size_t bytes(size_t count) { return (count * sizeof(T) + 15) / 16 * 16; }
  template <typename T>
  T* take(size_t count) {
    const size_t need = bytes<T>(count);
    assert(need <= left);
    T* q = (T*)at;
    at += need;
    left -= need;
    return q;
  }
};

// The sort's scratch: AUC_SORT_COUNTS entries each, carved from a caller's allocation or (b) an allocation of its own
// (cnt == NULL: hipMalloc failed).
struct SortScratch {
  uint32_t* cnt = nullptr;
  uint64_t* off = nullptr;
  SortScratch() = default;
  static constexpr size_t BYTES = Carver::bytes<uint32_t>(AUC_SORT_COUNTS) + Carver::bytes<uint64_t>(AUC_SORT_COUNTS);
  explicit SortScratch(Carver& c) : cnt(c.take<uint32_t>(AUC_SORT_COUNTS)), off(c.take<uint64_t>(AUC_SORT_COUNTS)) {}
  explicit SortScratch(AucBufs& b) : cnt(nullptr), off(nullptr) {
    if (uint8_t* q = b.get<uint8_t>(BYTES)) { Carver c{q, BYTES}; *this = SortScratch(c); }
  }
};

// The checks that need no device: n >= 1, every matrix [n x n] with ld >= n (NULL only where !required), at least min_idx
// selected nodes and at most cap.  idx == NULL: n_idx = n.
struct RankMat { const float* p; int ld; bool required; };
int rank_check_args(const char* who, int n, std::initializer_list<RankMat> mats, const int64_t* idx, int64_t& n_idx, int min_idx,
                    int64_t cap = AUC_MAX_NIDX);
// idx != NULL: every id in [0, n), and none twice unless allow_repeats (then *repeated says whether one is).  flags: a zeroed
// device word.  One allocation, one memset, one copy back, one sync.
int rank_check_idx(const char* who, hipStream_t st, AucBufs& b, int n, const int64_t* idx, int64_t rows, int* flags,
                   bool allow_repeats = false, bool* repeated = nullptr);
// the refusal of the AUC_BAD_* bits a pass over the selection left in flags (paired: DL_BAD_SCORE_B too); 0 when there is none
int rank_flag_error(const char* who, int flags, bool paired = false);
// contiguous tiles of `count` items: a multiple of `step` each, at most max_blocks of them
struct RankTiles { uint64_t tile; int nb; };
RankTiles rank_tiles(uint64_t count, int max_blocks, int step);
// off[i] = cnt[0] + ... + cnt[i - 1] over len entries (one block; the caller checks the launch)
void rank_scan(hipStream_t st, const uint32_t* cnt, int len, uint64_t* off);
// stable LSD radix sort of keys[0, count) (a multiple-of-4 aligned region), tmp the same size; result in keys.  pay != NULL:
// pay[i] travels with keys[i] (ptmp the same size; result in pay).  bits (a multiple of 8): every key is below 2^bits,
// bits / 8 passes; after an odd number of them the result is in tmp (and ptmp).
int auc_sort(hipStream_t st, uint32_t* keys, uint32_t* tmp, uint64_t count, const SortScratch& ss, uint32_t* pay = nullptr,
             uint32_t* ptmp = nullptr, int bits = 32);
// topk.hip: mark[p] = 1 where pair p (positions a > b of all n nodes, p = a (a - 1) / 2 + b) is one of the k best of
// mcgra_topk_metrics' ranking of scores' strict lower triangle (descending float32 value, ties by ascending p), else 0; mark:
// device, n (n - 1) / 2 bytes; 2 <= n <= AUC_MAX_NIDX and 1 <= k <= n (n - 1) / 2 are the caller's to hold.  The emit, the radix
// select and the take of the two entries, nothing of its own; a NaN or +-inf score: MCGRA_EINVAL.  Synchronises the stream.
int topk_mark(const char* who, hipStream_t stream, int n, const float* scores, int ld_scores, uint64_t k, uint8_t* mark);

// ---- both sides
// float32 (its bits) -> unsigned key with the same order; -0.0 and +0.0 are one value, +-inf are ordinary values.  Bit tests
// throughout, so that no floating-point mode (denormal flushing) can merge a subnormal with zero.
__host__ __device__ inline uint32_t auc_key_bits(uint32_t u) {
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the key of a threshold, for the kernels that compare auc_key(score) >= T
inline uint32_t auc_key_host(float s) {
  uint32_t u;
  memcpy(&u, &s, sizeof(u));
  return auc_key_bits(u);
}

// ---- device side
namespace {
__device__ __forceinline__ uint32_t auc_key(float s) { return auc_key_bits(__float_as_uint(s)); }
__device__ __forceinline__ bool auc_finite(float s) { return (__float_as_uint(s) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool auc_pos(float l) { return __float_as_uint(l) == 0x3f800000u; }
__device__ __forceinline__ bool auc_neg(float l) { return (__float_as_uint(l) & 0x7fffffffu) == 0u; }

// pair (a, b), a > b >= 0, of packed position p = a (a - 1) / 2 + b
__device__ __forceinline__ void topk_unpack(uint32_t p, uint32_t& a, uint32_t& b) {
  uint32_t x = (uint32_t)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
  while ((uint64_t)x * (x - 1) / 2 > p) --x;
  while ((uint64_t)x * (x + 1) / 2 <= p) ++x;
  a = x;
  b = p - (uint32_t)((uint64_t)x * (x - 1) / 2);
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the block (AUC_THREADS lanes), valid in thread 0
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t* sh) {
  v = wave_sum_u64(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < AUC_THREADS / 64; ++w) t += sh[w];
  return t;
}
// acc[q] += the block's sum of part[q] for each of the Q counters: one 64-bit atomic per non-zero counter and block
template <int Q>
__device__ __forceinline__ void block_add_u64(const uint64_t (&part)[Q], uint64_t* sh, unsigned long long* __restrict__ acc) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    __syncthreads();                                  // sh is reused
    const uint64_t tot = block_sum_u64(part[q], sh);
    if (threadIdx.x == 0 && tot) atomicAdd(&acc[q], (unsigned long long)tot);
  }
}

// The selected strict lower triangle: f(a, b, u, v) for every pair of positions b < a of the rows a = 1 + blockIdx.x,
// + gridDim.x, ... this block owns, u = idx[a], v = idx[b] (idx == NULL: the positions themselves); row_end(a) behind each row.
template <class F, class R>
__device__ __forceinline__ void tri_for_each(int rows, const int64_t* __restrict__ idx, F&& f, R&& row_end) {
  for (int a = 1 + blockIdx.x; a < rows; a += gridDim.x) {
    const int64_t u = idx ? idx[a] : a;
    for (int b = threadIdx.x; b < a; b += AUC_THREADS) f(a, b, u, idx ? idx[b] : (int64_t)b);
    row_end(a);
  }
}
template <class F>
__device__ __forceinline__ void tri_for_each(int rows, const int64_t* __restrict__ idx, F&& f) {
  tri_for_each(rows, idx, f, [](int) {});
}

// first index in [lo, hi) of the ascending keys B whose key is >= x (UPPER: > x); hi when there is none
template <bool UPPER, class Keys, class I>
__device__ __forceinline__ I rank_bound(const Keys& B, I lo, I hi, uint32_t x) {
  while (lo < hi) {
    const I mid = lo + ((hi - lo) >> 1);
    const uint32_t k = B[mid];
    if (UPPER ? k <= x : k < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// This lane's slot among the lanes of its wave that call with `pred`, behind the LDS counter *cursor: the first of them
// advances the cursor by their number, the others take their places in lane order.  Every active lane calls it; the value
// means something where pred holds.
__device__ __forceinline__ uint32_t wave_slot(bool pred, uint32_t* cursor) {
  const int lane = threadIdx.x & 63;
  const uint64_t m = __ballot(pred);
  if (m == 0) return 0;                                  // the same in every active lane
  const int leader = __ffsll((unsigned long long)m) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(cursor, (uint32_t)__popcll(m));
  return __shfl(base, leader, 64) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// One step of a block's ranking in index order: `before` = flagged lanes below this one in the block, `all` = flagged lanes
// of the block.  Every lane of the block calls it; w[par] holds the step's per-wave counts (par alternates, so one barrier
// a step is enough: a wave reaches the step after next only once every wave has read this one).
struct BlockRank { uint32_t before, all; };
__device__ __forceinline__ BlockRank block_rank(bool f, uint32_t (*w)[AUC_THREADS / 64], int par) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t m = __ballot(f);
  if (lane == 0) w[par][wv] = (uint32_t)__popcll(m);
  __syncthreads();
  BlockRank r{(uint32_t)__popcll(m & ((1ull << lane) - 1ull)), 0u};
#pragma unroll
  for (int q = 0; q < AUC_THREADS / 64; ++q) {
    if (q < wv) r.before += w[par][q];
    r.all += w[par][q];
  }
  return r;
}
}  // namespace
}  // namespace mcgra
