// The k-nearest-neighbour graph of a scored square matrix restricted to idx: every node keeps its own k best-scored partners,
// and the lists are symmetrised as the union and as the mutual graph (mcgra_knn_graph).
//
// Selection and candidates: those of mcgra_node_rank_metrics (node_rank.hip).  For position a of a repeat-free idx of m nodes
// (idx == NULL: all n nodes in order) the candidates are the m - 1 positions b != a with score scores[idx[a]][idx[b]]: row a of
// the gathered submatrix without its diagonal.  Scores compare through auc_key (float32 values, -0.0 == +0.0, subnormals
// distinct); the best-first ranking is key descending, ties by ascending position b.  L_k(a) is the first k positions of it.
//   D   the arc a -> b iff b is in L_k(a)          U   {a, b} iff a -> b or b -> a          Mu  {a, b} iff both
//   G   {a, b}, a > b, iff labels[idx[a]][idx[b]] == 1 (the strict lower triangle, as mcgra_graph_structure reads it)
//
// D, its transpose Dt and G are bit matrices (bit_graph.h: m rows of W = ceil(m / 64) words).  Passes:
//   rank_check_idx   idx only: range check, repeats (rank_common.hip)
//   k_knn_select     one workgroup a row.  The row's keys are gathered into LDS once (the diagonal slot holds 0, below every
//                    valid key; the argument predicate runs on what is read).  The row is SELECTED, not sorted: four 8-bit
//                    radix rounds over the LDS keys (a histogram of the keys that still share the prefix, a scan of its 256
//                    counts from the top) leave the k-th key T and r, how many of the keys equal to T belong to the list.
//                    One more walk in position order: key > T, or key == T and fewer than r equal keys before it (block_rank:
//                    ballots and per-wave counts, so the tie order is positional); __ballot of "chosen" IS the word of row a
//                    of D: one plain store per word.  Row-length classes 1024, 4096 and the capacity: LDS is 4 bytes per class element
//   k_knn_pack_g     given labels: bg_pack_tile with the bit "label is 1", and the label check
//   k_knn_transpose  Dt by 64 x 64 bit tiles: the 64 words of a tile go to LDS, every lane takes the word of its row and a
//                    ballot per column gives the transposed word (the mirror of bg_pack_tile); one writer per word
//   (the flag word is read back here; after a refusal nothing has been written to any output)
//   k_knn_count      one wave a node: U = D | Dt and Mu = D & Dt word by word; the seven columns are popcounts, and so is the
//                    number of U's edges {a, b} with b < a, the node's share of the edge list
//   k_knn_totals     one block: the seven column sums, the header
//   rank_scan        the running sum of the per-node edge counts: the edge list's order is packed position, by one scan
//   k_knn_edges      one wave a node: its edges in ascending b behind the node's offset, with idx, the score, the kind bits
//                    and the label bit
//   k_knn_lists      (lists asked for) one workgroup a row: the k set bits of row a of D become the composites
//                    key << 32 | ~b, re-read from the scores, and ONLY these k are sorted (bitonic, in LDS, descending)
// Integer arithmetic and key comparisons only; every output word has one writer (the histograms' LDS atomics add integers):
// the same bits on every call, whatever order the workgroups run in.
// Device scratch: 2 m W 8 bytes (D and Dt), m W 8 more with labels (96 MB at m = 16 384), 12 bytes per selected node, about
// 100 bytes, and 4 bytes per node of the graph when idx is given.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "../../include/mcgra.h"
#include "bit_graph.h"
#include "common.h"
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int KNN_WAVES = AUC_THREADS / 64;
constexpr int KNN_MAX_W = MCGRA_KNN_MAX_NIDX / 64;             // words per row at the capacity
static_assert(MCGRA_KNN_MAX_NIDX % 64 == 0 && KNN_MAX_W <= AUC_THREADS, "k_knn_lists: one lane per word of a row");
static_assert((MCGRA_KNN_MAX_K & (MCGRA_KNN_MAX_K - 1)) == 0, "the sort of the k winners runs on a power of two");

struct KnnState {
  unsigned long long tot[7];               // the sums of the seven columns
  int flags;
};

// inclusive sum scan over the block's lanes; sh: KNN_WAVES entries, free for reuse behind the caller's next barrier
__device__ __forceinline__ uint32_t knn_block_scan(uint32_t v, uint32_t* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  if (lane == 63) sh[w] = v;
  __syncthreads();
  for (int q = 0; q < w; ++q) v += sh[q];
  return v;
}

// Row a = blockIdx.x of D.  CAP: the row-length class, m <= CAP.
template <int CAP>
__global__ __launch_bounds__(AUC_THREADS) void k_knn_select(int m, int W, int k, const float* __restrict__ S, int64_t lds,
                                                            const int64_t* __restrict__ idx, uint64_t* __restrict__ D,
                                                            int* __restrict__ flags) {
  __shared__ uint32_t key[CAP];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wsum[KNN_WAVES], pick[3];
  __shared__ uint32_t weq[2][KNN_WAVES];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int a = blockIdx.x;
  // ---- gather: key[b] of every position; 0 at the diagonal, which is not read
  const float* __restrict__ srow = S + (idx ? idx[a] : (int64_t)a) * lds;
  int f = 0;
#pragma unroll 4
  for (int b = t; b < m; b += AUC_THREADS) {
    uint32_t kk = 0u;
    if (b != a) {
      const float s = srow[idx ? idx[b] : (int64_t)b];
      if (!auc_finite(s)) f |= AUC_BAD_SCORE;
      kk = auc_key(s);
    }
    key[b] = kk;
  }
  if (f) atomicOr(flags, f);
  // ---- the k-th key from the top: T = prefix, and r of the keys equal to T belong to the list (n_eq of them exist).  A valid
  // key is at least 0x00800000, so the diagonal's 0 is the one smallest entry and k <= m - 1 never reaches it
  uint32_t prefix = 0u, r = (uint32_t)k, n_eq = 0u;
  const int steps = (m + AUC_THREADS - 1) / AUC_THREADS;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[t] = 0u;
    __syncthreads();                                            // (the first round: also publishes key[])
    for (int q = 0; q < steps; ++q) {
      const int b = q * AUC_THREADS + t;
      const uint32_t kk = b < m ? key[b] : 0u;
      const bool act = b < m && (shift == 24 || (kk >> (shift + 8)) == (prefix >> (shift + 8)));
      const uint32_t d = (kk >> shift) & 255u;
      const uint64_t am = __ballot(act);
      if (am) {                                                 // the same in every lane of the wave
        const int first = __ffsll((unsigned long long)am) - 1;
        const uint32_t d0 = __shfl(d, first, 64);
        if (__ballot(act && d == d0) == am) {                   // one digit in the whole wave (scores of one binade): one add
          if (lane == first) atomicAdd(&hist[d0], (uint32_t)__popcll(am));
        } else if (act) {
          atomicAdd(&hist[d], 1u);
        }
      }
    }
    __syncthreads();
    const uint32_t c = hist[255 - t];                           // lane t: digit 255 - t, so the scan runs from the top digit
    const uint32_t incl = knn_block_scan(c, wsum);
    if (incl >= r && incl - c < r) { pick[0] = 255u - (uint32_t)t; pick[1] = r - (incl - c); pick[2] = c; }   // one lane
    __syncthreads();
    prefix |= pick[0] << shift;
    r = pick[1];
    n_eq = pick[2];
  }
  // ---- row a of D, 256 positions a step: a wave's ballot is one word.  The ties are ranked only when not all of them are in
  const uint32_t T = prefix;
  const bool some_ties = r < n_eq;
  const int words = (W + KNN_WAVES - 1) / KNN_WAVES;
  uint32_t run_eq = 0u;
  int par = 0;
  for (int q = 0; q < words; ++q, par ^= 1) {
    const int b = q * AUC_THREADS + t;
    const uint32_t kk = b < m ? key[b] : 0u;
    const bool eq = kk == T;
    bool chosen = kk >= T;
    if (some_ties) {
      const BlockRank re = block_rank(eq, weq, par);
      chosen = kk > T || (eq && run_eq + re.before < r);
      run_eq += re.all;
    }
    const uint64_t word = __ballot(chosen);
    const int j = q * KNN_WAVES + wv;
    if (lane == 0 && j < W) D[(size_t)a * W + j] = word;
  }
}

// Tile (A, B), B <= A, of block p = A (A + 1) / 2 + B: G's words, and the label check
__global__ __launch_bounds__(AUC_THREADS) void k_knn_pack_g(int m, int W, const float* __restrict__ L, int64_t ldl,
                                                            const int64_t* __restrict__ idx, uint64_t* __restrict__ G,
                                                            int* __restrict__ flags) {
  __shared__ uint64_t tile[1][BG_TILE];
  int f = 0;
  bg_pack_tile<1>(m, W, idx, tile, [&](int64_t u, int64_t v, bool (&bit)[1]) {
    const float l = L[u * ldl + v];
    bit[0] = auc_pos(l);
    if (!bit[0] && !auc_neg(l)) f |= AUC_BAD_LABEL;               // also NaN
  }, [&](size_t at, const uint64_t (&w)[1]) { G[at] = w[0]; });
  if (f) atomicOr(flags, f);
}

// Block (B, A): the words (row 64 A + r, word B), r = 0 .. 63, of D become the words (row 64 B + c, word A) of Dt
__global__ __launch_bounds__(AUC_THREADS) void k_knn_transpose(int m, int W, const uint64_t* __restrict__ D,
                                                               uint64_t* __restrict__ Dt) {
  __shared__ uint64_t tile[BG_TILE];
  const int B = blockIdx.x, A = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x < BG_TILE) {
    const int r = BG_TILE * A + (int)threadIdx.x;
    tile[threadIdx.x] = r < m ? D[(size_t)r * W + B] : 0ull;
  }
  __syncthreads();
  const uint64_t row = tile[lane];                               // this lane's ROW of the tile
  uint64_t mine = 0;
#pragma unroll 4
  for (int i = 0; i < BG_ROWS; ++i) {
    const int c = wv * BG_ROWS + i;                              // bit r of the transposed word = bit c of row r
    const uint64_t w = __ballot((row >> c) & 1ull);
    if (lane == i) mine = w;
  }
  if (lane < BG_ROWS) {
    const int r = BG_TILE * B + wv * BG_ROWS + lane;
    if (r < m) Dt[(size_t)r * W + A] = mine;
  }
}

__device__ __forceinline__ uint32_t knn_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the bits of word j of row a that lie below the diagonal: positions b < a
__device__ __forceinline__ uint64_t knn_below(int a, int j) {
  const int full = a >> 6;
  return j < full ? ~0ull : j == full ? (1ull << (a & 63)) - 1ull : 0ull;
}

// Wave (blockIdx.x, wv): node a.  out row a = {in, d_U, d_M, d_G, h_D, h_U, h_M}; cnt[a] = U's edges {a, b} with b < a
// (cnt[m] = 0: the scan's entry m is then E_U)
__global__ __launch_bounds__(AUC_THREADS) void k_knn_count(int m, int W, const uint64_t* __restrict__ D,
                                                           const uint64_t* __restrict__ Dt, const uint64_t* __restrict__ G,
                                                           int64_t* __restrict__ out, uint32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63, a = blockIdx.x * KNN_WAVES + (threadIdx.x >> 6);
  if (a >= m) return;                                            // a whole wave; the kernel has no barrier
  uint32_t c[8] = {};
  for (int j = lane; j < W; j += 64) {
    const uint64_t d = D[(size_t)a * W + j], t = Dt[(size_t)a * W + j], g = G ? G[(size_t)a * W + j] : 0ull;
    const uint64_t u = d | t, mu = d & t;
    c[0] += (uint32_t)__popcll(t);
    c[1] += (uint32_t)__popcll(u);
    c[2] += (uint32_t)__popcll(mu);
    c[3] += (uint32_t)__popcll(g);
    c[4] += (uint32_t)__popcll(d & g);
    c[5] += (uint32_t)__popcll(u & g);
    c[6] += (uint32_t)__popcll(mu & g);
    c[7] += (uint32_t)__popcll(u & knn_below(a, j));
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) c[q] = knn_wave_sum(c[q]);
  if (lane == 0) {
    int64_t* o = out + (size_t)a * 7;
#pragma unroll
    for (int q = 0; q < 7; ++q) o[q] = (G || q < 3) ? (int64_t)c[q] : -1;
    cnt[a] = c[7];
    if (a == 0) cnt[m] = 0u;
  }
}

// st->tot[q] = the sum of column q (one block)
__global__ __launch_bounds__(AUC_THREADS) void k_knn_totals(int m, int cols, const int64_t* __restrict__ out,
                                                            KnnState* __restrict__ st) {
  __shared__ uint64_t sh[KNN_WAVES];
  for (int q = 0; q < cols; ++q) {
    uint64_t s = 0;
    for (int v = threadIdx.x; v < m; v += AUC_THREADS) s += (uint64_t)out[(size_t)v * 7 + q];
    const uint64_t tot = block_sum_u64(s, sh);
    __syncthreads();
    if (threadIdx.x == 0) st->tot[q] = tot;
  }
}

// Wave (blockIdx.x, wv): node a >= 1.  Its edges {a, b}, b < a, of U in ascending b at off[a], off[a] + 1, ...
__global__ __launch_bounds__(AUC_THREADS) void k_knn_edges(int m, int W, const uint64_t* __restrict__ D,
                                                           const uint64_t* __restrict__ Dt, const uint64_t* __restrict__ G,
                                                           const uint64_t* __restrict__ off, const float* __restrict__ S,
                                                           int64_t lds, const int64_t* __restrict__ idx,
                                                           int64_t* __restrict__ pairs, float* __restrict__ pair_scores,
                                                           uint8_t* __restrict__ kind, uint8_t* __restrict__ hits) {
  const int lane = threadIdx.x & 63, a = 1 + blockIdx.x * KNN_WAVES + (threadIdx.x >> 6);
  if (a >= m) return;                                            // a whole wave; the kernel has no barrier
  const int64_t u = idx ? idx[a] : (int64_t)a;
  uint64_t run = off[a];
  for (int base = 0; base <= (a >> 6); base += 64) {             // 64 words a step, one a lane
    const int j = base + lane;
    uint64_t d = 0, t = 0, g = 0;
    if (j <= (a >> 6)) {
      const uint64_t low = knn_below(a, j);
      d = D[(size_t)a * W + j] & low;
      t = Dt[(size_t)a * W + j] & low;
      if (hits) g = G[(size_t)a * W + j];
    }
    uint64_t x = d | t;
    const uint32_t c = (uint32_t)__popcll(x);
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    uint64_t at = run + (incl - c);
    while (x) {
      const int bit = __ffsll((unsigned long long)x) - 1;
      x &= x - 1;
      const int b = BG_TILE * j + bit;
      const int64_t v = idx ? idx[b] : (int64_t)b;
      pairs[2 * at] = u;
      pairs[2 * at + 1] = v;
      if (pair_scores) pair_scores[at] = S[u * lds + v];
      if (kind) kind[at] = (uint8_t)(((d >> bit) & 1ull) | (((t >> bit) & 1ull) << 1));
      if (hits) hits[at] = (uint8_t)((g >> bit) & 1ull);
      ++at;
    }
    run += __shfl(incl, 63, 64);
  }
}

// Row a = blockIdx.x of lists: L_k(a) in ranking order.  KP: the smallest power of two >= k.
__global__ __launch_bounds__(AUC_THREADS) void k_knn_lists(int W, int k, int KP, const uint64_t* __restrict__ D,
                                                           const float* __restrict__ S, int64_t lds,
                                                           const int64_t* __restrict__ idx, int32_t* __restrict__ lists) {
  __shared__ uint64_t win[MCGRA_KNN_MAX_K];
  __shared__ uint32_t wsum[KNN_WAVES];
  const int t = threadIdx.x, a = blockIdx.x;
  const float* __restrict__ srow = S + (idx ? idx[a] : (int64_t)a) * lds;
  uint64_t x = t < W ? D[(size_t)a * W + t] : 0ull;              // lane t: word t of the row (W <= AUC_THREADS)
  const uint32_t c = (uint32_t)__popcll(x);
  uint32_t at = knn_block_scan(c, wsum) - c;                     // the k winners in position order; the sort does the rest
  while (x) {
    const int b = BG_TILE * t + __ffsll((unsigned long long)x) - 1;
    x &= x - 1;
    if (at < (uint32_t)k) win[at] = (uint64_t)auc_key(srow[idx ? idx[b] : (int64_t)b]) << 32 | (uint32_t)~(uint32_t)b;
    ++at;                                                        // (a row of D holds exactly k bits)
  }
  for (int i = k + t; i < KP; i += AUC_THREADS) win[i] = 0ull;   // below every winner
  __syncthreads();
  for (int size = 2; size <= KP; size <<= 1) {                   // bitonic, descending: key descending, then b ascending
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int p = t; p < KP / 2; p += AUC_THREADS) {
        const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;
        const uint64_t y = win[lo], z = win[hi];
        if ((y < z) == ((lo & size) == 0)) { win[lo] = z; win[hi] = y; }
      }
      __syncthreads();
    }
  }
  for (int i = t; i < k; i += AUC_THREADS) lists[(size_t)a * k + i] = (int32_t)~(uint32_t)win[i];
}

template <int CAP>
void knn_select_launch(hipStream_t st, int m, int W, int k, const float* S, int lds, const int64_t* idx, uint64_t* D,
                       int* flags) {
  k_knn_select<CAP><<<m, AUC_THREADS, 0, st>>>(m, W, k, S, lds, idx, D, flags);
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_knn_graph(void* stream, int n, const float* scores, int ld_scores, const float* labels, int ld_labels,
                               const int64_t* idx, int64_t n_idx, int64_t k_nn, int64_t* header, int64_t* out, int32_t* lists,
                               int64_t cap, int64_t* pairs, float* pair_scores, uint8_t* kind, uint8_t* hits) {
  const char* who = "knn_graph";
  if (!header || !out) { set_error("%s: bad argument (header or out NULL)", who); return MCGRA_EINVAL; }
  if (cap < 0 || (cap > 0 && !pairs)) {
    set_error("%s: bad argument (cap = %lld%s)", who, (long long)cap, cap > 0 ? " with pairs NULL" : "");
    return MCGRA_EINVAL;
  }
  if (hits && !labels) { set_error("%s: bad argument (hits needs labels)", who); return MCGRA_EINVAL; }
  if (int rc = rank_check_args(who, n, {{scores, ld_scores, true}, {labels, ld_labels, false}}, idx, n_idx, 2,
                               MCGRA_KNN_MAX_NIDX))
    return rc;
  if (k_nn < 1 || k_nn > n_idx - 1) {
    set_error("%s: bad argument (k = %lld; 1 <= k <= %lld, one less than the selected nodes)", who, (long long)k_nn,
              (long long)(n_idx - 1));
    return MCGRA_EINVAL;
  }
  if (k_nn > MCGRA_KNN_MAX_K) {
    set_error("%s: k = %lld; more than %d neighbours a node are not supported", who, (long long)k_nn, MCGRA_KNN_MAX_K);
    return MCGRA_ENOSUP;
  }
  hipStream_t st = (hipStream_t)stream;
  const int m = (int)n_idx, W = (m + 63) / 64, k = (int)k_nn;
  const size_t plane = (size_t)m * W;
  AucBufs b;
  KnnState* state = b.get<KnnState>(1);
  uint64_t* M = b.get<uint64_t>(plane * (labels ? 3 : 2));
  uint32_t* cnt = b.get<uint32_t>((size_t)m + 1);
  uint64_t* off = b.get<uint64_t>((size_t)m + 1);
  if (!state || !M || !cnt || !off) {
    set_error("%s: hipMalloc of %d bit matrices of %d x %d words (%llu bytes) failed", who, labels ? 3 : 2, m, W,
              (unsigned long long)(plane * (labels ? 3 : 2) * sizeof(uint64_t)));
    return MCGRA_ENOMEM;
  }
  uint64_t *D = M, *Dt = M + plane, *G = labels ? M + 2 * plane : nullptr;
  MCGRA_HIP(hipMemsetAsync(state, 0, sizeof(KnnState), st));
  if (int rc = rank_check_idx(who, st, b, n, idx, m, &state->flags)) return rc;
  if (m <= 1024) knn_select_launch<1024>(st, m, W, k, scores, ld_scores, idx, D, &state->flags);
  else if (m <= 4096) knn_select_launch<4096>(st, m, W, k, scores, ld_scores, idx, D, &state->flags);
  else knn_select_launch<MCGRA_KNN_MAX_NIDX>(st, m, W, k, scores, ld_scores, idx, D, &state->flags);
  MCGRA_KERNEL_CHECK();
  if (labels) k_knn_pack_g<<<bg_tiles(W), AUC_THREADS, 0, st>>>(m, W, labels, ld_labels, idx, G, &state->flags);
  k_knn_transpose<<<dim3((unsigned)W, (unsigned)W), AUC_THREADS, 0, st>>>(m, W, D, Dt);
  MCGRA_KERNEL_CHECK();
  KnnState h{};
  MCGRA_HIP(hipMemcpyAsync(&h, state, sizeof(KnnState), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (int rc = rank_flag_error(who, h.flags)) return rc;
  // every check has passed: from here on the outputs are written
  const int nodes = (m + KNN_WAVES - 1) / KNN_WAVES;
  k_knn_count<<<nodes, AUC_THREADS, 0, st>>>(m, W, D, Dt, G, out, cnt);
  k_knn_totals<<<1, AUC_THREADS, 0, st>>>(m, labels ? 7 : 3, out, state);
  rank_scan(st, cnt, m + 1, off);
  if (lists) {
    int KP = 1;
    while (KP < k) KP <<= 1;
    k_knn_lists<<<m, AUC_THREADS, 0, st>>>(W, k, KP, D, scores, ld_scores, idx, lists);
  }
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipMemcpyAsync(&h, state, sizeof(KnnState), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  const int64_t E_U = (int64_t)(h.tot[1] / 2);
  int64_t r[8] = {(int64_t)m * (m - 1) / 2, k, E_U, (int64_t)(h.tot[2] / 2), -1, -1, -1, -1};
  if (labels) {
    r[4] = (int64_t)(h.tot[3] / 2);
    r[5] = (int64_t)h.tot[4];
    r[6] = (int64_t)(h.tot[5] / 2);
    r[7] = (int64_t)(h.tot[6] / 2);
  }
  memcpy(header, r, sizeof(r));
  if (!pairs) return 0;                                                 // no edge list was asked for
  if (E_U > cap) {
    set_error("%s: the union graph has %lld edges, cap is %lld (header holds what is needed)", who, (long long)E_U,
              (long long)cap);
    return MCGRA_ENOMEM;
  }
  k_knn_edges<<<(m - 1 + KNN_WAVES - 1) / KNN_WAVES, AUC_THREADS, 0, st>>>(m, W, D, Dt, G, off, scores, ld_scores, idx, pairs,
                                                                         pair_scores, kind, hits);
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipStreamSynchronize(st));                                  // the scratch is freed on return
  return 0;
}
