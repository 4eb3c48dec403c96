// The recovered graph: the k best-scored unordered node pairs of a scored square matrix restricted to idx, as counts
// (mcgra_topk_metrics: TP among the k best, P among all candidates) and as an edge list in ranking order (mcgra_top_pairs).
// Inside the library also as a byte per pair in packed order (topk_mark, for dp_graph.hip's LapGraph).
//
// Candidates: the m = n_idx (n_idx - 1) / 2 pairs of positions a > b of idx (idx == NULL: all n nodes in order); pair (a, b)
// is nodes u = idx[a], v = idx[b], its score scores[u][v], its label labels[u][v] (the strict lower triangle of the gathered
// submatrix: for an asymmetric matrix that entry, not [v][u], is read), its packed position p = a (a - 1) / 2 + b (the order
// of torch.tril_indices(offset=-1) and of adj_changes).  The AUC and AP entries of auc.hip range over all ordered entries,
// diagonal included; these range over unordered off-diagonal pairs.
// Ranking: score descending as float32 values (-0.0 == +0.0, subnormals and negatives ordinary values), ties by ascending p:
// np.argsort(-s, kind="stable")[:k] over the scores in packed order.
//
// Passes:
//   rank_check_idx     idx only: range check, repeats (rank_common.hip)
//   k_topk_emit        the one read of the selected lower triangle: argument checks, P (64-bit integer atomics), each
//                      pair's order-preserving key to keys[p] and, for the metrics, its label to lab[p]
//   k_topk_hist/_pick  MSB-first radix select, 4 passes of 8 bits: a 256-bin histogram (LDS, merged with integer atomics) of
//                      the keys that match the prefix found so far, then one block walks the bins from 255 down.  Result:
//                      the threshold key T, g = #keys above T, r = k - g >= 1 keys equal to T to take.  No sort of the m keys
//   k_topk_count       per block of a contiguous packed range: #keys above T, #keys equal to T; rank_scan scans both
//   k_topk_take        every block ranks the threshold ties of its range in index order (block_rank; the scan gives the
//                      ties before the block) and takes those of rank < r: TP is counted (metrics), or
//                      the chosen (key, p) records are compacted in packed order (edge list); the pair of tie rank r - 1 is
//                      the k-th of the ranking and its score is the threshold reported
//   auc_sort           edge list: a stable LSD radix sort of the k records by descending key with p as payload; they enter
//                      in ascending p, so ties leave in ascending p
//   k_topk_write       each record's pair (u, v), and its score and label read back from the matrices (copied bits)
// All of it is integers and copied float32 bits; per-block counts are over fixed contiguous ranges and merged by a scan or by
// integer atomics, so no result depends on the order in which blocks run and every call returns the same bits.
// Device scratch: 4 bytes per candidate (the keys), + 1 byte per candidate (mcgra_topk_metrics: the labels), + 16 bytes per
// returned pair (mcgra_top_pairs: the records and the sort's second buffer), + about 3 MB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "../../include/mcgra.h"
#include "common.h"
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int TOPK_ROW_BLOCKS = 1024;      // blocks of the pass over the matrix (grid-stride over selected rows)
constexpr int TOPK_BLOCKS = 1024;          // at most this many contiguous packed ranges (and blocks) per pass over the keys
constexpr int TOPK_HIST_STEP = 4 * AUC_THREADS;   // keys per step of a histogram block (one 16-byte load per lane)

struct TopkState {
  unsigned long long hist[256];            // the current pass's bins; k_topk_pick clears them
  unsigned long long P;                    // candidates with label 1
  unsigned long long tp;                   // of the k best
  unsigned long long remaining;            // keys still to take among those that match the prefix
  uint32_t prefix;                         // the threshold key's digits found so far
  uint32_t thr_bits;                       // the k-th pair's score
  int flags;
};

// keys[p] = key of pair p, lab[p] = its label (lab != NULL); st->P += labels that are 1; st->flags |= argument errors.
__global__ __launch_bounds__(AUC_THREADS) void k_topk_emit(int rows, const float* __restrict__ S, int64_t lds,
                                                           const float* __restrict__ L, int64_t ldl,
                                                           const int64_t* __restrict__ idx, uint32_t* __restrict__ keys,
                                                           uint8_t* __restrict__ lab, TopkState* __restrict__ st) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  uint64_t pos = 0;
  int f = 0;
  tri_for_each(rows, idx, [&](int a, int b, int64_t u, int64_t v) {
    const uint64_t at = (uint64_t)a * (a - 1) / 2 + b;
    const float s = S[u * lds + v];
    if (!auc_finite(s)) f |= AUC_BAD_SCORE;
    keys[at] = auc_key(s);
    if (L) {
      const float l = L[u * ldl + v];
      const bool p = auc_pos(l);
      if (p) ++pos;
      else if (!auc_neg(l)) f |= AUC_BAD_LABEL;   // also NaN
      if (lab) lab[at] = p ? 1 : 0;
    }
  });
  if (f) atomicOr(&st->flags, f);
  const uint64_t tot = block_sum_u64(pos, sh);
  if (threadIdx.x == 0 && tot) atomicAdd(&st->P, (unsigned long long)tot);
}

// st->hist[d] += keys whose digits above `shift + 8` are the prefix's and whose digit (key >> shift) & 255 is d
__global__ __launch_bounds__(AUC_THREADS) void k_topk_hist(const uint32_t* __restrict__ keys, uint64_t count, int shift,
                                                           TopkState* __restrict__ st) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t prefix = st->prefix;
  const int hi = shift + 8;                                    // 32 on the first pass: every key matches
  auto add = [&](uint32_t k) {
    if ((uint32_t)((uint64_t)(k ^ prefix) >> hi) == 0u) atomicAdd(&h[(k >> shift) & 255u], 1u);
  };
  // a block adds at most ceil(2^31 / (TOPK_BLOCKS * TOPK_HIST_STEP)) * TOPK_HIST_STEP < 2^32 keys: the bins do not wrap
  for (uint64_t e = ((uint64_t)blockIdx.x * AUC_THREADS + threadIdx.x) * 4; e < count; e += (uint64_t)gridDim.x * TOPK_HIST_STEP) {
    if (e + 4 <= count) {
      const uint4 k = *(const uint4*)(keys + e);                // keys is a hipMalloc'ed base: 16-byte aligned
      add(k.x); add(k.y); add(k.z); add(k.w);
    } else {
      for (uint64_t q = e; q < count; ++q) add(keys[q]);
    }
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// one block: the digit d at which the bins, walked from 255 down, reach st->remaining; prefix |= d << shift, remaining -= the
// keys in the bins above d; the bins are cleared for the next pass
__global__ __launch_bounds__(256) void k_topk_pick(int shift, TopkState* __restrict__ st) {
  __shared__ unsigned long long h[256];
  h[threadIdx.x] = st->hist[threadIdx.x];
  __syncthreads();
  st->hist[threadIdx.x] = 0;
  if (threadIdx.x != 0) return;
  const unsigned long long want = st->remaining;
  unsigned long long above = 0;
  int d = 255;
  while (d > 0 && above + h[d] < want) { above += h[d]; --d; }
  st->prefix |= (uint32_t)d << shift;
  st->remaining = want - above;
}

// block b's contiguous range [b tile, (b + 1) tile): cnt[b] = #keys above T, cnt[nb + b] = #keys equal to T
__global__ __launch_bounds__(AUC_THREADS) void k_topk_count(const uint32_t* __restrict__ keys, uint64_t count, uint64_t tile,
                                                            uint32_t T, int nb, uint32_t* __restrict__ cnt) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  const uint64_t beg = blockIdx.x * tile, end = min(count, beg + tile);
  uint64_t gt = 0, eq = 0;
  for (uint64_t e = beg + threadIdx.x; e < end; e += AUC_THREADS) {
    const uint32_t k = keys[e];
    gt += k > T;
    eq += k == T;
  }
  const uint64_t g = block_sum_u64(gt, sh);
  __syncthreads();
  const uint64_t q = block_sum_u64(eq, sh);
  if (threadIdx.x == 0) { cnt[blockIdx.x] = (uint32_t)g; cnt[nb + blockIdx.x] = (uint32_t)q; }
}

// The k best of block b's range, in index order, 256 keys a step: a key above T, or a key equal to T whose rank among ALL
// keys equal to T (off[nb + b] - g before this block, then the earlier steps, the earlier waves, the lower lanes) is below
// r.  EMIT: the chosen (~key, p) go to rk / rp at their rank among the chosen, off[b] + min(ties before the block, r) before
// this block (packed order).  MARK: mark[p] = 1 for a chosen pair, 0 for every other one (the selection as a mask in packed
// order, topk_mark).  Otherwise st->tp += the chosen with label 1.  The tie of rank r - 1 is the k-th pair: its score goes to
// st->thr_bits.
enum TakeMode { TAKE_COUNT, TAKE_EMIT, TAKE_MARK };
template <TakeMode MODE>
__global__ __launch_bounds__(AUC_THREADS) void k_topk_take(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ lab,
                                                           uint64_t count, uint64_t tile, uint32_t T, uint64_t g, uint64_t r,
                                                           int nb, const uint64_t* __restrict__ off,
                                                           const float* __restrict__ S, int64_t lds,
                                                           const int64_t* __restrict__ idx, uint32_t* __restrict__ rk,
                                                           uint32_t* __restrict__ rp, uint8_t* __restrict__ mark,
                                                           TopkState* __restrict__ st) {
  constexpr bool EMIT = MODE == TAKE_EMIT;
  __shared__ uint32_t weq[2][AUC_THREADS / 64], wch[2][AUC_THREADS / 64];
  __shared__ uint64_t sh[AUC_THREADS / 64];
  const int t = threadIdx.x;
  const uint64_t beg = blockIdx.x * tile, end = min(count, beg + tile);
  uint64_t run_eq = off[nb + blockIdx.x] - g;                  // ties before this block
  uint64_t run_ch = off[blockIdx.x] + min(run_eq, r);          // chosen before this block
  uint64_t tp = 0;
  int par = 0;
  for (uint64_t base = beg; base < end; base += AUC_THREADS, par ^= 1) {
    const uint64_t e = base + t;
    const bool valid = e < end;
    const uint32_t k = valid ? keys[e] : 0u;
    const bool eq = valid && k == T;
    const BlockRank re = block_rank(eq, weq, par);
    const uint64_t rank = run_eq + re.before;
    const bool chosen = valid && (k > T || (eq && rank < r));
    if (eq && rank == r - 1) {
      uint32_t a, b;
      topk_unpack((uint32_t)e, a, b);
      const int64_t u = idx ? idx[a] : a, v = idx ? idx[b] : b;
      st->thr_bits = __float_as_uint(S[u * lds + v]);
    }
    run_eq += re.all;
    if (EMIT) {
      const BlockRank rc = block_rank(chosen, wch, par);
      if (chosen) { rk[run_ch + rc.before] = ~k; rp[run_ch + rc.before] = (uint32_t)e; }
      run_ch += rc.all;
    } else if (MODE == TAKE_MARK) {
      if (valid) mark[e] = chosen ? 1 : 0;
    } else if (chosen && lab[e]) {
      ++tp;
    }
  }
  if (MODE == TAKE_COUNT) {
    const uint64_t tot = block_sum_u64(tp, sh);
    if (t == 0 && tot) atomicAdd(&st->tp, (unsigned long long)tot);
  }
}

// row i of the answer: the pair of record i, its score and its label read back from the matrices
__global__ __launch_bounds__(AUC_THREADS) void k_topk_write(uint64_t k, const uint32_t* __restrict__ rp,
                                                            const float* __restrict__ S, int64_t lds,
                                                            const float* __restrict__ L, int64_t ldl,
                                                            const int64_t* __restrict__ idx, int64_t* __restrict__ pairs,
                                                            float* __restrict__ pair_scores, uint8_t* __restrict__ hits) {
  for (uint64_t i = (uint64_t)blockIdx.x * AUC_THREADS + threadIdx.x; i < k; i += (uint64_t)gridDim.x * AUC_THREADS) {
    uint32_t a, b;
    topk_unpack(rp[i], a, b);
    const int64_t u = idx ? idx[a] : a, v = idx ? idx[b] : b;
    pairs[2 * i] = u;
    pairs[2 * i + 1] = v;
    if (pair_scores) pair_scores[i] = S[u * lds + v];
    if (hits) hits[i] = auc_pos(L[u * ldl + v]) ? 1 : 0;
  }
}

// What the two entries share: the argument pass, the keys and the select.
struct TopkRun {
  const char* who;
  hipStream_t st;
  AucBufs b;
  TopkState* state = nullptr;
  TopkState h{};                          // the host's copy, after emit() and after select()
  uint32_t* keys = nullptr;
  uint8_t* lab = nullptr;
  SortScratch ss{b};                      // also the counts of select() and their scan
  uint64_t m = 0, tile = 0;
  int nb = 0;

  int fetch() {
    MCGRA_HIP(hipMemcpyAsync(&h, state, sizeof(TopkState), hipMemcpyDeviceToHost, st));
    MCGRA_HIP(hipStreamSynchronize(st));
    return 0;
  }
  // idx check, then the one read of the selected lower triangle; on return h.P is P
  int emit(int n, const float* S, int lds, const float* L, int ldl, const int64_t* idx, int rows, bool want_lab) {
    m = (uint64_t)rows * (rows - 1) / 2;
    state = b.get<TopkState>(1);
    keys = b.get<uint32_t>(m);
    lab = want_lab ? b.get<uint8_t>(m) : nullptr;
    if (!state || !keys || (want_lab && !lab) || !ss.cnt) {
      set_error("%s: hipMalloc of the scratch of %llu pairs failed", who, (unsigned long long)m);
      return MCGRA_ENOMEM;
    }
    MCGRA_HIP(hipMemsetAsync(state, 0, sizeof(TopkState), st));
    if (int rc = rank_check_idx(who, st, b, n, idx, rows, &state->flags)) return rc;
    k_topk_emit<<<std::min(rows - 1, TOPK_ROW_BLOCKS), AUC_THREADS, 0, st>>>(rows, S, lds, L, ldl, idx, keys, lab, state);
    MCGRA_KERNEL_CHECK();
    if (int rc = fetch()) return rc;
    if (int rc = rank_flag_error(who, h.flags)) return rc;
    const RankTiles ti = rank_tiles(m, TOPK_BLOCKS, AUC_THREADS);
    tile = ti.tile;
    nb = ti.nb;
    return 0;
  }
  // the threshold of the k best, 1 <= k <= m: h.prefix = T, h.remaining = r; then the per-range counts and their scan
  int select(uint64_t k) {
    MCGRA_HIP(hipMemcpyAsync(&state->remaining, &k, sizeof(k), hipMemcpyHostToDevice, st));
    const int g = (int)std::min<uint64_t>(TOPK_BLOCKS, (m + TOPK_HIST_STEP - 1) / TOPK_HIST_STEP);
    for (int shift = 24; shift >= 0; shift -= 8) {
      k_topk_hist<<<g, AUC_THREADS, 0, st>>>(keys, m, shift, state);
      k_topk_pick<<<1, 256, 0, st>>>(shift, state);
    }
    MCGRA_KERNEL_CHECK();
    if (int rc = fetch()) return rc;      // (also: &k was read)
    k_topk_count<<<nb, AUC_THREADS, 0, st>>>(keys, m, tile, h.prefix, nb, ss.cnt);
    rank_scan(st, ss.cnt, 2 * nb, ss.off);
    MCGRA_KERNEL_CHECK();
    return 0;
  }
};

int topk_check(const char* who, int n, const float* scores, int ld_scores, const float* labels, int ld_labels,
               const int64_t* idx, int64_t& n_idx, int64_t k, int64_t k_min) {
  if (k < k_min) { set_error("%s: bad argument (k = %lld)", who, (long long)k); return MCGRA_EINVAL; }
  if (int rc = rank_check_args(who, n, {{scores, ld_scores, true}, {labels, ld_labels, false}}, idx, n_idx, 2)) return rc;
  const int64_t m = n_idx * (n_idx - 1) / 2;
  if (k > m) { set_error("%s: k = %lld of %lld pairs", who, (long long)k, (long long)m); return MCGRA_EINVAL; }
  return 0;
}
}  // namespace

// rank_common.h: the k best pairs of all n nodes as a mask in packed order, for a caller inside the library (dp_graph.hip).
int topk_mark(const char* who, hipStream_t stream, int n, const float* scores, int ld_scores, uint64_t k, uint8_t* mark) {
  TopkRun run{who, stream};
  if (int rc = run.emit(n, scores, ld_scores, nullptr, 0, nullptr, n, false)) return rc;
  if (int rc = run.select(k)) return rc;
  const uint64_t r = run.h.remaining, g = k - r;
  k_topk_take<TAKE_MARK><<<run.nb, AUC_THREADS, 0, stream>>>(run.keys, nullptr, run.m, run.tile, run.h.prefix, g, r, run.nb,
                                                            run.ss.off, scores, ld_scores, nullptr, nullptr, nullptr, mark,
                                                            run.state);
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipStreamSynchronize(stream));      // the scratch is freed on return
  return 0;
}
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_topk_metrics(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                                  const int64_t* idx, int64_t n_idx, int64_t k, int64_t* counts, float* threshold) {
  if (!labels || !counts) { set_error("topk_metrics: bad argument"); return MCGRA_EINVAL; }
  if (int rc = topk_check("topk_metrics", n, scores, ld_scores, labels, ld_labels, idx, n_idx, k, 0)) return rc;
  TopkRun run{"topk_metrics", (hipStream_t)stream};
  hipStream_t st = run.st;
  if (int rc = run.emit(n, scores, ld_scores, labels, ld_labels, idx, (int)n_idx, true)) return rc;
  const uint64_t P = run.h.P;
  const uint64_t kk = k ? (uint64_t)k : P;                  // k == 0: the true graph's own edge count in the selection
  counts[0] = (int64_t)kk; counts[1] = (int64_t)P; counts[2] = 0; counts[3] = (int64_t)run.m;
  if (kk == 0) return 0;
  if (int rc = run.select(kk)) return rc;
  const uint64_t r = run.h.remaining, g = kk - r;
  k_topk_take<TAKE_COUNT><<<run.nb, AUC_THREADS, 0, st>>>(run.keys, run.lab, run.m, run.tile, run.h.prefix, g, r, run.nb,
                                                          run.ss.off, scores, ld_scores, idx, nullptr, nullptr, nullptr, run.state);
  MCGRA_KERNEL_CHECK();
  if (int rc = run.fetch()) return rc;
  counts[2] = (int64_t)run.h.tp;
  if (threshold) memcpy(threshold, &run.h.thr_bits, sizeof(float));
  return 0;
}

extern "C" int mcgra_top_pairs(void* stream, int n, const float* scores, int ld_scores, const int64_t* idx, int64_t n_idx,
                               int64_t k, const float* labels, int ld_labels, int64_t* pairs, float* pair_scores,
                               uint8_t* hits) {
  if (!pairs || (hits && !labels)) { set_error("top_pairs: bad argument"); return MCGRA_EINVAL; }
  if (int rc = topk_check("top_pairs", n, scores, ld_scores, labels, ld_labels, idx, n_idx, k, 1)) return rc;
  TopkRun run{"top_pairs", (hipStream_t)stream};
  hipStream_t st = run.st;
  if (int rc = run.emit(n, scores, ld_scores, labels, ld_labels, idx, (int)n_idx, false)) return rc;
  const uint64_t kk = (uint64_t)k;
  uint32_t* rk = run.b.get<uint32_t>(kk);
  uint32_t* rp = run.b.get<uint32_t>(kk);
  uint32_t* tk = run.b.get<uint32_t>(kk);
  uint32_t* tp = run.b.get<uint32_t>(kk);
  if (!rk || !rp || !tk || !tp) { set_error("top_pairs: hipMalloc of %llu records failed", (unsigned long long)kk); return MCGRA_ENOMEM; }
  if (int rc = run.select(kk)) return rc;
  const uint64_t r = run.h.remaining, g = kk - r;
  k_topk_take<TAKE_EMIT><<<run.nb, AUC_THREADS, 0, st>>>(run.keys, nullptr, run.m, run.tile, run.h.prefix, g, r, run.nb,
                                                         run.ss.off, scores, ld_scores, idx, rk, rp, nullptr, run.state);
  MCGRA_KERNEL_CHECK();
  if (int rc = auc_sort(st, rk, tk, kk, run.ss, rp, tp)) return rc;
  const int gw = (int)std::min<uint64_t>(2048, (kk + AUC_THREADS - 1) / AUC_THREADS);
  k_topk_write<<<gw, AUC_THREADS, 0, st>>>(kk, rp, scores, ld_scores, labels, ld_labels, idx, pairs, pair_scores, hits);
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipStreamSynchronize(st));      // the scratch is freed on return
  return 0;
}
