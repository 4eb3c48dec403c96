// The recovered graph without the truth: a 2-means split of the selected scores into "no edge" and "edge"
// (mcgra_two_means_split; the reference's PGDAttack.kmeans, baseline.py:88-109, made exact and repeatable), and the edge list
// of every candidate at or above a threshold in packed order (mcgra_threshold_pairs; with the reference's filter() cut, the
// 2-means threshold or best_threshold of the curves).
//
// Candidates, selection and packed position are those of topk.hip.  q = rint(s 2^28), round half to even, is an unsigned
// 32-bit integer for 0 <= s < 16, and Lloyd's iteration runs on the q in integers (include/mcgra.h has the definition,
// DESIGN.md 3f the argument that neither cluster is ever empty).
//
// Passes of mcgra_two_means_split:
//   rank_check_idx  idx only: range check, repeats (rank_common.hip)
//   k_tm_emit     the one read of the selected lower triangle for the rounds: argument checks, q[p] and, given labels, lab[p]
//                 (the layout of k_topk_emit), P, the sum of all q, min q and max q (integer atomics)
//   k_tm_start    one lane: t_0 = floor((min + max) / 2) + 1
//   k_tm_round    one streaming pass over q (16-byte loads): count and sum of the q below t, per lane in 64 bits, reduced over
//                 the wave and the block, merged with 64-bit integer atomics; the high cluster is the rest of m and of the sum
//   k_tm_update   one lane: c0, c1 (two 64-bit divisions), t_{k+1}; records the partition just counted; sets `done` when the
//                 threshold repeats or max_iter is reached; clears the two accumulators
//                 The host launches TM_BATCH rounds at a time, at most max_iter in all, and reads the state back after each
//                 batch; a round launched after `done` returns at once.  No kernel waits for another one's progress.
//   k_tm_final    a second read of the selected scores: the smallest score of the high cluster, the largest of the low one
//                 (min / max of the order-preserving key), and TP from lab[p]
// Passes of mcgra_threshold_pairs: k_tp_count (per contiguous packed range: argument checks, the pairs at or above the
// threshold, the hits among them), rank_scan, k_tp_write (every block ranks its qualifying pairs in packed order, block_rank,
// behind the scan's offset).  No atomics decide an order.
// Everything is integers and copied float32 bits, merged by integer atomics or a scan: no result depends on the order in which
// blocks run, and every call returns the same bits.
// Device scratch: mcgra_two_means_split 4 bytes per candidate (q) + 1 byte per candidate (the labels, when given) + a few KB;
// mcgra_threshold_pairs about 16 KB (+ 4 bytes per node of the graph when idx is given).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "../../include/mcgra.h"
#include "common.h"
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int TM_ROW_BLOCKS = 1024;        // blocks of the passes over the matrix (grid-stride over selected rows)
constexpr int TM_BLOCKS = 1024;            // at most this many blocks per streaming pass over q
constexpr int TM_STEP = 4 * AUC_THREADS;   // q per step of a streaming block (one 16-byte load per lane)
constexpr int TM_BATCH = 4;                // rounds launched between two reads of the state
constexpr int TP_BLOCKS = 1024;            // at most this many contiguous packed ranges (and blocks) of mcgra_threshold_pairs
constexpr int TM_BAD_RANGE = 64;           // a flag beside the shared ones: a finite selected score below 0 or >= 16

struct TmState {
  unsigned long long P, tp;                // candidates with label 1; those of the high cluster
  unsigned long long total;                // sum of all q
  unsigned long long n_low, sum_low;       // the current round's accumulators; k_tm_update clears them
  unsigned long long t;                    // the threshold the next round counts with
  unsigned long long rep_t, rep_n_high, rep_c0, rep_c1;   // the partition last counted
  uint32_t inv_min, max;                   // ~min q (so that zero-filled memory is the identity of atomicMax) and max q
  uint32_t inv_hi_min, lo_max;             // ~(smallest key of the high cluster), largest key of the low cluster
  int iterations, converged, done, flags;
};

struct TpState {
  unsigned long long hits;
  int flags;
};

// q = rint(s 2^28), half to even, of the bits u of a float32 0 <= s < 16 (u < 0x41800000), in integers: s = man 2^(E - 150)
// with E = max(exponent field, 1), so s 2^28 = man 2^(E - 122), E <= 130, man < 2^24
__device__ __forceinline__ uint32_t tm_quantise(uint32_t u) {
  const int ex = (int)(u >> 23);
  const uint32_t man = (u & 0x007fffffu) | (ex ? 0x00800000u : 0u);
  const int sh = (ex ? ex : 1) - 122;
  if (sh >= 0) return man << sh;
  const int r = -sh;
  if (r > 24) return 0u;                   // man 2^-r < 1 / 2
  const uint32_t q = man >> r, rem = man & ((1u << r) - 1u), half = 1u << (r - 1);
  return q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u);
}

// the bits of a score that is neither NaN nor infinite: in range (0 <= s < 16, -0.0 as 0)?
__device__ __forceinline__ bool tm_in_range(uint32_t u) { return u == 0x80000000u || u < 0x41800000u; }

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
// max over the block, valid in thread 0
__device__ __forceinline__ uint32_t block_max_u32(uint32_t v, uint32_t* sh) {
  v = wave_max_u32(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < AUC_THREADS / 64; ++w) t = max(t, sh[w]);
  return t;
}

// the score of a key (auc_key inverted; the key of -0.0 and +0.0 gives +0.0)
inline uint32_t tm_key_bits(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// q[p] = the quantised score of pair p, lab[p] = its label (L != NULL); st: P, total, min, max, flags.
__global__ __launch_bounds__(AUC_THREADS) void k_tm_emit(int rows, const float* __restrict__ S, int64_t lds,
                                                         const float* __restrict__ L, int64_t ldl,
                                                         const int64_t* __restrict__ idx, uint32_t* __restrict__ q,
                                                         uint8_t* __restrict__ lab, TmState* __restrict__ st) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  __shared__ uint32_t shm[AUC_THREADS / 64];
  uint64_t pos = 0, sum = 0;
  uint32_t inv_mn = 0, mx = 0;
  int f = 0;
  tri_for_each(rows, idx, [&](int a, int b, int64_t u, int64_t v) {
    const uint64_t at = (uint64_t)a * (a - 1) / 2 + b;
    const float s = S[u * lds + v];
    const uint32_t bits = __float_as_uint(s);
    uint32_t x = 0;
    if (!auc_finite(s)) f |= AUC_BAD_SCORE;
    else if (!tm_in_range(bits)) f |= TM_BAD_RANGE;
    else x = tm_quantise(bits & 0x7fffffffu);
    q[at] = x;
    sum += x;
    mx = max(mx, x);
    inv_mn = max(inv_mn, ~x);
    if (L) {
      const float l = L[u * ldl + v];
      const bool p = auc_pos(l);
      if (p) ++pos;
      else if (!auc_neg(l)) f |= AUC_BAD_LABEL;   // also NaN
      lab[at] = p ? 1 : 0;
    }
  });
  if (f) atomicOr(&st->flags, f);
  const uint64_t tot = block_sum_u64(pos, sh);
  __syncthreads();
  const uint64_t tsum = block_sum_u64(sum, sh);
  const uint32_t bmx = block_max_u32(mx, shm);
  __syncthreads();
  const uint32_t bmn = block_max_u32(inv_mn, shm);
  if (threadIdx.x == 0) {
    if (tot) atomicAdd(&st->P, (unsigned long long)tot);
    if (tsum) atomicAdd(&st->total, (unsigned long long)tsum);
    atomicMax(&st->max, bmx);
    atomicMax(&st->inv_min, bmn);
  }
}

__global__ void k_tm_start(TmState* __restrict__ st) {
  st->t = ((unsigned long long)(~st->inv_min) + st->max) / 2 + 1;
}

// st->n_low += #q below st->t, st->sum_low += their sum
__global__ __launch_bounds__(AUC_THREADS) void k_tm_round(const uint32_t* __restrict__ q, uint64_t count,
                                                          TmState* __restrict__ st) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  if (st->done) return;                                          // (the same in every lane of the grid)
  const uint32_t t = (uint32_t)st->t;                            // lo < t <= hi < 2^32
  uint64_t n = 0, sum = 0;
  auto add = [&](uint32_t x) { if (x < t) { ++n; sum += x; } };
  for (uint64_t e = ((uint64_t)blockIdx.x * AUC_THREADS + threadIdx.x) * 4; e < count; e += (uint64_t)gridDim.x * TM_STEP) {
    if (e + 4 <= count) {
      const uint4 k = *(const uint4*)(q + e);                     // q is a hipMalloc'ed base: 16-byte aligned
      add(k.x); add(k.y); add(k.z); add(k.w);
    } else {
      for (uint64_t i = e; i < count; ++i) add(q[i]);
    }
  }
  const uint64_t bn = block_sum_u64(n, sh);
  __syncthreads();
  const uint64_t bs = block_sum_u64(sum, sh);
  if (threadIdx.x == 0 && bn) {
    atomicAdd(&st->n_low, (unsigned long long)bn);
    if (bs) atomicAdd(&st->sum_low, (unsigned long long)bs);
  }
}

// one lane, behind a round: the centres of the partition it counted and the next threshold
__global__ void k_tm_update(uint64_t m, int max_iter, TmState* __restrict__ st) {
  if (st->done) return;
  const unsigned long long n_low = st->n_low, n_high = m - n_low;     // both >= 1
  const unsigned long long c0 = st->sum_low / n_low, c1 = (st->total - st->sum_low) / n_high;
  const unsigned long long t = st->t, tn = (c0 + c1) / 2 + 1;
  st->rep_t = t; st->rep_n_high = n_high; st->rep_c0 = c0; st->rep_c1 = c1;
  st->n_low = 0; st->sum_low = 0;
  const int it = ++st->iterations;
  if (tn == t) { st->converged = 1; st->done = 1; }
  else if (it >= max_iter) { st->converged = 0; st->done = 1; }
  else st->t = tn;
}

// the smallest score at or above t (as a quantised value), the largest below, and the labels of the high cluster
__global__ __launch_bounds__(AUC_THREADS) void k_tm_final(int rows, const float* __restrict__ S, int64_t lds,
                                                          const int64_t* __restrict__ idx, const uint8_t* __restrict__ lab,
                                                          uint64_t t, TmState* __restrict__ st) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  __shared__ uint32_t shm[AUC_THREADS / 64];
  uint64_t tp = 0;
  uint32_t inv_hi = 0, lo = 0;
  tri_for_each(rows, idx, [&](int a, int b, int64_t u, int64_t v) {
    const float s = S[u * lds + v];
    const uint32_t key = auc_key(s);
    if ((uint64_t)tm_quantise(__float_as_uint(s) & 0x7fffffffu) >= t) {
      inv_hi = max(inv_hi, ~key);
      if (lab && lab[(uint64_t)a * (a - 1) / 2 + b]) ++tp;
    } else {
      lo = max(lo, key);
    }
  });
  const uint64_t btp = block_sum_u64(tp, sh);
  const uint32_t bhi = block_max_u32(inv_hi, shm);
  __syncthreads();
  const uint32_t blo = block_max_u32(lo, shm);
  if (threadIdx.x == 0) {
    if (btp) atomicAdd(&st->tp, (unsigned long long)btp);
    atomicMax(&st->inv_hi_min, bhi);
    atomicMax(&st->lo_max, blo);
  }
}

// block b's contiguous packed range [b tile, (b + 1) tile): cnt[b] = its pairs with a key >= T (cnt[nb] = 0: the scan's
// entry nb is then the total); st->hits += those with label 1; st->flags |= argument errors
__global__ __launch_bounds__(AUC_THREADS) void k_tp_count(uint64_t count, uint64_t tile, int nb, const float* __restrict__ S,
                                                          int64_t lds, const float* __restrict__ L, int64_t ldl,
                                                          const int64_t* __restrict__ idx, uint32_t T,
                                                          uint32_t* __restrict__ cnt, TpState* __restrict__ st) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  const uint64_t beg = blockIdx.x * tile, end = min(count, beg + tile);
  uint64_t c = 0, h = 0;
  int f = 0;
  for (uint64_t e = beg + threadIdx.x; e < end; e += AUC_THREADS) {
    uint32_t a, b;
    topk_unpack((uint32_t)e, a, b);
    const int64_t u = idx ? idx[a] : a, v = idx ? idx[b] : b;
    const float s = S[u * lds + v];
    if (!auc_finite(s)) f |= AUC_BAD_SCORE;
    const bool in = auc_key(s) >= T;
    c += in ? 1u : 0u;
    if (L) {
      const float l = L[u * ldl + v];
      const bool p = auc_pos(l);
      if (p) h += in ? 1u : 0u;
      else if (!auc_neg(l)) f |= AUC_BAD_LABEL;
    }
  }
  if (f) atomicOr(&st->flags, f);
  const uint64_t bc = block_sum_u64(c, sh);
  __syncthreads();
  const uint64_t bh = block_sum_u64(h, sh);
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = (uint32_t)bc;
    if (blockIdx.x == 0) cnt[nb] = 0u;
    if (bh) atomicAdd(&st->hits, (unsigned long long)bh);
  }
}

// the qualifying pairs of block b's range in packed order, 256 positions a step, at off[b] + their rank inside the range
__global__ __launch_bounds__(AUC_THREADS) void k_tp_write(uint64_t count, uint64_t tile, const float* __restrict__ S, int64_t lds,
                                                          const float* __restrict__ L, int64_t ldl,
                                                          const int64_t* __restrict__ idx, uint32_t T,
                                                          const uint64_t* __restrict__ off, int64_t* __restrict__ pairs,
                                                          float* __restrict__ pair_scores, uint8_t* __restrict__ hits) {
  __shared__ uint32_t wc[2][AUC_THREADS / 64];
  const uint64_t beg = blockIdx.x * tile, end = min(count, beg + tile);
  uint64_t run = off[blockIdx.x];
  int par = 0;
  for (uint64_t base = beg; base < end; base += AUC_THREADS, par ^= 1) {
    const uint64_t e = base + threadIdx.x;
    int64_t u = 0, v = 0;
    float s = 0.f;
    bool in = false;
    if (e < end) {
      uint32_t a, b;
      topk_unpack((uint32_t)e, a, b);
      u = idx ? idx[a] : a; v = idx ? idx[b] : b;
      s = S[u * lds + v];
      in = auc_key(s) >= T;
    }
    const BlockRank r = block_rank(in, wc, par);
    const uint64_t at = run + r.before;
    if (in) {
      pairs[2 * at] = u;
      pairs[2 * at + 1] = v;
      if (pair_scores) pair_scores[at] = s;
      if (hits) hits[at] = auc_pos(L[u * ldl + v]) ? 1 : 0;
    }
    run += r.all;
  }
}

}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_two_means_split(void* stream, int n, const float* scores, int ld_scores, const float* labels,
                                     int ld_labels, const int64_t* idx, int64_t n_idx, int max_iter, int64_t* out,
                                     float* thr_high, float* thr_low) {
  const char* who = "two_means_split";
  if (!out || max_iter < 1) { set_error("%s: bad argument", who); return MCGRA_EINVAL; }
  if (int rc = rank_check_args(who, n, {{scores, ld_scores, true}, {labels, ld_labels, false}}, idx, n_idx, 2)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int rows = (int)n_idx;
  const uint64_t m = (uint64_t)rows * (rows - 1) / 2;
  AucBufs b;
  TmState* state = b.get<TmState>(1);
  uint32_t* q = b.get<uint32_t>(m);
  uint8_t* lab = labels ? b.get<uint8_t>(m) : nullptr;
  if (!state || !q || (labels && !lab)) {
    set_error("%s: hipMalloc of the scratch of %llu pairs failed", who, (unsigned long long)m);
    return MCGRA_ENOMEM;
  }
  MCGRA_HIP(hipMemsetAsync(state, 0, sizeof(TmState), st));
  if (int rc = rank_check_idx(who, st, b, n, idx, rows, &state->flags)) return rc;
  TmState h{};
  auto fetch = [&]() -> int {
    MCGRA_HIP(hipMemcpyAsync(&h, state, sizeof(TmState), hipMemcpyDeviceToHost, st));
    MCGRA_HIP(hipStreamSynchronize(st));
    return 0;
  };
  const int gr = std::min(rows - 1, TM_ROW_BLOCKS);
  k_tm_emit<<<gr, AUC_THREADS, 0, st>>>(rows, scores, ld_scores, labels, ld_labels, idx, q, lab, state);
  k_tm_start<<<1, 1, 0, st>>>(state);
  MCGRA_KERNEL_CHECK();
  if (int rc = fetch()) return rc;
  if (int rc = rank_flag_error(who, h.flags)) return rc;
  if (h.flags & TM_BAD_RANGE) {
    set_error("%s: a selected score is below 0 or not below 16 (q = rint(s 2^28) must fit 32 bits)", who);
    return MCGRA_ENOSUP;
  }
  const uint64_t lo = (uint32_t)~h.inv_min, hi = h.max;
  const int64_t P = labels ? (int64_t)h.P : -1;
  if (lo == hi) {                                                 // one value: nothing to split
    const int64_t r[10] = {(int64_t)m, 0, 1, (int64_t)lo + 1, 0, (int64_t)lo, (int64_t)lo, P, labels ? 0 : -1, 1};
    memcpy(out, r, sizeof(r));
    return 0;
  }
  const int gs = (int)std::min<uint64_t>(TM_BLOCKS, (m + TM_STEP - 1) / TM_STEP);
  for (int launched = 0; !h.done;) {                              // done is set at the latest by round max_iter
    const int batch = std::min(TM_BATCH, max_iter - launched);
    if (batch < 1) { set_error("%s: %d rounds ran and none ended the iteration", who, launched); return MCGRA_EHIP; }
    for (int i = 0; i < batch; ++i) {
      k_tm_round<<<gs, AUC_THREADS, 0, st>>>(q, m, state);
      k_tm_update<<<1, 1, 0, st>>>(m, max_iter, state);
    }
    MCGRA_KERNEL_CHECK();
    launched += batch;
    if (int rc = fetch()) return rc;
  }
  k_tm_final<<<gr, AUC_THREADS, 0, st>>>(rows, scores, ld_scores, idx, lab, h.rep_t, state);
  MCGRA_KERNEL_CHECK();
  if (int rc = fetch()) return rc;
  const int64_t r[10] = {(int64_t)m, h.iterations, h.converged, (int64_t)h.rep_t, (int64_t)h.rep_n_high, (int64_t)h.rep_c0,
                         (int64_t)h.rep_c1, P, labels ? (int64_t)h.tp : -1, 0};
  memcpy(out, r, sizeof(r));
  const uint32_t bh = tm_key_bits(~h.inv_hi_min), bl = tm_key_bits(h.lo_max);
  if (thr_high) memcpy(thr_high, &bh, sizeof(float));
  if (thr_low) memcpy(thr_low, &bl, sizeof(float));
  return 0;
}

extern "C" int mcgra_threshold_pairs(void* stream, int n, const float* scores, int ld_scores, const float* labels,
                                     int ld_labels, const int64_t* idx, int64_t n_idx, float threshold, int64_t cap,
                                     int64_t* pairs, float* pair_scores, uint8_t* hits, int64_t* counts) {
  const char* who = "threshold_pairs";
  if (!counts || cap < 0 || (cap > 0 && !pairs) || (hits && !labels) || threshold != threshold) {
    set_error("%s: bad argument%s", who, threshold != threshold ? " (the threshold is NaN)" : "");
    return MCGRA_EINVAL;
  }
  if (int rc = rank_check_args(who, n, {{scores, ld_scores, true}, {labels, ld_labels, false}}, idx, n_idx, 2)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int rows = (int)n_idx;
  const uint64_t m = (uint64_t)rows * (rows - 1) / 2;
  AucBufs b;
  TpState* state = b.get<TpState>(1);
  uint32_t* cnt = b.get<uint32_t>(TP_BLOCKS + 1);
  uint64_t* off = b.get<uint64_t>(TP_BLOCKS + 1);
  if (!state || !cnt || !off) { set_error("%s: hipMalloc failed", who); return MCGRA_ENOMEM; }
  MCGRA_HIP(hipMemsetAsync(state, 0, sizeof(TpState), st));
  if (int rc = rank_check_idx(who, st, b, n, idx, rows, &state->flags)) return rc;
  const uint32_t T = auc_key_host(threshold);
  const auto [tile, nb] = rank_tiles(m, TP_BLOCKS, AUC_THREADS);
  k_tp_count<<<nb, AUC_THREADS, 0, st>>>(m, tile, nb, scores, ld_scores, labels, ld_labels, idx, T, cnt, state);
  rank_scan(st, cnt, nb + 1, off);
  MCGRA_KERNEL_CHECK();
  TpState h{};
  uint64_t total = 0;
  MCGRA_HIP(hipMemcpyAsync(&h, state, sizeof(TpState), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipMemcpyAsync(&total, off + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (int rc = rank_flag_error(who, h.flags)) return rc;
  counts[0] = (int64_t)m; counts[1] = (int64_t)total; counts[2] = labels ? (int64_t)h.hits : -1;
  if ((int64_t)total > cap) {
    if (cap == 0 && !pairs) return 0;                             // the counts alone were asked for
    set_error("%s: %lld pairs are at or above the threshold, cap is %lld (counts holds what is needed)", who, (long long)total,
              (long long)cap);
    return MCGRA_ENOMEM;
  }
  if (total == 0) return 0;
  k_tp_write<<<nb, AUC_THREADS, 0, st>>>(m, tile, scores, ld_scores, labels, ld_labels, idx, T, off, pairs, pair_scores, hits);
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipStreamSynchronize(st));                            // the scratch is freed on return
  return 0;
}
