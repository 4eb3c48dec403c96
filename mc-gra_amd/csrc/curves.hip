// The ROC and precision-recall curves of a scored square matrix restricted to idx x idx (mcgra_rank_curves): what
// sklearn.metrics.roc_curve and precision_recall_curve return for labels[idx][:, idx] against scores[idx][:, idx], as exact
// integer counts per kept threshold, and the level of the best F1.  Classify, emit and the two sorts are AucRun's (auc.hip);
// this file is the third consumer of the two sorted key regions: Pk[0, P) the positives' keys ascending, Nk[0, N) the
// negatives'.  The larger of the two is region A, the smaller region B.
//
// A LEVEL is a distinct selected score; levels are numbered by descending score, l = 0 the highest.  Level l carries
// tp[l] = #positives with a key >= its key, fp[l] = the same for negatives (sklearn's _binary_clf_curve).
//
// Passes:
//   k_cv_head_count    per contiguous tile of a region: its level heads.  A head of A is the first key of a run of equal keys;
//                      a head of B is such a key that A does not hold (one lower bound in A), so every level has one head
//   rank_scan          one block scans the per-tile counts (rank_common.hip); entry nb of the scan is the region's total
//   k_cv_head_cum      cum[i] = heads of the region at indices < i (the tile's offset, then block_rank in index order),
//                      into the sort's second key buffer, which is free after the sorts
//   k_cv_levels        every head: one lower bound lb in the other region; its ascending rank among the levels is
//                      cum_own[i] + cum_other[lb], its counts are (n_own - i, n_other - lb); it writes (tp, fp, key) at
//                      l = levels - 1 - rank.  Each level is written exactly once
//   k_cv_keep_count    per tile of levels: the levels roc_curve keeps and those precision_recall_curve keeps (a stencil on
//                      l - 1, l, l + 1 read from the level arrays, so a tile's edge is no special case), and the tile's best
//                      F1 level; two scans; k_cv_best merges the tiles' best levels in one block
//   k_cv_write         the same stencil again; every kept level is ranked inside its tile in index order and copied to the
//                      caller's buffers behind the tile's offset (ROC: behind point 0 = (0, 0, +inf))
// Everything is integers and copied key bits: per-tile counts over fixed contiguous ranges merged by a scan, a strict total
// order for the best level, no atomics at all and no floating-point arithmetic.  So no result depends on the order in which
// blocks run and every call returns the same bits.
// Best F1: 2 tp / (tp + fp + P) is compared as tp1 (tp2 + fp2 + P) against tp2 (tp1 + fp1 + P), both below 2^32 * 2^34, in
// 128 bits (__umul64hi and the low product); equal values go to the lower l (the higher threshold).
// Device scratch: the 8 bytes per selected entry of the sort (keys and the second buffer, reused for cum) + 12 bytes per
// level (tp, fp and key as 32-bit words; levels <= selected entries) + about 3 MB of counts, offsets and candidates.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "../../include/mcgra.h"
#include "common.h"
#include "curves.h"
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int CV_BLOCKS = 65536;           // at most this many contiguous tiles (and blocks) per pass; one block scans their counts
constexpr int CV_GRID = 4096;              // blocks of the grid-stride pass over the heads

// first index of R[0, n) whose key is >= x
__device__ __forceinline__ uint64_t cv_lower(const uint32_t* __restrict__ R, uint64_t n, uint32_t x) {
  return rank_bound<false>(R, (uint64_t)0, n, x);
}

// R[i] heads a level: the first key of its run and, EXCL, a key the other region O does not hold
template <bool EXCL>
__device__ __forceinline__ bool cv_head(const uint32_t* __restrict__ R, uint64_t i, const uint32_t* __restrict__ O, uint64_t no) {
  const uint32_t x = R[i];
  if (i && R[i - 1] == x) return false;
  if (!EXCL) return true;
  const uint64_t lb = cv_lower(O, no, x);
  return !(lb < no && O[lb] == x);
}

// the score of a key (auc_key inverted; the key of -0.0 and +0.0 gives +0.0)
__device__ __forceinline__ float cv_score(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// roc_curve's and precision_recall_curve's keep rules at level l of L (drop: drop_intermediate and L > 2)
__device__ __forceinline__ bool cv_keep_roc(const uint32_t* __restrict__ ltp, const uint32_t* __restrict__ lfp, uint64_t L,
                                            uint64_t l, bool drop) {
  if (!drop || l == 0 || l + 1 == L) return true;
  const int64_t f0 = lfp[l - 1], f1 = lfp[l], f2 = lfp[l + 1], t0 = ltp[l - 1], t1 = ltp[l], t2 = ltp[l + 1];
  return f0 - 2 * f1 + f2 != 0 || t0 - 2 * t1 + t2 != 0;
}
__device__ __forceinline__ bool cv_keep_pr(const uint32_t* __restrict__ ltp, uint64_t L, uint64_t l, bool drop) {
  if (!drop || l == 0 || l + 1 == L) return true;
  const uint32_t t1 = ltp[l];
  return t1 != ltp[l - 1] || ltp[l + 1] != t1;
}

// a candidate for the best F1: level l with tp and d = tp + fp + P; l = ~0 is "none" (tp = 0, d = 1: any level beats it)
struct CvBest { uint64_t tp, d, l; };
// a's F1 is higher than b's, or equal at a lower level: tp_a d_b against tp_b d_a in 128 bits
__device__ __forceinline__ bool cv_better(const CvBest& a, const CvBest& b) {
  const uint64_t ha = __umul64hi(a.tp, b.d), la = a.tp * b.d, hb = __umul64hi(b.tp, a.d), lb = b.tp * a.d;
  if (ha != hb) return ha > hb;
  if (la != lb) return la > lb;
  return a.l < b.l;
}
// the best candidate of the block, valid in thread 0 (the order is total, so every lane of a wave ends with the same one)
__device__ __forceinline__ CvBest cv_block_best(CvBest v, CvBest* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const CvBest u{__shfl_xor(v.tp, o, 64), __shfl_xor(v.d, o, 64), __shfl_xor(v.l, o, 64)};
    if (cv_better(u, v)) v = u;
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 1; q < AUC_THREADS / 64; ++q)
      if (cv_better(sh[q], v)) v = sh[q];
  return v;
}
}  // namespace

// cnt[b] = level heads of tile b = R[b tile, (b + 1) tile); cnt[nb] = 0 (the scan's entry nb is then the total)
template <bool EXCL>
__global__ __launch_bounds__(AUC_THREADS) void k_cv_head_count(const uint32_t* __restrict__ R, uint64_t n,
                                                               const uint32_t* __restrict__ O, uint64_t no, uint64_t tile,
                                                               int nb, uint32_t* __restrict__ cnt) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  const uint64_t beg = blockIdx.x * tile, end = min(n, beg + tile);
  uint64_t c = 0;
  for (uint64_t e = beg + threadIdx.x; e < end; e += AUC_THREADS) c += cv_head<EXCL>(R, e, O, no) ? 1u : 0u;
  const uint64_t tot = block_sum_u64(c, sh);
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = (uint32_t)tot;
    if (blockIdx.x == 0) cnt[nb] = 0u;
  }
}

// cum[i] = level heads of the region at indices < i, for every i of tile b (off[b]: those before the tile)
template <bool EXCL>
__global__ __launch_bounds__(AUC_THREADS) void k_cv_head_cum(const uint32_t* __restrict__ R, uint64_t n,
                                                             const uint32_t* __restrict__ O, uint64_t no, uint64_t tile,
                                                             const uint64_t* __restrict__ off, uint32_t* __restrict__ cum) {
  __shared__ uint32_t w[2][AUC_THREADS / 64];
  const uint64_t beg = blockIdx.x * tile, end = min(n, beg + tile);
  uint64_t run = off[blockIdx.x];
  int par = 0;
  for (uint64_t base = beg; base < end; base += AUC_THREADS, par ^= 1) {
    const uint64_t e = base + threadIdx.x;
    const bool valid = e < end;
    const bool f = valid && cv_head<EXCL>(R, e, O, no);
    const BlockRank r = block_rank(f, w, par);
    if (valid) cum[e] = (uint32_t)(run + r.before);
    run += r.all;
  }
}

// every head R[i] writes its level: (tp, fp, key) at l = L - 1 - (cumR[i] + heads of O below its key).  r_pos: R holds the
// positives.  tot_o: the heads of O.
template <bool EXCL>
__global__ __launch_bounds__(AUC_THREADS) void k_cv_levels(const uint32_t* __restrict__ R, uint64_t n,
                                                           const uint32_t* __restrict__ cumR, const uint32_t* __restrict__ O,
                                                           uint64_t no, const uint32_t* __restrict__ cumO, uint64_t tot_o,
                                                           uint64_t L, int r_pos, uint32_t* __restrict__ ltp,
                                                           uint32_t* __restrict__ lfp, uint32_t* __restrict__ lkey) {
  for (uint64_t i = (uint64_t)blockIdx.x * AUC_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * AUC_THREADS) {
    const uint32_t x = R[i];
    if (i && R[i - 1] == x) continue;
    const uint64_t lb = cv_lower(O, no, x);
    if (EXCL && lb < no && O[lb] == x) continue;
    const uint64_t rank = (uint64_t)cumR[i] + (lb == no ? tot_o : (uint64_t)cumO[lb]);
    if (rank >= L) continue;                          // (cannot happen: the ranks of the L heads are 0 .. L - 1)
    const uint64_t l = L - 1 - rank;
    const uint32_t ge_r = (uint32_t)(n - i), ge_o = (uint32_t)(no - lb);
    ltp[l] = r_pos ? ge_r : ge_o;
    lfp[l] = r_pos ? ge_o : ge_r;
    lkey[l] = x;
  }
}

// tile b of the levels: cnt_roc[b] / cnt_pr[b] = the levels the two rules keep (entry nb = 0), bb[3 b ..] = the tile's best
// F1 candidate (P > 0 only)
__global__ __launch_bounds__(AUC_THREADS) void k_cv_keep_count(uint64_t L, const uint32_t* __restrict__ ltp,
                                                               const uint32_t* __restrict__ lfp, int drop, uint64_t tile, int nb,
                                                               uint64_t P, uint32_t* __restrict__ cnt_roc,
                                                               uint32_t* __restrict__ cnt_pr, uint64_t* __restrict__ bb) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  __shared__ CvBest shb[AUC_THREADS / 64];
  const uint64_t beg = blockIdx.x * tile, end = min(L, beg + tile);
  uint64_t cr = 0, cp = 0;
  CvBest best{0, 1, ~0ull};
  for (uint64_t l = beg + threadIdx.x; l < end; l += AUC_THREADS) {
    cr += cv_keep_roc(ltp, lfp, L, l, drop != 0) ? 1u : 0u;
    cp += cv_keep_pr(ltp, L, l, drop != 0) ? 1u : 0u;
    if (P) {
      const uint64_t tp = ltp[l];
      const CvBest c{tp, tp + lfp[l] + P, l};
      if (cv_better(c, best)) best = c;
    }
  }
  const uint64_t r = block_sum_u64(cr, sh);
  __syncthreads();
  const uint64_t p = block_sum_u64(cp, sh);
  best = cv_block_best(best, shb);
  if (threadIdx.x == 0) {
    cnt_roc[blockIdx.x] = (uint32_t)r;
    cnt_pr[blockIdx.x] = (uint32_t)p;
    if (blockIdx.x == 0) { cnt_roc[nb] = 0u; cnt_pr[nb] = 0u; }
    bb[3 * (size_t)blockIdx.x] = best.tp; bb[3 * (size_t)blockIdx.x + 1] = best.d; bb[3 * (size_t)blockIdx.x + 2] = best.l;
  }
}

// one block: out = {tp, fp, l, key} of the best of the nb tiles' candidates
__global__ __launch_bounds__(AUC_THREADS) void k_cv_best(const uint64_t* __restrict__ bb, int nb, uint64_t P,
                                                         const uint32_t* __restrict__ lkey, uint64_t* __restrict__ out) {
  __shared__ CvBest shb[AUC_THREADS / 64];
  CvBest best{0, 1, ~0ull};
  for (int b = threadIdx.x; b < nb; b += AUC_THREADS) {
    const CvBest c{bb[3 * (size_t)b], bb[3 * (size_t)b + 1], bb[3 * (size_t)b + 2]};
    if (cv_better(c, best)) best = c;
  }
  best = cv_block_best(best, shb);
  if (threadIdx.x == 0 && best.l != ~0ull) {
    out[0] = best.tp; out[1] = best.d - best.tp - P; out[2] = best.l; out[3] = lkey[best.l];
  }
}

// the kept levels of tile b in level order: ROC point 1 + off_roc[b] + rank, PR point off_pr[b] + rank (either curve's
// buffers may be NULL); block 0 writes ROC point 0 = (0, 0, +inf)
__global__ __launch_bounds__(AUC_THREADS) void k_cv_write(uint64_t L, const uint32_t* __restrict__ ltp,
                                                          const uint32_t* __restrict__ lfp, const uint32_t* __restrict__ lkey,
                                                          int drop, uint64_t tile, const uint64_t* __restrict__ off_roc,
                                                          const uint64_t* __restrict__ off_pr, int64_t* __restrict__ roc_tps,
                                                          int64_t* __restrict__ roc_fps, float* __restrict__ roc_thr,
                                                          int64_t* __restrict__ pr_tps, int64_t* __restrict__ pr_fps,
                                                          float* __restrict__ pr_thr) {
  __shared__ uint32_t wr[2][AUC_THREADS / 64], wp[2][AUC_THREADS / 64];
  if (roc_tps && blockIdx.x == 0 && threadIdx.x == 0) { roc_tps[0] = 0; roc_fps[0] = 0; roc_thr[0] = INFINITY; }
  const uint64_t beg = blockIdx.x * tile, end = min(L, beg + tile);
  uint64_t run_r = 1 + off_roc[blockIdx.x], run_p = off_pr[blockIdx.x];
  int par = 0;
  for (uint64_t base = beg; base < end; base += AUC_THREADS, par ^= 1) {
    const uint64_t l = base + threadIdx.x;
    const bool valid = l < end;
    const int64_t tp = valid ? ltp[l] : 0, fp = valid ? lfp[l] : 0;
    const float thr = valid ? cv_score(lkey[l]) : 0.f;
    if (roc_tps) {                                    // (the same in every lane)
      const bool k = valid && cv_keep_roc(ltp, lfp, L, l, drop != 0);
      const BlockRank r = block_rank(k, wr, par);
      if (k) { const uint64_t at = run_r + r.before; roc_tps[at] = tp; roc_fps[at] = fp; roc_thr[at] = thr; }
      run_r += r.all;
    }
    if (pr_tps) {
      const bool k = valid && cv_keep_pr(ltp, L, l, drop != 0);
      const BlockRank r = block_rank(k, wp, par);
      if (k) { const uint64_t at = run_p + r.before; pr_tps[at] = tp; pr_fps[at] = fp; pr_thr[at] = thr; }
      run_p += r.all;
    }
  }
}

int rank_curves_sorted(const char* who, hipStream_t st, const uint32_t* keys, uint32_t* tmp, uint64_t P, uint64_t nbase,
                       uint64_t N, const CurveRequest& rq) {
  // region A: the larger class (every run of equal keys heads a level); region B: the smaller (its keys A does not hold)
  const bool a_pos = P >= N;
  const uint32_t* A = a_pos ? keys : keys + nbase;
  const uint32_t* B = a_pos ? keys + nbase : keys;
  uint32_t* cumA = a_pos ? tmp : tmp + nbase;
  uint32_t* cumB = a_pos ? tmp + nbase : tmp;
  const uint64_t na = a_pos ? P : N, nbk = a_pos ? N : P;
  AucBufs b;
  const size_t stride = (size_t)CV_BLOCKS + 1;
  uint32_t* cnt = b.get<uint32_t>(2 * stride);
  uint64_t* off = b.get<uint64_t>(2 * stride);
  uint64_t* res = b.get<uint64_t>(4);
  if (!cnt || !off || !res) { set_error("%s: hipMalloc failed", who); return MCGRA_ENOMEM; }

  const auto [tile_a, nb_a] = rank_tiles(na, CV_BLOCKS, AUC_THREADS);
  const auto [tile_b, nb_b] = rank_tiles(nbk, CV_BLOCKS, AUC_THREADS);       // no blocks when B is empty
  k_cv_head_count<false><<<nb_a, AUC_THREADS, 0, st>>>(A, na, B, nbk, tile_a, nb_a, cnt);
  rank_scan(st, cnt, nb_a + 1, off);
  uint64_t heads_a = 0, heads_b = 0;
  MCGRA_HIP(hipMemcpyAsync(&heads_a, off + nb_a, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (nbk) {
    k_cv_head_count<true><<<nb_b, AUC_THREADS, 0, st>>>(B, nbk, A, na, tile_b, nb_b, cnt + stride);
    rank_scan(st, cnt + stride, nb_b + 1, off + stride);
    MCGRA_HIP(hipMemcpyAsync(&heads_b, off + stride + nb_b, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  }
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipStreamSynchronize(st));
  const uint64_t L = heads_a + heads_b;                 // >= 1: a selection is never empty
  if (L < 1 || L > na + nbk) { set_error("%s: %llu levels of %llu entries", who, (unsigned long long)L, (unsigned long long)(na + nbk)); return MCGRA_EHIP; }

  uint32_t* ltp = b.get<uint32_t>(L);
  uint32_t* lfp = b.get<uint32_t>(L);
  uint32_t* lkey = b.get<uint32_t>(L);
  const auto [tile_l, nb_l] = rank_tiles(L, CV_BLOCKS, AUC_THREADS);
  uint64_t* bb = b.get<uint64_t>(3 * (size_t)nb_l);
  if (!ltp || !lfp || !lkey || !bb) { set_error("%s: hipMalloc of %llu levels failed", who, (unsigned long long)L); return MCGRA_ENOMEM; }
  k_cv_head_cum<false><<<nb_a, AUC_THREADS, 0, st>>>(A, na, B, nbk, tile_a, off, cumA);
  if (nbk) k_cv_head_cum<true><<<nb_b, AUC_THREADS, 0, st>>>(B, nbk, A, na, tile_b, off + stride, cumB);
  const int ga = (int)std::min<uint64_t>(CV_GRID, (na + AUC_THREADS - 1) / AUC_THREADS);
  k_cv_levels<false><<<ga, AUC_THREADS, 0, st>>>(A, na, cumA, B, nbk, cumB, heads_b, L, a_pos ? 1 : 0, ltp, lfp, lkey);
  if (nbk) {
    const int gb = (int)std::min<uint64_t>(CV_GRID, (nbk + AUC_THREADS - 1) / AUC_THREADS);
    k_cv_levels<true><<<gb, AUC_THREADS, 0, st>>>(B, nbk, cumB, A, na, cumA, heads_a, L, a_pos ? 0 : 1, ltp, lfp, lkey);
  }
  MCGRA_KERNEL_CHECK();

  const int drop = (rq.drop_intermediate && L > 2) ? 1 : 0;
  k_cv_keep_count<<<nb_l, AUC_THREADS, 0, st>>>(L, ltp, lfp, drop, tile_l, nb_l, P, cnt, cnt + stride, bb);
  rank_scan(st, cnt, nb_l + 1, off);
  rank_scan(st, cnt + stride, nb_l + 1, off + stride);
  uint64_t kept_roc = 0, kept_pr = 0, h_res[4] = {0, 0, 0, 0};
  MCGRA_HIP(hipMemcpyAsync(&kept_roc, off + nb_l, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipMemcpyAsync(&kept_pr, off + stride + nb_l, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  const bool want_best = P && (rq.best || rq.best_thr);
  if (want_best) {
    k_cv_best<<<1, AUC_THREADS, 0, st>>>(bb, nb_l, P, lkey, res);
    MCGRA_HIP(hipMemcpyAsync(h_res, res, sizeof(h_res), hipMemcpyDeviceToHost, st));
  }
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipStreamSynchronize(st));
  rq.counts[0] = (int64_t)P; rq.counts[1] = (int64_t)N; rq.counts[2] = (int64_t)L;
  rq.counts[3] = (int64_t)kept_roc + 1; rq.counts[4] = (int64_t)kept_pr;
  if (want_best) {
    if (rq.best) { rq.best[0] = (int64_t)h_res[0]; rq.best[1] = (int64_t)h_res[1]; rq.best[2] = (int64_t)h_res[2]; }
    if (rq.best_thr) {
      const uint32_t k = (uint32_t)h_res[3], u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
      memcpy(rq.best_thr, &u, sizeof(float));
    }
  }
  const int64_t need = std::max<int64_t>(rq.roc_tps ? rq.counts[3] : 0, rq.pr_tps ? rq.counts[4] : 0);
  if (need > rq.cap) {
    set_error("%s: the curves have %lld points, cap is %lld (counts holds each curve's)", who, (long long)need, (long long)rq.cap);
    return MCGRA_ENOMEM;
  }
  if (rq.roc_tps || rq.pr_tps) {
    k_cv_write<<<nb_l, AUC_THREADS, 0, st>>>(L, ltp, lfp, lkey, drop, tile_l, off, off + stride, rq.roc_tps, rq.roc_fps,
                                             rq.roc_thr, rq.pr_tps, rq.pr_fps, rq.pr_thr);
    MCGRA_KERNEL_CHECK();
    MCGRA_HIP(hipStreamSynchronize(st));              // the scratch is freed on return
  }
  return 0;
}

}  // namespace mcgra
