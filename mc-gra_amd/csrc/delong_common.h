// What the placement entries share (delong.hip: DeLong's sums; node_jackknife.hip: the per-node sums): one scoring's device
// arrays, the search of a negative among the sorted positives through samples staged in LDS, the wave-merged histogram add,
// a negative's and a positive's placement, and the positives' stage -- k_dl_classify, the host's dl_counted behind it, and
// k_dl_emit -- parameterised by what travels with a positive (NODES false, DeLong: the key of the second scoring, if there is
// one; NODES true, the jackknife: the pair's endpoints a << 16 | b, and the count of positives per position).  Integer work
// only.  Each of the two files instantiates its own variant of the two kernels.
#pragma once
#include <vector>

#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int DL_STAGE = 4096;             // samples of the sorted positives a block of the negatives' pass keeps in LDS, per scoring

// what one scoring's positives need on the device
struct DlSide {
  const float* S;        // the score matrix (NULL: no second scoring)
  int64_t ld;
  uint32_t* slot;        // [P] the positives' keys by slot
  uint32_t* sorted;      // [P] ascending
  uint32_t* hist;        // [P + 1] negatives whose lb is this position
  uint32_t* ties;        // [P + 1] of those, the ones equal to the positive at this position
  uint64_t* cum;         // [P + 1] hist[0] + ... + hist[l - 1]
};

// rank_bound over all np sorted positives S through the ns samples smp[q] = S[q stride]: the bound among the samples leaves one
// stretch between two samples.  c = first sample >= x (> x): every position up to (c - 1) stride is below (at or below) x and
// position c stride is not, so the bound lies in ((c - 1) stride, c stride]; past the last sample it lies before np.
template <bool UPPER>
__device__ __forceinline__ uint32_t dl_find(const uint32_t* __restrict__ S, uint32_t np, const uint32_t* smp, uint32_t ns,
                                            uint32_t stride, uint32_t x) {
  const uint32_t c = rank_bound<UPPER>(smp, 0u, ns, x);
  if (c == 0) return 0;
  const uint32_t lo = (c - 1) * stride + 1, hi = c < ns ? c * stride : np;
  return rank_bound<UPPER>(S, lo, hi, x);
}

// h[bin] += 1 for every lane with `on`.  The lanes of the wave that share one of its first DL_SHARED_BINS distinct bins add
// once (tied scores and scores outside the positives' range put a whole wave into a few bins: one address would serialise 64
// atomics); lanes left after that hold scattered bins and add on their own.  Every lane that is active in the caller must
// call it (the loop is the same in all of them).
constexpr int DL_SHARED_BINS = 4;
__device__ __forceinline__ void dl_hist_add(uint32_t* __restrict__ h, uint32_t bin, bool on) {
  const int lane = threadIdx.x & 63;
  uint64_t todo = __ballot(on);
  for (int it = 0; it < DL_SHARED_BINS && todo; ++it) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t lb = __shfl(bin, leader, 64);
    const uint64_t same = __ballot(on && bin == lb);
    if (lane == leader) atomicAdd(&h[lb], (uint32_t)__popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&h[bin], 1u);
}

// one scoring's share of a negative: lb, ub among the sorted positives, the two counts, the placement 2 np - lb - ub
__device__ __forceinline__ uint32_t dl_negative(const DlSide& s, uint32_t np, const uint32_t* smp, uint32_t ns, uint32_t stride,
                                                float score, bool neg) {
  uint32_t lb = 0, ub = 0;
  bool tie = false;
  if (neg) {
    const uint32_t x = auc_key(score);
    lb = dl_find<false>(s.sorted, np, smp, ns, stride, x);
    tie = lb < np && s.sorted[lb] == x;
    ub = tie ? dl_find<true>(s.sorted, np, smp, ns, stride, x) : lb;
  }
  dl_hist_add(s.hist, lb, neg);
  dl_hist_add(s.ties, lb, tie);
  return 2u * np - lb - ub;          // <= 2 np < 2^32
}

// one scoring's share of the positive at `slot`: a = 2 (negatives at or below it) - (negatives equal to it)
__device__ __forceinline__ uint64_t dl_positive(const DlSide& s, uint32_t np, uint64_t slot) {
  const uint32_t l = rank_bound<false>(s.sorted, 0u, np, s.slot[slot]);      // its own key is there: l < np
  return 2 * (s.cum[l] + s.hist[l]) - s.ties[l];                          // <= 2 N < 2^32
}

// counts[b] = positives of block b's rows; flags |= the argument errors it meets (SB != NULL: of the second scoring too);
// NODES: deg[v] = positives that contain position v
template <bool NODES>
__global__ __launch_bounds__(AUC_THREADS) void k_dl_classify(int rows, const float* __restrict__ SA, int64_t lda,
                                                             const float* __restrict__ SB, int64_t ldb,
                                                             const float* __restrict__ L, int64_t ldl,
                                                             const int64_t* __restrict__ idx, uint64_t* __restrict__ counts,
                                                             uint32_t* __restrict__ deg, int* __restrict__ flags) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  uint32_t pos = 0, mine = 0;                          // mine: this lane's positives of the row at hand
  int f = 0;
  tri_for_each(rows, idx, [&](int, int b, int64_t u, int64_t v) {
    const float l = L[u * ldl + v];
    if (!auc_finite(SA[u * lda + v])) f |= AUC_BAD_SCORE;
    if (!NODES && SB && !auc_finite(SB[u * ldb + v])) f |= DL_BAD_SCORE_B;
    if (auc_pos(l)) { ++mine; if (NODES) atomicAdd(&deg[b], 1u); }
    else if (!auc_neg(l)) f |= AUC_BAD_LABEL;   // also NaN
  }, [&](int a) {
    if (NODES && mine) atomicAdd(&deg[a], mine);
    pos += mine;
    mine = 0;
  });
  if (f) atomicOr(flags, f);
  const uint64_t p = block_sum_u64(pos, sh);
  if (threadIdx.x == 0) counts[blockIdx.x] = p;
}

// block b's positives take the slots offs[b] .. (any order inside a block): ka[slot] = key of the pair's score in SA;
// second[slot] = NODES: its endpoints a << 16 | b; else (SB != NULL) the key of its score in SB
template <bool NODES>
__global__ __launch_bounds__(AUC_THREADS) void k_dl_emit(int rows, const float* __restrict__ SA, int64_t lda,
                                                         const float* __restrict__ SB, int64_t ldb,
                                                         const float* __restrict__ L, int64_t ldl,
                                                         const int64_t* __restrict__ idx, const uint64_t* __restrict__ offs,
                                                         uint32_t* __restrict__ ka, uint32_t* __restrict__ second) {
  __shared__ uint32_t cur;
  if (threadIdx.x == 0) cur = 0;
  __syncthreads();
  const uint64_t o_pos = offs[blockIdx.x];
  tri_for_each(rows, idx, [&](int a, int b, int64_t u, int64_t v) {
    const bool p = auc_pos(L[u * ldl + v]);
    const uint64_t at = o_pos + wave_slot(p, &cur);
    if (!p) return;
    ka[at] = auc_key(SA[u * lda + v]);
    if (NODES) second[at] = (uint32_t)a << 16 | (uint32_t)b;
    else if (SB) second[at] = auc_key(SB[u * ldb + v]);
  });
}

// Behind the classify pass of g blocks: its counts and flags come back (one sync), a flagged argument is refused, h[b]
// becomes the slots before block b, and P, N are the two classes of the rows (rows - 1) / 2 pairs.
inline int dl_counted(const char* who, hipStream_t st, const uint64_t* counts, const int* flags, int g, bool paired, int rows,
                      std::vector<uint64_t>& h, uint64_t& P, uint64_t& N) {
  h.resize(g);
  int h_flags = 0;
  MCGRA_HIP(hipMemcpyAsync(h.data(), counts, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (int rc = rank_flag_error(who, h_flags, paired)) return rc;
  P = 0;
  for (int i = 0; i < g; ++i) { const uint64_t p = h[i]; h[i] = P; P += p; }        // counts -> offsets
  N = (uint64_t)rows * (rows - 1) / 2 - P;
  return 0;
}
}  // namespace
}  // namespace mcgra
