// What the placement entries share (delong.hip: DeLong's sums; node_jackknife.hip: the per-node sums): one scoring's device
// arrays, the search of a negative among the sorted positives through samples staged in LDS, the wave-merged histogram add,
// a negative's and a positive's placement, and the argument checks that need no device.  Integer work only.  Each
// translation unit gets its own copy.
#pragma once
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int DL_STAGE = 4096;             // samples of the sorted positives a block of the negatives' pass keeps in LDS, per scoring
enum { DL_BAD_SCORE_B = 32 };              // beside the AUC_BAD_* flags: the second score matrix

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

// first index in [lo, hi) of the ascending keys B whose key is >= x (UPPER: > x); hi when there is none
template <bool UPPER, class Keys, class I>
__device__ __forceinline__ I dl_bound(const Keys& B, I lo, I hi, uint32_t x) {
  while (lo < hi) {
    const I mid = lo + ((hi - lo) >> 1);
    const uint32_t k = B[mid];
    if (UPPER ? k <= x : k < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// dl_bound over all np sorted positives S through the ns samples smp[q] = S[q stride]: the bound among the samples leaves one
// stretch between two samples.  c = first sample >= x (> x): every position up to (c - 1) stride is below (at or below) x and
// position c stride is not, so the bound lies in ((c - 1) stride, c stride]; past the last sample it lies before np.
template <bool UPPER>
__device__ __forceinline__ uint32_t dl_find(const uint32_t* __restrict__ S, uint32_t np, const uint32_t* smp, uint32_t ns,
                                            uint32_t stride, uint32_t x) {
  const uint32_t c = dl_bound<UPPER>(smp, 0u, ns, x);
  if (c == 0) return 0;
  const uint32_t lo = (c - 1) * stride + 1, hi = c < ns ? c * stride : np;
  return dl_bound<UPPER>(S, lo, hi, x);
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
  const uint32_t l = dl_bound<false>(s.sorted, 0u, np, s.slot[slot]);      // its own key is there: l < np
  return 2 * (s.cum[l] + s.hist[l]) - s.ties[l];                          // <= 2 N < 2^32
}

// the argument checks that need no device
inline int dl_check(const char* who, int n, const float* labels, int ld_labels, const float* sa, int ld_a, const float* sb,
                    int ld_b, bool paired, const int64_t* idx, int64_t& n_idx, const void* out) {
  if (!idx) n_idx = n;
  if (n < 1 || !labels || !sa || (paired && !sb) || !out || ld_labels < n || ld_a < n || (paired && ld_b < n) || n_idx < 2) {
    set_error("%s: bad argument (n >= 1, the matrices and out not NULL, every ld >= n, at least 2 selected nodes)", who);
    return MCGRA_EINVAL;
  }
  if (n_idx > AUC_MAX_NIDX) {
    set_error("%s: %lld selected nodes; a pair count of more than %lld nodes does not fit 31 bits", who, (long long)n_idx,
              (long long)AUC_MAX_NIDX);
    return MCGRA_ENOSUP;
  }
  return 0;
}
}  // namespace
}  // namespace mcgra
