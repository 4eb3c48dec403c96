// What the placement entries share (delong.hip: DeLong's sums; node_jackknife.hip: the per-node sums; hop_auc.hip: the sums by
// distance; class_auc.hip: the sums inside a stratum).
// Host side, defined once in delong_common.hip with its kernels (k_dl_classify, k_dl_emit): the positives' stage, DlStage.
// Device side, inlined into each file's kernels: one scoring's device arrays, the samples of the sorted positives a block
// stages in LDS, the search of a key among the sorted positives (or a segment of them) through the samples, a candidate's
// placement, the wave-merged histogram add, and a negative's and a positive's share of DeLong's counts.  Integer work only.
#pragma once
#include <vector>

#include "rank_common.h"

namespace mcgra {
// ---- host side (delong_common.hip)
// The positives' stage of an entry over the candidates of mcgra_auc_delong: the pairs of positions a > b of `rows` selected
// nodes, label L[idx[a]][idx[b]], score SA[..] (SB != NULL: a second scoring of the same pairs), g blocks grid-striding over
// the selected rows.  In order:
//   start    one allocation {flags | the per-block counts | `extra` bytes of the caller's, 8-byte aligned}, zeroed;
//            rank_check_idx; k_dl_classify: the argument checks and the positives per block (deg != NULL, an offset into
//            extra: also deg[v] = the positives that contain position v).  Returns with the kernel in flight
//   counted  one sync: a flagged argument is refused; P, N = the two classes of the rows (rows - 1) / 2 candidates
//   pool     one allocation for what scales with P -- `p4` arrays of P4 and `h4` arrays of H4 32-bit words (P4 = P rounded up
//            to 4 keys, H4 = P4 + 4; a 64-bit array counts twice) and the sort's scratch; returns the carver behind the sort's
//            scratch.  The per-block offsets (the scan of the counts) replace the counts on the device
//   emit     k_dl_emit: block b's positives take the slots offs[b] .. (any order inside a block): ka[slot] = the key of the
//            pair's score in SA; second[slot] = with deg its endpoints a << 16 | b, else (SB != NULL) the key of its score in
//            SB.  An entry that carries something else launches its own kernel on `counts` instead
struct DlStage {
  const char* who;
  hipStream_t st;
  AucBufs& b;
  int n;
  const float *L, *SA, *SB;
  int ldl, lda, ldb;
  const int64_t* idx;
  int rows, g;

  int* flags = nullptr;
  uint64_t* counts = nullptr;          // [g]; the offsets after pool()
  uint8_t* extra = nullptr;
  uint32_t* deg = nullptr;
  uint64_t P = 0, N = 0;
  size_t P4 = 0, H4 = 0;
  SortScratch sort;
  std::vector<uint64_t> h;

  int start(size_t extra_bytes, ptrdiff_t deg_at = -1);
  int counted();
  int pool(size_t p4, size_t h4, Carver& c, const char* what = "positives");
  int emit(uint32_t* ka, uint32_t* second);
};

// ---- device side
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

// The samples smp[q] = S[q stride], q < ns, of the np ascending keys S that a block stages in LDS (at most DL_STAGE of them;
// np == 0: none).  The caller's barrier publishes them.
struct DlSamples { uint32_t stride, ns; };
__device__ __forceinline__ DlSamples dl_stage(const uint32_t* __restrict__ S, uint32_t np, uint32_t* smp) {
  DlSamples s{1u, 0u};
  if (np) {
    s.stride = (np + DL_STAGE - 1) / DL_STAGE;
    s.ns = (np + s.stride - 1) / s.stride;
    for (uint32_t q = threadIdx.x; q < s.ns; q += AUC_THREADS) smp[q] = S[(uint64_t)q * s.stride];
  }
  return s;
}

// A segment [lo, hi) of S and the samples whose positions lie in it, q in [qlo, qhi)
struct DlSeg { uint32_t lo, hi, qlo, qhi; };
__device__ __forceinline__ DlSeg dl_all(uint32_t np, DlSamples s) { return {0u, np, 0u, s.ns}; }
__device__ __forceinline__ DlSeg dl_segment(uint32_t lo, uint32_t hi, uint32_t stride) {
  return {lo, hi, (lo + stride - 1) / stride, (hi + stride - 1) / stride};
}

// rank_bound over the segment g of the ascending keys S through the samples: c = the first sample of the segment >= x (> x).
// Position (c - 1) stride is below (at or below) x when c > qlo, position c stride is not when c < qhi; the bound lies between
// them, or between them and the segment's ends.
template <bool UPPER>
__device__ __forceinline__ uint32_t dl_find(const uint32_t* __restrict__ S, const uint32_t* smp, uint32_t stride, DlSeg g,
                                            uint32_t x) {
  const uint32_t c = rank_bound<UPPER>(smp, g.qlo, g.qhi, x);
  const uint32_t slo = c > g.qlo ? (c - 1) * stride + 1 : g.lo, shi = c < g.qhi ? c * stride : g.hi;
  return rank_bound<UPPER>(S, slo, shi, x);
}

// The placement of a candidate of key x against the positives of the segment: 2 #{above x} + #{equal to x} = 2 (hi - lo) -
// (lb - lo) - (ub - lo) <= 2 np < 2^32; lb = the first position at or above x, tie = whether that one equals x.
__device__ __forceinline__ uint32_t dl_placement(const uint32_t* __restrict__ S, const uint32_t* smp, uint32_t stride, DlSeg g,
                                                 uint32_t x, uint32_t& lb, bool& tie) {
  lb = dl_find<false>(S, smp, stride, g, x);
  tie = lb < g.hi && S[lb] == x;
  const uint32_t ub = tie ? dl_find<true>(S, smp, stride, g, x) : lb;
  return 2u * (g.hi - g.lo) - (lb - g.lo) - (ub - g.lo);
}
__device__ __forceinline__ uint32_t dl_placement(const uint32_t* __restrict__ S, const uint32_t* smp, uint32_t stride, DlSeg g,
                                                 uint32_t x) {
  uint32_t lb;
  bool tie;
  return dl_placement(S, smp, stride, g, x, lb, tie);
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

// one scoring's share of a negative: its placement among the sorted positives and the two counts
__device__ __forceinline__ uint32_t dl_negative(const DlSide& s, uint32_t np, const uint32_t* smp, DlSamples sm, float score,
                                                bool neg) {
  uint32_t lb = 0, b = 0;
  bool tie = false;
  if (neg) b = dl_placement(s.sorted, smp, sm.stride, dl_all(np, sm), auc_key(score), lb, tie);
  dl_hist_add(s.hist, lb, neg);
  dl_hist_add(s.ties, lb, tie);
  return b;                          // (0 for a positive: the callers use it under `neg`)
}

// one scoring's share of the positive at `slot`: a = 2 (negatives at or below it) - (negatives equal to it)
__device__ __forceinline__ uint64_t dl_positive(const DlSide& s, uint32_t np, uint64_t slot) {
  const uint32_t l = rank_bound<false>(s.sorted, 0u, np, s.slot[slot]);      // its own key is there: l < np
  return 2 * (s.cum[l] + s.hist[l]) - s.ties[l];                          // <= 2 N < 2^32
}

}  // namespace
}  // namespace mcgra
