// What the entries that rank every selected pair through the two sorted key regions share (auc.hip: mcgra_roc_auc,
// mcgra_rank_metrics, mcgra_rank_curves, mcgra_decode_auc, mcgra_decode_rank_metrics; pair_distance.hip:
// mcgra_pair_distance_rank_metrics).  Device side, inlined into each file's kernels: the bodies of the classify and the emit
// pass over one selected entry.  Host side, defined once in auc.hip beside its kernels (k_auc_pairs, k_ap_terms, k_ap_sum):
// AucRun, the scratch, the checks and everything behind the classify pass.
#pragma once
#include <functional>

#include "rank_common.h"
#include "curves.h"

namespace mcgra {
constexpr int AUC_ROW_BLOCKS = 1024;       // at most this many blocks in a classify / emit pass (their counts: 2 per block)

// emit(offs, keys) launches the emit pass: block b's positives to keys[offs[2 b] ..), its negatives to keys[offs[2 b + 1] ..)
using AucEmit = std::function<void(const uint64_t* offs, uint32_t* keys)>;

struct AucRun {
  const char* who;
  hipStream_t st;
  AucBufs b;
  int* flags = nullptr;
  uint64_t* counts = nullptr;
  unsigned long long* acc = nullptr;
  int h_flags = 0;

  int begin();
  // idx != NULL: range check and repeats; a permutation of all nodes becomes idx = NULL (the same multiset)
  int select(int n, const int64_t*& idx, int64_t n_idx);
  // Behind the classify pass of g blocks: its counts and flags, the per-block offsets, the emit pass (emit(offs, keys)
  // launches it), the two sorts, then what was asked for: auc != NULL the pair count and the division, ap != NULL the
  // average-precision terms and their sum (both read the same sorted regions); cv != NULL (then auc == ap == NULL) the
  // curves of curves.hip, which also take a single-class selection.  pnt != NULL (host[3]): {P, N, 2U}, 2U counted when
  // auc != NULL and both classes are present, else 0.
  int finish(int g, const AucEmit& emit, double* auc, double* ap, const CurveRequest* cv = nullptr, uint64_t* pnt = nullptr);
};

namespace {
// one selected entry of the classify pass: the argument checks and the counts of positives and of all entries
__device__ __forceinline__ void auc_classify_one(float s, float l, uint32_t& pos, uint32_t& tot, int& f) {
  if (!auc_finite(s)) f |= AUC_BAD_SCORE;
  if (auc_pos(l)) ++pos;
  else if (!auc_neg(l)) f |= AUC_BAD_LABEL;   // also NaN
  ++tot;
}
// what the classify pass leaves: counts[2 b] / counts[2 b + 1] = positives / negatives of block b, flags |= f
__device__ __forceinline__ void auc_classify_end(uint32_t pos, uint32_t tot, int f, uint64_t* sh, uint64_t* __restrict__ counts,
                                                 int* __restrict__ flags) {
  if (f) atomicOr(flags, f);
  const uint64_t p = block_sum_u64(pos, sh);
  __syncthreads();
  const uint64_t t = block_sum_u64(tot, sh);
  if (threadIdx.x == 0) { counts[2 * blockIdx.x] = p; counts[2 * blockIdx.x + 1] = t - p; }
}
// one selected entry of the emit pass: its key behind the block's positives (cur[0]) or negatives (cur[1]) so far.  Not two
// calls of wave_slot: every lane takes a slot here, and one leader that advances both cursors in one go keeps the two LDS
// round trips of a step overlapped, as they were.
__device__ __forceinline__ void auc_emit_one(float s, float l, uint64_t o_pos, uint64_t o_neg, uint32_t* cur,
                                             uint32_t* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const uint64_t below = (1ull << lane) - 1ull;
  const bool p = auc_pos(l);
  const uint64_t act = __ballot(1), mp = __ballot(p);
  const int leader = __ffsll((unsigned long long)act) - 1;
  uint32_t bp = 0, bn = 0;
  if (lane == leader) {
    bp = atomicAdd(&cur[0], (uint32_t)__popcll(mp));
    bn = atomicAdd(&cur[1], (uint32_t)__popcll(act & ~mp));
  }
  bp = __shfl(bp, leader, 64);
  bn = __shfl(bn, leader, 64);
  keys[p ? o_pos + bp + __popcll(mp & below) : o_neg + bn + __popcll(act & ~mp & below)] = auc_key(s);
}
}  // namespace
}  // namespace mcgra
