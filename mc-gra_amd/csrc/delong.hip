// How far the AUC of the recovered graph can be trusted: the integers of DeLong's variance of the AUC (mcgra_auc_delong) and
// of DeLong's covariance of the AUCs of two scorings of the same pairs (mcgra_auc_delong_paired).  DeLong, DeLong and
// Clarke-Pearson, "Comparing the areas under two or more correlated receiver operating characteristic curves", Biometrics 44
// (1988).
//
// Candidates: those of mcgra_topk_metrics (topk.hip) -- the m = n_idx (n_idx - 1) / 2 unordered pairs of positions a > b of a
// repeat-free idx, score scores[idx[a]][idx[b]], label labels[idx[a]][idx[b]]; nothing outside the selected strict lower
// triangle is looked at.  NOT the population of mcgra_roc_auc (auc.hip), which ranges over the ordered entries with the
// diagonal: there each pair appears twice and a variance over it would be too small by about two.  The AUC these integers
// give, T / (2 P N), is the AUC of the unordered pairs.
// Scores compare as float32 values through the order-preserving key (rank_common.h): -0.0 == +0.0, subnormals and negative
// scores are ordinary values, ties are float32 equality.
// Placements, P positives and N negatives:
//   positive i:  a_i = 2 #{neg: s < s_i} + #{neg: s == s_i}  in [0, 2N]
//   negative j:  b_j = 2 #{pos: s > s_j} + #{pos: s == s_j}  in [0, 2P]
//   T = sum a_i (= sum b_j = 2U),  A2 = sum a_i^2,  B2 = sum b_j^2,  and for two scorings A, B of the same pairs
//   A_ab = sum a_i^A a_i^B,  B_ab = sum b_j^A b_j^B.
// m < 2^31, so a placement fits 32 bits and a product of two 64; a sum of products is below 2^95.
//
// Only the POSITIVES are stored and sorted (a graph has few edges among its pairs); the negatives are streamed from the
// matrices and never stored.  Passes:
//   rank_check_idx     idx only: range check, repeats (rank_common.hip)
//   k_dl_classify      (DlStage of delong_common.hip, as k_dl_emit) one read of the selected lower triangle: the argument
//                      checks (both score matrices), per-block positive counts
//   k_dl_emit          a second read of the labels: each positive's key (paired: of both matrices) to its slot, at per-block
//                      offsets (the host's scan of the counts).  Which slot of its block's range a positive takes depends on
//                      the order the waves run in; every result below is a sum over slots, which no such order changes.  The
//                      slot pairs the two scorings of a positive
//   auc_sort           a sorted copy of each scoring's positive keys (the stable LSD radix sort of rank_common.h)
//   k_dl_negatives     a third read: every negative x finds lb = #positives below x and ub = #positives at or below x in the
//                      sorted positives -- first in DL_STAGE evenly spaced samples of them staged in LDS, then inside the one
//                      stretch between two samples -- and that is its placement, b = 2 P - lb - ub, for both scorings at once:
//                      sum b, the halves of b^2 and of b^A b^B.  It also counts itself into hist[lb] and, when it ties a
//                      positive, into ties[lb] (32-bit integer atomics; the lanes of a wave that share a bin add once)
//   rank_scan          the running sum of hist
//   k_dl_positives     every positive slot: l = the first sorted position of its own key; the negatives at or below it are
//                      cum = hist[0] + ... + hist[l], those equal to it ties[l], so a = 2 cum - ties[l]; sum a, the halves of
//                      a^2 and of a^A a^B
// Each product is added as its low and its high 32-bit half into two 64-bit sums, each below 2^31 2^32 = 2^63; they are
// combined on the host side of the entry (unsigned 128-bit) and leave as (low, high) 64-bit limbs.
// There is no floating-point arithmetic on the device; everything is integer counts merged by integer atomics, so every call
// returns the same bits.
// Device scratch: 24 bytes per POSITIVE and scoring (its key by slot, the sorted copy, hist, ties and the 8-byte running sum)
// plus 4 for the sort's second buffer, about 3 MB for the sort's counts, and 4 bytes per node of the graph when idx is given:
// nothing per candidate.
// DlSide, the staged samples, the searches, the histogram add and the two placements are in delong_common.h, the positives'
// stage in delong_common.hip; node_jackknife.hip, hop_auc.hip and class_auc.hip share them.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/mcgra.h"
#include "common.h"
#include "delong_common.h"
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int DL_ROW_BLOCKS = 1024;        // blocks of the three passes over the matrix (grid-stride over selected rows)
constexpr int DL_POS_BLOCKS = 2048;        // at most this many blocks of the pass over the positives (grid-stride)

// slots of the accumulators, per class
enum { DL_T_A = 0, DL_T_B, DL_SQ_A_LO, DL_SQ_A_HI, DL_SQ_B_LO, DL_SQ_B_HI, DL_X_LO, DL_X_HI, DL_ACC };

// The negatives, streamed: acc[DL_T_A / _B] += b, acc[DL_SQ_*] += the halves of b^2, acc[DL_X_*] += the halves of b^A b^B
// (sb.S != NULL), and the counts hist / ties of each scoring.
__global__ __launch_bounds__(AUC_THREADS) void k_dl_negatives(int rows, DlSide sa, DlSide sb, const float* __restrict__ L,
                                                              int64_t ldl, const int64_t* __restrict__ idx, uint32_t np,
                                                              unsigned long long* __restrict__ acc) {
  __shared__ uint32_t smp_a[DL_STAGE], smp_b[DL_STAGE];
  __shared__ uint64_t sh[AUC_THREADS / 64];
  const bool paired = sb.S != nullptr;
  const DlSamples sm = dl_stage(sa.sorted, np, smp_a);
  if (paired) dl_stage(sb.sorted, np, smp_b);
  __syncthreads();
  uint64_t part[DL_ACC] = {};
  tri_for_each(rows, idx, [&](int, int, int64_t u, int64_t v) {
    const float xa = sa.S[u * sa.ld + v], xb = paired ? sb.S[u * sb.ld + v] : 0.f;
    const bool neg = !auc_pos(L[u * ldl + v]);                 // the labels were checked: 0 or 1
    const uint64_t ba = dl_negative(sa, np, smp_a, sm, xa, neg);
    const uint64_t bb = paired ? dl_negative(sb, np, smp_b, sm, xb, neg) : 0;
    if (neg) {
      const uint64_t qa = ba * ba, qb = bb * bb, qx = ba * bb;
      part[DL_T_A] += ba;
      part[DL_T_B] += bb;
      part[DL_SQ_A_LO] += qa & 0xffffffffull;
      part[DL_SQ_A_HI] += qa >> 32;
      part[DL_SQ_B_LO] += qb & 0xffffffffull;
      part[DL_SQ_B_HI] += qb >> 32;
      part[DL_X_LO] += qx & 0xffffffffull;
      part[DL_X_HI] += qx >> 32;
    }
  });
  block_add_u64(part, sh, acc);
}

// The positives, by slot: acc[DL_T_A / _B] += a, acc[DL_SQ_*] += the halves of a^2, acc[DL_X_*] += the halves of a^A a^B
__global__ __launch_bounds__(AUC_THREADS) void k_dl_positives(DlSide sa, DlSide sb, uint32_t np,
                                                              unsigned long long* __restrict__ acc) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  const bool paired = sb.S != nullptr;
  uint64_t part[DL_ACC] = {};
  for (uint64_t i = (uint64_t)blockIdx.x * AUC_THREADS + threadIdx.x; i < np; i += (uint64_t)gridDim.x * AUC_THREADS) {
    const uint64_t aa = dl_positive(sa, np, i), ab = paired ? dl_positive(sb, np, i) : 0;
    const uint64_t qa = aa * aa, qb = ab * ab, qx = aa * ab;
    part[DL_T_A] += aa;
    part[DL_T_B] += ab;
    part[DL_SQ_A_LO] += qa & 0xffffffffull;
    part[DL_SQ_A_HI] += qa >> 32;
    part[DL_SQ_B_LO] += qb & 0xffffffffull;
    part[DL_SQ_B_HI] += qb >> 32;
    part[DL_X_LO] += qx & 0xffffffffull;
    part[DL_X_HI] += qx >> 32;
  }
  block_add_u64(part, sh, acc);
}

// (low, high) limbs of lo + hi 2^32
void dl_limbs(uint64_t lo, uint64_t hi, uint64_t* out) {
  typedef unsigned __int128 u128;
  const u128 x = (u128)lo + ((u128)hi << 32);
  out[0] = (uint64_t)x;
  out[1] = (uint64_t)(x >> 64);
}

// Both entries: m, P, N, then per scoring T, A2 (2 limbs), B2 (2 limbs), then (paired) A_ab, B_ab (2 limbs each).
struct DlResult {
  uint64_t m = 0, P = 0, N = 0;
  uint64_t T[2] = {0, 0}, A2[2][2] = {}, B2[2][2] = {}, Aab[2] = {0, 0}, Bab[2] = {0, 0};
};

int dl_run(const char* who, hipStream_t st, int n, const float* L, int ldl, const float* SA, int lda, const float* SB, int ldb,
           const int64_t* idx, int rows, DlResult& r) {
  AucBufs b;
  const int sides = SB ? 2 : 1;
  DlStage stage{who, st, b, n, L, SA, SB, ldl, lda, ldb, idx, rows, std::min(rows - 1, DL_ROW_BLOCKS)};
  typedef unsigned long long Acc[2][DL_ACC];            // the two classes' accumulators
  if (int rc = stage.start(sizeof(Acc))) return rc;
  if (int rc = stage.counted()) return rc;
  Acc& acc = *(Acc*)stage.extra;
  const uint64_t P = r.P = stage.P;
  r.N = stage.N;
  r.m = P + r.N;
  if (P == 0 || r.N == 0) return 0;                    // every placement is 0
  // per scoring cum, slot, sorted, hist, ties; then the sort's second buffer
  const size_t P4 = stage.P4, H4 = stage.H4;
  Carver c{};
  if (int rc = stage.pool(sides * 2 + 1, sides * 4, c)) return rc;
  DlSide side[2] = {};
  for (int s = 0; s < sides; ++s) {
    side[s].S = s ? SB : SA;
    side[s].ld = s ? ldb : lda;
    side[s].cum = c.take<uint64_t>(H4);
    side[s].slot = c.take<uint32_t>(P4);
    side[s].sorted = c.take<uint32_t>(P4);
    side[s].hist = c.take<uint32_t>(H4);
    side[s].ties = c.take<uint32_t>(H4);
  }
  uint32_t* tmp = c.take<uint32_t>(P4);
  if (int rc = stage.emit(side[0].slot, side[1].slot)) return rc;
  for (int s = 0; s < sides; ++s) {
    MCGRA_HIP(hipMemcpyAsync(side[s].sorted, side[s].slot, sizeof(uint32_t) * P, hipMemcpyDeviceToDevice, st));
    if (int rc = auc_sort(st, side[s].sorted, tmp, P, stage.sort)) return rc;
    MCGRA_HIP(hipMemsetAsync(side[s].hist, 0, sizeof(uint32_t) * 2 * H4, st));          // hist and ties are adjacent
  }
  k_dl_negatives<<<stage.g, AUC_THREADS, 0, st>>>(rows, side[0], side[1], L, ldl, idx, (uint32_t)P, acc[1]);
  MCGRA_KERNEL_CHECK();
  for (int s = 0; s < sides; ++s) rank_scan(st, side[s].hist, (int)P, side[s].cum);
  const int gp = (int)std::min<uint64_t>(DL_POS_BLOCKS, (P + AUC_THREADS - 1) / AUC_THREADS);
  k_dl_positives<<<gp, AUC_THREADS, 0, st>>>(side[0], side[1], (uint32_t)P, acc[0]);
  MCGRA_KERNEL_CHECK();
  unsigned long long ha[2][DL_ACC];
  MCGRA_HIP(hipMemcpyAsync(ha, acc, sizeof(ha), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));                  // also: the scratch is freed on return
  const unsigned long long *ap = ha[0], *an = ha[1];
  if (ap[DL_T_A] != an[DL_T_A] || ap[DL_T_B] != an[DL_T_B]) {             // sum a_i == sum b_j == 2U by construction
    set_error("%s: internal error: the two placement sums differ (%llu, %llu; %llu, %llu)", who, ap[DL_T_A], an[DL_T_A],
              ap[DL_T_B], an[DL_T_B]);
    return MCGRA_EHIP;
  }
  r.T[0] = ap[DL_T_A];
  r.T[1] = ap[DL_T_B];
  dl_limbs(ap[DL_SQ_A_LO], ap[DL_SQ_A_HI], r.A2[0]);
  dl_limbs(an[DL_SQ_A_LO], an[DL_SQ_A_HI], r.B2[0]);
  dl_limbs(ap[DL_SQ_B_LO], ap[DL_SQ_B_HI], r.A2[1]);
  dl_limbs(an[DL_SQ_B_LO], an[DL_SQ_B_HI], r.B2[1]);
  dl_limbs(ap[DL_X_LO], ap[DL_X_HI], r.Aab);
  dl_limbs(an[DL_X_LO], an[DL_X_HI], r.Bab);
  return 0;
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_auc_delong(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                                const int64_t* idx, int64_t n_idx, uint64_t* out) {
  if (!out) { set_error("auc_delong: bad argument (out NULL)"); return MCGRA_EINVAL; }
  if (int rc = rank_check_args("auc_delong", n, {{labels, ld_labels, true}, {scores, ld_scores, true}}, idx, n_idx, 2)) return rc;
  DlResult r;
  if (int rc = dl_run("auc_delong", (hipStream_t)stream, n, labels, ld_labels, scores, ld_scores, nullptr, 0, idx, (int)n_idx, r))
    return rc;
  const uint64_t res[8] = {r.m, r.P, r.N, r.T[0], r.A2[0][0], r.A2[0][1], r.B2[0][0], r.B2[0][1]};
  memcpy(out, res, sizeof(res));
  return 0;
}

extern "C" int mcgra_auc_delong_paired(void* stream, int n, const float* labels, int ld_labels, const float* scores_a, int ld_a,
                                       const float* scores_b, int ld_b, const int64_t* idx, int64_t n_idx, uint64_t* out) {
  if (!out) { set_error("auc_delong_paired: bad argument (out NULL)"); return MCGRA_EINVAL; }
  if (int rc = rank_check_args("auc_delong_paired", n, {{labels, ld_labels, true}, {scores_a, ld_a, true}, {scores_b, ld_b, true}}, idx,
                               n_idx, 2))
    return rc;
  DlResult r;
  if (int rc = dl_run("auc_delong_paired", (hipStream_t)stream, n, labels, ld_labels, scores_a, ld_a, scores_b, ld_b, idx,
                      (int)n_idx, r))
    return rc;
  const uint64_t res[17] = {r.m, r.P, r.N, r.T[0], r.T[1], r.A2[0][0], r.A2[0][1], r.B2[0][0], r.B2[0][1],
                            r.A2[1][0], r.A2[1][1], r.B2[1][0], r.B2[1][1], r.Aab[0], r.Aab[1], r.Bab[0], r.Bab[1]};
  memcpy(out, res, sizeof(res));
  return 0;
}
