// Which summand carries the ensemble: the AUC integers of up to 255 subset sums of up to eight n x n components in one pass over
// the pairs (mcgra_subset_auc).
//
// Candidates, selection, label checks and idx rules: those of mcgra_auc_delong (delong.hip) -- the m = n_idx (n_idx - 1) / 2
// unordered pairs of positions a > b of a repeat-free idx; every component is read at [idx[a]][idx[b]] only.
// The score of a pair under mask M is the float32 sum of its components k in M in ascending k, s = c_first; s = s + c_next; ...
// (plain adds: there is nothing to contract or reassociate); T_s is mcgra_auc_delong's T on that sum.
// The walk list (host): the masks asked for, without repeats, closed under "mask -> mask without its top bit", as the
// depth-first walk of that tree from the empty mask.  A step {depth d, component k, emit as unique mask u or not} sets
// stack[d] = d == 1 ? c_k : stack[d - 1] + c_k: stack[d - 1] is the parent's sum, so every sum costs one add and comes out in
// ascending-k order.  The list is the same for every lane (it sits in LDS), the stack is eight registers.
// Passes:
//   DlStage       (delong_common.hip) rank_check_idx; k_dl_classify on component 0: the label checks, per-block counts of the edges
//   k_sa_emit     a second read of the labels: an edge at slot t walks the list and writes the key of its sum under unique mask u to
//                 keys[u P + t], with u beside it
//   auc_sort      by key, u as payload; then ONE more stable pass by u's eight bits: segment u = [u P, (u + 1) P) ascending
//   k_sa_stream   ONE pass over the selected strict lower triangle, row by row (coalesced along b).  A block stages the list, and
//                 for every unique mask the same number of samples of its segment (SA_SMP_WORDS words of LDS shared out evenly:
//                 8192 / U samples a mask, at most DL_STAGE).  A non-edge loads its K values once, walks the list and places each
//                 emitted sum inside that mask's segment (dl_placement through the mask's samples).  The list is wave-uniform, so
//                 the 64 placements of a step belong to ONE mask: they are summed over the wave and added once to the block's
//                 64-bit counter of the mask in LDS; at the end one 64-bit atomic per non-zero mask and block.
// Both passes flag a selected component value or a sum of the list that is NaN or +-inf (an inner sum of the list is an ancestor
// of a mask asked for, whose sum is then not finite either).
// Integer work apart from the adds: the same bits on every call and under any permutation of idx.  T of a repeated mask is
// copied on the host.
// Device scratch: 16 bytes per edge and unique mask, about 3 MB for the sort's counts, 8 bytes per block, and 4 bytes per node
// of the graph when idx is given.
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
constexpr int SA_ROW_BLOCKS = 1024;                  // blocks of the passes over the selected rows (grid-stride)
constexpr int SA_K = MCGRA_SUBSET_MAX_K;             // components
constexpr int SA_MASKS = MCGRA_SUBSET_MAX_MASKS;     // masks of a call = the non-zero masks of SA_K components
constexpr int SA_STEPS = 256;                        // the closure holds non-zero masks below 2^SA_K: at most 255 steps
constexpr int SA_SMP_WORDS = 8192;                   // 32 KB of LDS for the samples of all segments
constexpr uint32_t SA_EMIT = 0x100u;                 // a step: depth | k << 4 | SA_EMIT | u << 16
static_assert(SA_MASKS == (1 << SA_K) - 1 && SA_MASKS < SA_STEPS && SA_MASKS <= 256, "u is one digit of the sort");
static_assert(SA_SMP_WORDS / SA_MASKS >= 2, "every segment keeps samples");

struct SaComps { const float* p[SA_K]; };

// what follows the stage's counts on the device
struct SaHead {
  unsigned long long acc[SA_MASKS + 1];
  int flags, pad;
  uint32_t steps[SA_STEPS];
};

// the K values of one pair (the rest 0); whether all are finite
__device__ __forceinline__ bool sa_load(const SaComps& C, int K, int64_t at, float (&c)[SA_K]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < SA_K; ++k) {
    c[k] = 0.f;
    if (k < K) { c[k] = C.p[k][at]; ok = ok && auc_finite(c[k]); }
  }
  return ok;
}

// The walk: emit(u, sum) for every emitting step; false when a sum of the list is not finite.  Depth and component are the same
// in every lane, so the selects below are scalar compares.
template <class F>
__device__ __forceinline__ bool sa_walk(const uint32_t* steps, int n_steps, const float (&c)[SA_K], F&& emit) {
  float s[SA_K];
#pragma unroll
  for (int j = 0; j < SA_K; ++j) s[j] = 0.f;
  bool ok = true;
  for (int q = 0; q < n_steps; ++q) {
    const uint32_t w = steps[q];
    const int d = (int)(w & 15u), k = (int)((w >> 4) & 15u);
    float ck = c[0], par = 0.f;
#pragma unroll
    for (int j = 1; j < SA_K; ++j) ck = k == j ? c[j] : ck;
#pragma unroll
    for (int j = 1; j < SA_K; ++j) par = d == j + 1 ? s[j - 1] : par;      // the parent's sum, at depth d - 1
    const float v = d == 1 ? ck : __fadd_rn(par, ck);
#pragma unroll
    for (int j = 0; j < SA_K; ++j) s[j] = d == j + 1 ? v : s[j];
    ok = ok && auc_finite(v);
    if (w & SA_EMIT) emit(w >> 16, v);
  }
  return ok;
}

// k_dl_emit for the sums: the edge at slot t writes keys[u P + t] = the key of its sum under unique mask u, which[..] = u
__global__ __launch_bounds__(AUC_THREADS) void k_sa_emit(int rows, int K, SaComps C, int64_t ldc, const float* __restrict__ L,
                                                         int64_t ldl, const int64_t* __restrict__ idx,
                                                         const uint64_t* __restrict__ offs, const uint32_t* __restrict__ steps_g,
                                                         int n_steps, uint64_t P, uint32_t* __restrict__ keys,
                                                         uint32_t* __restrict__ which, int* __restrict__ flags) {
  __shared__ uint32_t cur;
  __shared__ uint32_t steps[SA_STEPS];
  if (threadIdx.x == 0) cur = 0;
  for (int q = threadIdx.x; q < n_steps; q += AUC_THREADS) steps[q] = steps_g[q];
  __syncthreads();
  const uint64_t o_pos = offs[blockIdx.x];
  bool ok = true;
  tri_for_each(rows, idx, [&](int, int, int64_t u, int64_t v) {
    const bool p = auc_pos(L[u * ldl + v]);
    const uint64_t at = o_pos + wave_slot(p, &cur);
    if (!p) return;
    float c[SA_K];
    ok = sa_load(C, K, u * ldc + v, c) && ok;
    ok = sa_walk(steps, n_steps, c, [&](uint32_t m, float sum) {
      keys[(uint64_t)m * P + at] = auc_key(sum);
      which[(uint64_t)m * P + at] = m;
    }) && ok;
  });
  if (!ok) atomicOr(flags, AUC_BAD_SCORE);
}

// The non-edges, streamed: acc[u] += the placements of their sums under unique mask u among the np edges' sums under u,
// sorted[u np .. (u + 1) np) ascending.  spm: samples a segment may keep in LDS (U spm <= SA_SMP_WORDS).
__global__ __launch_bounds__(AUC_THREADS) void k_sa_stream(int rows, int K, SaComps C, int64_t ldc, const float* __restrict__ L,
                                                           int64_t ldl, const int64_t* __restrict__ idx,
                                                           const uint32_t* __restrict__ sorted, uint32_t np, int U, uint32_t spm,
                                                           const uint32_t* __restrict__ steps_g, int n_steps,
                                                           unsigned long long* __restrict__ acc, int* __restrict__ flags) {
  __shared__ uint32_t smp[SA_SMP_WORDS];
  __shared__ unsigned long long tsum[SA_MASKS + 1];
  __shared__ uint32_t steps[SA_STEPS];
  const uint32_t stride = np ? (np + spm - 1) / spm : 1u, ns = np ? (np + stride - 1) / stride : 0u;      // ns <= spm
  for (uint32_t q = threadIdx.x; q < (uint32_t)U * ns; q += AUC_THREADS)
    smp[q] = sorted[(uint64_t)(q / ns) * np + (uint64_t)(q % ns) * stride];
  for (int q = threadIdx.x; q < U; q += AUC_THREADS) tsum[q] = 0;
  for (int q = threadIdx.x; q < n_steps; q += AUC_THREADS) steps[q] = steps_g[q];
  __syncthreads();
  const DlSeg seg{0u, np, 0u, ns};
  const int lane = threadIdx.x & 63;
  bool ok = true;
  for (int a = 1 + blockIdx.x; a < rows; a += gridDim.x) {
    const int64_t u = idx ? idx[a] : a;
    for (int b0 = 0; b0 < a; b0 += AUC_THREADS) {          // every lane stays in: a step's placements are summed over the wave
      const int b = b0 + (int)threadIdx.x;
      bool neg = false;
      float c[SA_K] = {};
      if (b < a) {
        const int64_t v = idx ? idx[b] : (int64_t)b;
        neg = !auc_pos(L[u * ldl + v]);                    // the labels were checked
        if (neg) ok = sa_load(C, K, u * ldc + v, c) && ok;
      }
      if (!__ballot(neg)) continue;                        // (the same in the whole wave)
      ok = sa_walk(steps, n_steps, c, [&](uint32_t m, float sum) {
        uint32_t bq = 0;                                   // <= 2 P < 2^32
        if (neg && np) bq = dl_placement(sorted + (uint64_t)m * np, smp + m * ns, stride, seg, auc_key(sum));
        const uint64_t t = wave_sum_u64(bq);
        if (lane == 0 && t) atomicAdd(&tsum[m], (unsigned long long)t);
      }) && ok;
    }
  }
  if (!ok) atomicOr(flags, AUC_BAD_SCORE);
  __syncthreads();
  for (int q = threadIdx.x; q < U; q += AUC_THREADS)
    if (tsum[q]) atomicAdd(&acc[q], tsum[q]);
}

// The walk list of the unique masks uniq (ascending) of K components: see the head of the file.  uid[M] = M's place in uniq or -1.
void sa_steps(int K, const int (&uid)[1 << SA_K], const bool (&clo)[1 << SA_K], unsigned M, int depth, int top,
              std::vector<uint32_t>& steps) {
  for (int j = top + 1; j < K; ++j) {
    const unsigned child = M | (1u << j);
    if (!clo[child]) continue;
    steps.push_back((uint32_t)(depth + 1) | (uint32_t)j << 4 | (uid[child] >= 0 ? SA_EMIT | (uint32_t)uid[child] << 16 : 0u));
    sa_steps(K, uid, clo, child, depth + 1, j, steps);
  }
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_subset_auc(void* stream, int n, const float* labels, int ld_labels, const float* const* comps, int K,
                                int ld_comps, const int64_t* idx, int64_t n_idx, const uint32_t* masks, int n_masks,
                                uint64_t* out) {
  const char* who = "subset_auc";
  if (!out || !comps || !masks) { set_error("%s: bad argument (out, comps or masks NULL)", who); return MCGRA_EINVAL; }
  if (K < 1 || K > SA_K || n_masks < 1 || n_masks > SA_MASKS) {
    set_error("%s: bad argument (K = %d, n_masks = %d; 1 to %d components, 1 to %d masks)", who, K, n_masks, SA_K, SA_MASKS);
    return MCGRA_EINVAL;
  }
  SaComps C{};
  for (int k = 0; k < K; ++k) {
    if (!comps[k]) { set_error("%s: bad argument (component %d is NULL)", who, k); return MCGRA_EINVAL; }
    C.p[k] = comps[k];
  }
  int uid[1 << SA_K];
  bool clo[1 << SA_K] = {};
  std::fill(uid, uid + (1 << SA_K), -1);
  for (int s = 0; s < n_masks; ++s) {
    if (masks[s] < 1u || masks[s] >= (1u << K)) {
      set_error("%s: bad argument (masks[%d] = %u; a mask of %d components lies in [1, %u))", who, s, masks[s], K, 1u << K);
      return MCGRA_EINVAL;
    }
    uid[masks[s]] = 0;
  }
  if (int rc = rank_check_args(who, n, {{labels, ld_labels, true}, {comps[0], ld_comps, true}}, idx, n_idx, 2)) return rc;
  int U = 0;
  for (unsigned M = 1; M < (1u << K); ++M) {
    if (uid[M] < 0) continue;
    uid[M] = U++;
    for (unsigned A = M; A; A &= ~(1u << (31 - __builtin_clz(A)))) clo[A] = true;      // M and its ancestors
  }
  std::vector<uint32_t> steps;
  sa_steps(K, uid, clo, 0u, 0, -1, steps);
  hipStream_t st = (hipStream_t)stream;
  const int m = (int)n_idx;
  AucBufs b;
  DlStage stage{who, st, b, n, labels, comps[0], nullptr, ld_labels, ld_comps, 0, idx, m, std::min(m - 1, SA_ROW_BLOCKS)};
  if (int rc = stage.start(sizeof(SaHead))) return rc;
  const int g = stage.g;
  SaHead* hd = (SaHead*)stage.extra;
  MCGRA_HIP(hipMemcpyAsync(hd->steps, steps.data(), sizeof(uint32_t) * steps.size(), hipMemcpyHostToDevice, st));
  if (int rc = stage.counted()) return rc;
  const uint64_t P = stage.P, N = stage.N, Q = P * (uint64_t)U;
  uint32_t* sorted = nullptr;
  if (P) {
    Carver c{};
    if (int rc = stage.pool(0, 0, c, "edges")) return rc;                  // the sort's scratch; the offsets replace the counts
    const size_t Q4 = (Q + 3) / 4 * 4, bytes = 4 * Carver::bytes<uint32_t>(Q4);
    uint8_t* q = b.get<uint8_t>(bytes);
    if (!q) {
      set_error("%s: hipMalloc of the scratch of %llu edges under %d masks failed", who, (unsigned long long)P, U);
      return MCGRA_ENOMEM;
    }
    Carver kc{q, bytes};
    uint32_t *ka = kc.take<uint32_t>(Q4), *kb = kc.take<uint32_t>(Q4), *wa = kc.take<uint32_t>(Q4), *wb = kc.take<uint32_t>(Q4);
    k_sa_emit<<<g, AUC_THREADS, 0, st>>>(m, K, C, ld_comps, labels, ld_labels, idx, stage.counts, hd->steps, (int)steps.size(), P,
                                         ka, wa, &hd->flags);
    MCGRA_KERNEL_CHECK();
    if (int rc = auc_sort(st, ka, kb, Q, stage.sort, wa, wb)) return rc;             // by key: back in ka, wa
    if (int rc = auc_sort(st, wa, wb, Q, stage.sort, ka, kb, 8)) return rc;          // one pass by mask: in wb, kb
    sorted = Q > 1 ? kb : ka;                                                        // (fewer than two keys: nothing moved)
  }
  const uint32_t spm = (uint32_t)std::min(DL_STAGE, SA_SMP_WORDS / U);
  k_sa_stream<<<g, AUC_THREADS, 0, st>>>(m, K, C, ld_comps, labels, ld_labels, idx, sorted, (uint32_t)P, U, spm, hd->steps,
                                         (int)steps.size(), hd->acc, &hd->flags);
  MCGRA_KERNEL_CHECK();
  std::vector<unsigned long long> T(U);
  int flags = 0;
  MCGRA_HIP(hipMemcpyAsync(T.data(), hd->acc, sizeof(unsigned long long) * T.size(), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipMemcpyAsync(&flags, &hd->flags, sizeof(int), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));                                  // the scratch is freed on return
  if (flags) {
    set_error("%s: a selected component value or subset sum is NaN or infinite", who);
    return MCGRA_EINVAL;
  }
  out[0] = P + N;
  out[1] = P;
  out[2] = N;
  for (int s = 0; s < n_masks; ++s) out[3 + s] = T[uid[masks[s]]];
  return 0;
}
