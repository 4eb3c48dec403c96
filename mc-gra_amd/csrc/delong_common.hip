// The positives' stage of the placement entries (DlStage, declared in delong_common.h) and its kernels, compiled here and
// nowhere else:
//   k_dl_classify<NODES>  one read of the selected lower triangle: the argument checks, per-block positive counts (NODES: and
//                         the positives per position)
//   k_dl_emit<NODES>      a second read of the labels: each positive's key to a slot of its block's range, with (NODES) its
//                         endpoints or the key of a second scoring
#include "delong_common.h"

#include <algorithm>

namespace mcgra {

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

int DlStage::start(size_t extra_bytes, ptrdiff_t deg_at) {
  const size_t fixed = sizeof(uint64_t) * (1 + (size_t)g);          // the flag word (and its pad), the counts
  uint8_t* head = b.get<uint8_t>(fixed + extra_bytes);
  if (!head) { set_error("%s: hipMalloc failed", who); return MCGRA_ENOMEM; }
  flags = (int*)head;
  counts = (uint64_t*)head + 1;
  extra = head + fixed;
  deg = deg_at < 0 ? nullptr : (uint32_t*)(extra + deg_at);
  MCGRA_HIP(hipMemsetAsync(head, 0, fixed + extra_bytes, st));
  if (int rc = rank_check_idx(who, st, b, n, idx, rows, flags)) return rc;
  if (deg) k_dl_classify<true><<<g, AUC_THREADS, 0, st>>>(rows, SA, lda, SB, ldb, L, ldl, idx, counts, deg, flags);
  else k_dl_classify<false><<<g, AUC_THREADS, 0, st>>>(rows, SA, lda, SB, ldb, L, ldl, idx, counts, nullptr, flags);
  MCGRA_KERNEL_CHECK();
  return 0;
}

int DlStage::counted() {
  h.resize(g);
  int h_flags = 0;
  MCGRA_HIP(hipMemcpyAsync(h.data(), counts, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (int rc = rank_flag_error(who, h_flags, SB != nullptr)) return rc;
  P = 0;
  for (int i = 0; i < g; ++i) { const uint64_t p = h[i]; h[i] = P; P += p; }        // counts -> offsets
  N = (uint64_t)rows * (rows - 1) / 2 - P;
  P4 = (P + 3) / 4 * 4;
  H4 = P4 + 4;
  return 0;
}

int DlStage::pool(size_t p4, size_t h4, Carver& c, const char* what) {
  const size_t bytes = SortScratch::BYTES + sizeof(uint32_t) * (p4 * P4 + h4 * H4);
  uint8_t* q = b.get<uint8_t>(bytes);
  if (!q) { set_error("%s: hipMalloc of the scratch of %llu %s failed", who, (unsigned long long)P, what); return MCGRA_ENOMEM; }
  c = Carver{q, bytes};
  sort = SortScratch(c);
  MCGRA_HIP(hipMemcpyAsync(counts, h.data(), sizeof(uint64_t) * h.size(), hipMemcpyHostToDevice, st));
  return 0;
}

int DlStage::emit(uint32_t* ka, uint32_t* second) {
  if (deg) k_dl_emit<true><<<g, AUC_THREADS, 0, st>>>(rows, SA, lda, SB, ldb, L, ldl, idx, counts, ka, second);
  else k_dl_emit<false><<<g, AUC_THREADS, 0, st>>>(rows, SA, lda, SB, ldb, L, ldl, idx, counts, ka, second);
  MCGRA_KERNEL_CHECK();
  return 0;
}

}  // namespace mcgra
