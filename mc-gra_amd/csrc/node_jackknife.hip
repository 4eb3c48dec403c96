// Which nodes carry the AUC of the recovered graph, and how far it can be trusted when nodes, not pairs, are the independent
// units: the integers of the delete-one-node jackknife of the AUC (mcgra_auc_node_jackknife).  Efron and Stein, "The jackknife
// estimate of variance", Ann. Statist. 9 (1981).
//
// Candidates, comparison and placements: those of mcgra_auc_delong (delong.hip) -- the m = n_idx (n_idx - 1) / 2 unordered pairs
// of positions a > b of a repeat-free idx, score scores[idx[a]][idx[b]], label labels[idx[a]][idx[b]], float32 values through
// auc_key, a tie counts 1/2.  With 2 psi(p, q) in {0, 1, 2} the doubled win of positive p over negative q,
//   a_p = sum_q 2 psi(p, q),  b_q = sum_p 2 psi(p, q),  T = sum a_p = sum b_q,
// position v of idx gets five integers over the pairs that contain v:
//   P_v, N_v   its positives and negatives (P_v + N_v = n_idx - 1)
//   A_v        sum of a_p over its positives            <= 2 P_v N < 2^17 2^31
//   B_v        sum of b_q over its negatives            <= 2 N_v P < 2^48
//   C_v        sum of 2 psi(p, q) over its positives p and its negatives q   <= 2 P_v N_v < 2^33
// Deleting v leaves T - A_v - B_v + C_v (C_v is in both sums), P - P_v positives and N - N_v negatives.
//
// Only the positives are stored, as in delong.hip; the negatives are streamed.  Passes:
//   rank_check_idx     idx only: range check, repeats (rank_common.hip)
//   k_dl_classify      (DlStage of delong_common.hip, NODES) one read of the selected lower triangle: the argument checks,
//                      per-block positive counts, and P_v (deg[a] += 1, deg[b] += 1 per positive: 32-bit integer atomics)
//   k_dl_emit          (DlStage, NODES) a second read of the labels: each positive's key and its endpoints
//                      a << 16 | b to a slot of its block's range.  Which slot depends on the order the waves run in; the
//                      sort below ends that
//   auc_sort           the positives by key, the endpoints riding along.  Equal keys may keep either order of their endpoints:
//                      everything below is a sum over the positives of one key
//   k_nj_lists         every sorted positive i becomes two entries (node a, key) and (node b, key) at 2 i, 2 i + 1
//   auc_sort           the entries by node, stable, the keys riding along: node v's positives' keys, ascending, are
//                      lkey[noff[v] .. noff[v + 1]), noff the running sum of deg
//   k_nj_negatives     a third read.  Every negative x = (a, b) finds its placement b_q among all sorted positives (dl_negative:
//                      samples in LDS, hist / ties for the positives' pass) and its doubled wins lost to a's positives and to
//                      b's positives in the two nodes' lists (2 d - lb - ub in a list of d keys).  Row endpoint: the block that
//                      owns row a sums over its lanes and adds once per row and column chunk.  Column endpoint: a block works
//                      through the columns in chunks of NJ_COLS; lane t alone meets the columns c0 + t, c0 + t + 256, ... of a
//                      chunk in every row, so it keeps their sums in LDS without atomics and adds the non-zero ones to the
//                      node's sum when the chunk ends: global 64-bit atomics per (block, node), not per pair
//   rank_scan          the running sum of hist
//   k_nj_positives     every sorted positive: a_p as in delong.hip, added to both endpoints' A (64-bit atomics, two per positive)
//   k_nj_finish        P_v = deg[v], N_v = n_idx - 1 - deg[v]
// Everything is integer counts merged by integer adds: no floating-point arithmetic on the device, the same bits on every
// call.  The five columns are summed in scratch and copied to `out` when every check has passed.
// Device scratch: 40 bytes per selected node + 12 for deg and noff; per POSITIVE 32 bytes (key, endpoints, hist, ties and the
// 8-byte running sum, the sort's two second buffers) + 32 for the two list entries and their second buffers; about 3 MB for
// the sort's counts; 4 bytes per node of the graph when idx is given.  Nothing per candidate.
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
constexpr int NJ_ROW_BLOCKS = 512;         // blocks of the three passes over the matrix (grid-stride over selected rows)
constexpr int NJ_POS_BLOCKS = 1024;        // at most this many blocks of the passes over the positives (grid-stride)
constexpr int NJ_COLS = 2048;              // columns of one chunk of k_nj_negatives: 2 x 8 bytes of LDS each
static_assert(NJ_COLS % AUC_THREADS == 0, "a lane owns the same columns of every chunk");
static_assert(AUC_MAX_NIDX <= 0xffff, "a position fits 16 bits");
enum { NJ_P = 0, NJ_N, NJ_A, NJ_B, NJ_C, NJ_WORDS };     // the columns of out

// the two list entries of every sorted positive
__global__ __launch_bounds__(AUC_THREADS) void k_nj_lists(const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ ends,
                                                          uint32_t np, uint32_t* __restrict__ lnode, uint32_t* __restrict__ lkey) {
  for (uint64_t i = (uint64_t)blockIdx.x * AUC_THREADS + threadIdx.x; i < np; i += (uint64_t)gridDim.x * AUC_THREADS) {
    const uint32_t e = ends[i], k = sorted[i];
    lnode[2 * i] = e >> 16;
    lnode[2 * i + 1] = e & 0xffffu;
    lkey[2 * i] = k;
    lkey[2 * i + 1] = k;
  }
}

// the doubled wins of a node's d positives (keys ascending at `list`) over a negative of key x: 2 #{> x} + #{== x}
__device__ __forceinline__ uint32_t nj_lost(const uint32_t* __restrict__ list, uint32_t d, uint32_t x) {
  if (d == 0) return 0;
  const uint32_t lb = rank_bound<false>(list, 0u, d, x);
  const uint32_t ub = rank_bound<true>(list, lb, d, x);
  return 2u * d - lb - ub;
}

// (The walk below is not tri_for_each: the columns go in chunks of NJ_COLS with the rows inside and per-row block sums between
// them, which the walker's row-by-row order does not give.)
// The negatives, streamed: out[a][NJ_B] += b_q and out[b][NJ_B] += b_q, out[a][NJ_C] += q's losses to a's positives,
// out[b][NJ_C] += its losses to b's positives, *t_neg += b_q, and the counts hist / ties.
__global__ __launch_bounds__(AUC_THREADS) void k_nj_negatives(int rows, DlSide s, const float* __restrict__ L, int64_t ldl,
                                                              const int64_t* __restrict__ idx, uint32_t np,
                                                              const uint32_t* __restrict__ lkey, const uint64_t* __restrict__ noff,
                                                              unsigned long long* __restrict__ out,
                                                              unsigned long long* __restrict__ t_neg) {
  __shared__ uint32_t smp[DL_STAGE];
  __shared__ uint64_t col_b[NJ_COLS], col_c[NJ_COLS];
  __shared__ uint64_t sh_b[AUC_THREADS / 64], sh_c[AUC_THREADS / 64];
  const DlSamples sm = dl_stage(s.sorted, np, smp);
  __syncthreads();
  uint64_t total = 0;
  for (int c0 = 0; c0 + 1 < rows; c0 += NJ_COLS) {                 // column rows - 1 has no row above it
    for (int j = threadIdx.x; j < NJ_COLS; j += AUC_THREADS) { col_b[j] = 0; col_c[j] = 0; }   // this lane's own columns
    for (int a = 1 + blockIdx.x; a < rows; a += gridDim.x) {
      if (a <= c0) continue;                                        // the same in the whole block
      const int64_t u = idx ? idx[a] : a;
      const float* srow = s.S + u * s.ld;
      const float* lrow = L + u * ldl;
      const uint64_t oa = noff[a];
      const uint32_t da = (uint32_t)(noff[a + 1] - oa);
      const int hi = min(a, c0 + NJ_COLS);
      uint64_t row_b = 0, row_c = 0;
      for (int b = c0 + threadIdx.x; b < hi; b += AUC_THREADS) {
        const int64_t v = idx ? idx[b] : b;
        const float x = srow[v];
        const bool neg = !auc_pos(lrow[v]);                         // the labels were checked: 0 or 1
        const uint64_t bq = dl_negative(s, np, smp, sm, x, neg);
        if (neg) {
          const uint32_t k = auc_key(x);
          const uint64_t ob = noff[b];
          const uint64_t ca = nj_lost(lkey + oa, da, k), cb = nj_lost(lkey + ob, (uint32_t)(noff[b + 1] - ob), k);
          row_b += bq;
          row_c += ca;
          col_b[b - c0] += bq;
          col_c[b - c0] += cb;
        }
      }
      total += row_b;
      const uint64_t tb = block_sum_u64(row_b, sh_b), tc = block_sum_u64(row_c, sh_c);
      if (threadIdx.x == 0) {
        if (tb) atomicAdd(&out[(size_t)a * NJ_WORDS + NJ_B], (unsigned long long)tb);
        if (tc) atomicAdd(&out[(size_t)a * NJ_WORDS + NJ_C], (unsigned long long)tc);
      }
    }
    for (int j = threadIdx.x; j < NJ_COLS && c0 + j < rows; j += AUC_THREADS) {
      if (col_b[j]) atomicAdd(&out[(size_t)(c0 + j) * NJ_WORDS + NJ_B], (unsigned long long)col_b[j]);
      if (col_c[j]) atomicAdd(&out[(size_t)(c0 + j) * NJ_WORDS + NJ_C], (unsigned long long)col_c[j]);
    }
  }
  const uint64_t tot[1] = {total};
  block_add_u64(tot, sh_b, t_neg);
}

// The positives, in sorted order: out[a][NJ_A] += a_p, out[b][NJ_A] += a_p, *t_pos += a_p
__global__ __launch_bounds__(AUC_THREADS) void k_nj_positives(DlSide s, const uint32_t* __restrict__ ends, uint32_t np,
                                                              unsigned long long* __restrict__ out,
                                                              unsigned long long* __restrict__ t_pos) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  uint64_t total = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * AUC_THREADS + threadIdx.x; i < np; i += (uint64_t)gridDim.x * AUC_THREADS) {
    const uint64_t ap = dl_positive(s, np, i);
    const uint32_t e = ends[i];
    total += ap;
    if (ap) {
      atomicAdd(&out[(size_t)(e >> 16) * NJ_WORDS + NJ_A], (unsigned long long)ap);
      atomicAdd(&out[(size_t)(e & 0xffffu) * NJ_WORDS + NJ_A], (unsigned long long)ap);
    }
  }
  const uint64_t tot = block_sum_u64(total, sh);
  if (threadIdx.x == 0 && tot) atomicAdd(t_pos, (unsigned long long)tot);
}

__global__ __launch_bounds__(AUC_THREADS) void k_nj_finish(int rows, const uint32_t* __restrict__ deg,
                                                           unsigned long long* __restrict__ out) {
  for (int v = blockIdx.x * AUC_THREADS + threadIdx.x; v < rows; v += gridDim.x * AUC_THREADS) {
    out[(size_t)v * NJ_WORDS + NJ_P] = deg[v];
    out[(size_t)v * NJ_WORDS + NJ_N] = (uint32_t)(rows - 1) - deg[v];
  }
}

int nj_run(const char* who, hipStream_t st, int n, const float* L, int ldl, const float* S, int lds, const int64_t* idx, int rows,
           uint64_t* header, uint64_t* out) {
  AucBufs b;
  DlStage stage{who, st, b, n, L, S, nullptr, ldl, lds, 0, idx, rows, std::min(rows - 1, NJ_ROW_BLOCKS)};
  // behind the stage's counts, what scales with the selection: the two placement sums, the staged answer, noff [rows + 1],
  // deg [rows + 1] (deg[rows] = 0: the scan's last entry is the total)
  const size_t R1 = (size_t)rows + 1, words = 2 + (size_t)rows * NJ_WORDS + R1;
  if (int rc = stage.start(sizeof(uint64_t) * words + sizeof(uint32_t) * R1, sizeof(uint64_t) * words)) return rc;
  unsigned long long* t_sums = (unsigned long long*)stage.extra;           // {t_pos, t_neg}
  unsigned long long* out_stage = t_sums + 2;
  uint64_t* noff = (uint64_t*)(out_stage + (size_t)rows * NJ_WORDS);
  uint32_t* deg = stage.deg;
  if (int rc = stage.counted()) return rc;
  const uint64_t P = stage.P, N = stage.N, m = P + N;
  const int g = stage.g, gr = (rows + AUC_THREADS - 1) / AUC_THREADS;
  unsigned long long t[2] = {0, 0};
  if (P != 0 && N != 0) {                               // else every placement is 0
    // cum; key, ends, their second buffers; hist, ties; lnode, lkey, their second buffers [2 P4]
    const size_t P4 = stage.P4, H4 = stage.H4;
    Carver c{};
    if (int rc = stage.pool(4 + 8, 2 + 2, c)) return rc;
    DlSide s = {};
    s.S = S;
    s.ld = lds;
    s.cum = c.take<uint64_t>(H4);
    s.sorted = s.slot = c.take<uint32_t>(P4);           // the positives' pass runs over the sorted positives
    uint32_t* ends = c.take<uint32_t>(P4);
    uint32_t* tmp = c.take<uint32_t>(P4);
    uint32_t* etmp = c.take<uint32_t>(P4);
    s.hist = c.take<uint32_t>(H4);
    s.ties = c.take<uint32_t>(H4);
    uint32_t* lnode = c.take<uint32_t>(2 * P4);
    uint32_t* lkey = c.take<uint32_t>(2 * P4);
    uint32_t* ltmp = c.take<uint32_t>(2 * P4);
    uint32_t* ktmp = c.take<uint32_t>(2 * P4);
    if (int rc = stage.emit(s.sorted, ends)) return rc;
    if (int rc = auc_sort(st, s.sorted, tmp, P, stage.sort, ends, etmp)) return rc;
    const int gp = (int)std::min<uint64_t>(NJ_POS_BLOCKS, (P + AUC_THREADS - 1) / AUC_THREADS);
    k_nj_lists<<<gp, AUC_THREADS, 0, st>>>(s.sorted, ends, (uint32_t)P, lnode, lkey);
    MCGRA_KERNEL_CHECK();
    if (int rc = auc_sort(st, lnode, ltmp, 2 * P, stage.sort, lkey, ktmp)) return rc;
    rank_scan(st, deg, rows + 1, noff);
    MCGRA_HIP(hipMemsetAsync(s.hist, 0, sizeof(uint32_t) * 2 * H4, st));               // hist and ties are adjacent
    k_nj_negatives<<<g, AUC_THREADS, 0, st>>>(rows, s, L, ldl, idx, (uint32_t)P, lkey, noff, out_stage, t_sums + 1);
    MCGRA_KERNEL_CHECK();
    rank_scan(st, s.hist, (int)P, s.cum);
    k_nj_positives<<<gp, AUC_THREADS, 0, st>>>(s, ends, (uint32_t)P, out_stage, t_sums);
    MCGRA_KERNEL_CHECK();
  }
  k_nj_finish<<<gr, AUC_THREADS, 0, st>>>(rows, deg, out_stage);
  MCGRA_KERNEL_CHECK();
  MCGRA_HIP(hipMemcpyAsync(t, t_sums, sizeof(t), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (t[0] != t[1]) {                                   // sum a_p == sum b_q by construction
    set_error("%s: internal error: the two placement sums differ (%llu, %llu)", who, t[0], t[1]);
    return MCGRA_EHIP;
  }
  MCGRA_HIP(hipMemcpyAsync(out, out_stage, sizeof(uint64_t) * NJ_WORDS * (size_t)rows, hipMemcpyDeviceToDevice, st));
  MCGRA_HIP(hipStreamSynchronize(st));                  // the scratch is freed on return
  const uint64_t res[4] = {m, P, N, t[0]};
  memcpy(header, res, sizeof(res));
  return 0;
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_auc_node_jackknife(void* stream, int n, const float* labels, int ld_labels, const float* scores,
                                        int ld_scores, const int64_t* idx, int64_t n_idx, uint64_t* header, uint64_t* out) {
  if (!header || !out) { set_error("auc_node_jackknife: bad argument (header or out NULL)"); return MCGRA_EINVAL; }
  if (int rc = rank_check_args("auc_node_jackknife", n, {{labels, ld_labels, true}, {scores, ld_scores, true}}, idx, n_idx, 2))
    return rc;
  return nj_run("auc_node_jackknife", (hipStream_t)stream, n, labels, ld_labels, scores, ld_scores, idx, (int)n_idx, header, out);
}
