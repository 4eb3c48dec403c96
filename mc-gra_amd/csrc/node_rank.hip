// Whose neighbourhood leaked: per-node ranking counts of a scored square matrix restricted to idx (mcgra_node_rank_metrics).
//
// For position a of idx (idx == NULL: all n nodes in order) the candidates are the c = n_idx - 1 positions b != a; candidate b
// has score scores[idx[a]][idx[b]] and label labels[idx[a]][idx[b]]: row a of the gathered submatrix without its diagonal (an
// asymmetric matrix is ranked by rows).  Scores compare through auc_key (float32 values, -0.0 == +0.0, subnormals distinct);
// the best-first ranking is key descending, ties by ascending position b.  Row a of the answer is five integers:
//   P           positive candidates
//   wins        (positive, negative) candidate pairs with key(pos) > key(neg)
//   ties        (positive, negative) candidate pairs with equal keys
//   hits        positives among the P best of the best-first ranking
//   first_rank  1 + candidates with a key strictly above the best positive's (0 when P == 0)
//
// One workgroup of NODE_RANK_THREADS lanes owns one row at a time (rows are dealt over a grid the chip holds) and keeps it in
// LDS from the gather to the counts:
//   (rank_check_idx: idx only, range check and repeats -- rank_common.hip)
//   gather   one read of the row: candidate b becomes the 64-bit composite  key << 32 | (0x7fff - b) << 1 | label  (a valid key
//            is never 0, so 0 pads the row to its class length and sorts last); the argument predicates run on what is read
//   sort     an in-place bitonic sort of the composites, descending: key descending, then position ascending, the label riding
//            along; lane t holds elements [t E, (t + 1) E) in registers for the strides below E, only the wider strides go
//            through LDS.  Its cost is a function of the class length alone -- not of the scores, and not of how many are
//            positive
//   counts   lane t owns the E = CAP / NODE_RANK_THREADS consecutive ranks [t E, (t + 1) E).  A sum scan over the lanes gives
//            the positives and negatives before each rank; a max scan carries the (positives, negatives) before the HEAD of the
//            tie group that is open at the lane's first rank (both counts grow from head to head, so the last head is the
//            maximum).  At the end of each tie group its positives g_p and negatives g_n and the negatives below it are then at
//            hand: wins += g_p * below, ties += g_p * g_n; the first group with a positive gives first_rank = 1 + its head's
//            rank; hits = labels among the ranks below P.
// Element i of a row lives at LDS slot i + i / 32: the sort's lanes touch consecutive slots, and the counts' lanes, E elements
// apart, land on distinct banks.
// Row-length classes: the sort needs a power of two, so a row of c candidates runs in the smallest class CAP >= c of
// NODE_RANK_CLASSES; LDS per workgroup is 8.25 bytes per class element (8.25 KiB ... 132 KiB), so short rows get several
// workgroups per CU.  n_idx <= MCGRA_NODE_RANK_MAX_NIDX = the largest class.
// Everything is integers: no result depends on the order in which workgroups run, and every call returns the same bits.
// Device scratch: 40 bytes per selected node (the answer is staged and copied to `out` only when every check has passed) and 4
// bytes per node of the graph when idx is given.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mcgra.h"
#include "common.h"
#include "rank_common.h"

namespace mcgra {
namespace {
constexpr int NODE_RANK_THREADS = 512;
constexpr int NODE_RANK_WAVES = NODE_RANK_THREADS / 64;
constexpr int NODE_RANK_MIN_CLASS = 1024;                       // the classes: 1024, 2048, ..., MCGRA_NODE_RANK_MAX_NIDX
constexpr int NODE_RANK_LDS = 160 * 1024;                       // per CU
static_assert(NODE_RANK_MIN_CLASS >= 2 * NODE_RANK_THREADS, "every lane owns at least two ranks");
static_assert((MCGRA_NODE_RANK_MAX_NIDX & (MCGRA_NODE_RANK_MAX_NIDX - 1)) == 0 && MCGRA_NODE_RANK_MAX_NIDX <= 0x8000,
              "a class is a power of two and a position fits 15 bits");

__device__ __forceinline__ int nr_slot(int i) { return i + (i >> 5); }

// inclusive scan over the workgroup's lanes; sh: NODE_RANK_WAVES entries, free for reuse behind the call's second barrier
template <typename Op>
__device__ __forceinline__ uint32_t nr_block_scan(uint32_t v, uint32_t* sh, Op op) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(v, o, 64);
    if (lane >= o) v = op(v, up);
  }
  if (lane == 63) sh[w] = v;
  __syncthreads();
  uint32_t before = 0;                                          // 0 is the identity of both scans used here (sum, max)
  for (int q = 0; q < w; ++q) before = op(before, sh[q]);
  __syncthreads();
  return op(v, before);
}

// one stride j < E of the bitonic network on the E elements a lane holds (element e is element base + e of the row): the
// pair (e, e | j) is put in descending order where (base + e) & k is 0, in ascending order elsewhere
template <int E>
__device__ __forceinline__ void nr_local_pass(uint64_t (&r)[E], int j, int base, int k) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if ((e & j) == 0) {
      const uint64_t x = r[e], y = r[e | j];
      const bool swap = (x < y) == (((base + e) & k) == 0);
      r[e] = swap ? y : x;
      r[e | j] = swap ? x : y;
    }
  }
}

// sum over the workgroup, valid in every lane
__device__ __forceinline__ uint32_t nr_block_sum(uint32_t v, uint32_t* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
  for (int q = 0; q < NODE_RANK_WAVES; ++q) t += sh[q];
  __syncthreads();
  return t;
}

// stage[a][0..5) = the five counts of row a of the selection, a = blockIdx.x, + gridDim.x, ...; *flags |= argument errors
template <int CAP>
__global__ __launch_bounds__(NODE_RANK_THREADS) void k_node_rank(int rows, const float* __restrict__ S, int64_t lds,
                                                                 const float* __restrict__ L, int64_t ldl,
                                                                 const int64_t* __restrict__ idx, int64_t* __restrict__ stage,
                                                                 int* __restrict__ flags) {
  constexpr int E = CAP / NODE_RANK_THREADS;
  __shared__ uint64_t rec[CAP + CAP / 32];
  __shared__ uint32_t sh[NODE_RANK_WAVES], wave_last[NODE_RANK_WAVES];
  __shared__ uint32_t first_rank;
  const int t = threadIdx.x;
  const int c = rows - 1;                                       // candidates per row, 1 <= c <= CAP
  int f = 0;
  for (int a = blockIdx.x; a < rows; a += gridDim.x) {
    // ---- gather
    const int64_t u = idx ? idx[a] : a;
    const float* srow = S + u * lds;
    const float* lrow = L + u * ldl;
    for (int b = t; b < rows; b += NODE_RANK_THREADS) {
      if (b == a) continue;
      const int64_t v = idx ? idx[b] : b;
      const float s = srow[v], l = lrow[v];
      const bool p = auc_pos(l);
      if (!auc_finite(s)) f |= AUC_BAD_SCORE;
      if (!p && !auc_neg(l)) f |= AUC_BAD_LABEL;                // also NaN
      rec[nr_slot(b - (b > a))] = (uint64_t)auc_key(s) << 32 | (uint64_t)(0x7fff - b) << 1 | (p ? 1u : 0u);
    }
    for (int i = c + t; i < CAP; i += NODE_RANK_THREADS) rec[nr_slot(i)] = 0;
    if (t == 0) first_rank = 0;
    __syncthreads();
    // ---- sort, descending.  Lane t keeps elements [t E, (t + 1) E) in registers for every compare-exchange whose two
    // elements lie less than E apart (the stages up to k = E entirely, and the last log2 E strides of every later stage); the
    // wider strides go through LDS, one barrier each
    uint64_t r[E];
#pragma unroll
    for (int e = 0; e < E; ++e) r[e] = rec[nr_slot(t * E + e)];
#pragma unroll
    for (int k = 2; k <= E; k <<= 1) {
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) nr_local_pass<E>(r, j, t * E, k);
    }
    for (int k = 2 * E; k <= CAP; k <<= 1) {
#pragma unroll
      for (int e = 0; e < E; ++e) rec[nr_slot(t * E + e)] = r[e];
      __syncthreads();
      for (int j = k >> 1; j >= E; j >>= 1) {
#pragma unroll 8
        for (int q = 0; q < E / 2; ++q) {
          const int p = q * NODE_RANK_THREADS + t;              // pair p of CAP / 2
          const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;
          const uint64_t x = rec[nr_slot(lo)], y = rec[nr_slot(hi)];
          if ((x < y) == ((lo & k) == 0)) { rec[nr_slot(lo)] = y; rec[nr_slot(hi)] = x; }
        }
        __syncthreads();
      }
#pragma unroll
      for (int e = 0; e < E; ++e) r[e] = rec[nr_slot(t * E + e)];
#pragma unroll
      for (int j = E >> 1; j > 0; j >>= 1) nr_local_pass<E>(r, j, t * E, k);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) rec[nr_slot(t * E + e)] = r[e];
    __syncthreads();
    // ---- counts: this lane's ranks [t E, (t + 1) E) are in r; the key before them and the key behind them
    const uint32_t key_before = t ? (uint32_t)(rec[nr_slot(t * E - 1)] >> 32) : 0u;          // 0: rank 0 is a head
    const uint32_t key_behind = t + 1 < NODE_RANK_THREADS ? (uint32_t)(rec[nr_slot(t * E + E)] >> 32) : 0u;
    uint32_t mine = 0;                                          // positives << 16 | negatives among this lane's ranks
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (t * E + e < c) mine += (r[e] & 1u) ? 0x10000u : 1u;
    const uint32_t incl = nr_block_scan(mine, sh, [](uint32_t x, uint32_t y) { return x + y; });
    const uint32_t total = nr_block_sum(mine, sh);
    const uint32_t P = total >> 16, N = total & 0xffffu;
    // (positives << 16 | negatives) before the last head among this lane's ranks; 0 without one
    uint32_t run = incl - mine, head = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (t * E + e < c) {
        const uint32_t key = (uint32_t)(r[e] >> 32), prev = e ? (uint32_t)(r[e - 1] >> 32) : key_before;
        if (key != prev) head = run;
        run += (r[e] & 1u) ? 0x10000u : 1u;
      }
    }
    const uint32_t hscan = nr_block_scan(head, sh, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
    // the head of the group open at this lane's first rank: the scan's value one lane down (0 for lane 0: rank 0 is a head)
    uint32_t open = __shfl_up(hscan, 1, 64);
    if ((t & 63) == 63) wave_last[t >> 6] = hscan;
    __syncthreads();
    if ((t & 63) == 0) open = t ? wave_last[(t >> 6) - 1] : 0u;
    uint32_t wins = 0, ties = 0, hits = 0;
    run = incl - mine;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = t * E + e;
      if (i < c) {
        const uint32_t key = (uint32_t)(r[e] >> 32), prev = e ? (uint32_t)(r[e - 1] >> 32) : key_before;
        const uint32_t next = e + 1 < E ? (uint32_t)(r[e + 1] >> 32) : key_behind;
        if (key != prev) open = run;
        const uint32_t lab = (uint32_t)(r[e] & 1u);
        run += lab ? 0x10000u : 1u;
        if (lab && (uint32_t)i < P) ++hits;
        if (i == c - 1 || next != key) {                        // the group ends here
          const uint32_t gp = (run >> 16) - (open >> 16), gn = (run & 0xffffu) - (open & 0xffffu);
          wins += gp * (N - (run & 0xffffu));
          ties += gp * gn;
          if (gp && (open >> 16) == 0) first_rank = 1 + (open & 0xffffu);   // one group: the first with a positive
        }
      }
    }
    const uint32_t w_all = nr_block_sum(wins, sh), t_all = nr_block_sum(ties, sh), h_all = nr_block_sum(hits, sh);
    if (t == 0) {
      int64_t* o = stage + (int64_t)a * 5;
      o[0] = P; o[1] = w_all; o[2] = t_all; o[3] = h_all; o[4] = first_rank;
    }
    __syncthreads();                                            // rec and first_rank are rewritten by the next row
  }
  if (f) atomicOr(flags, f);
}

template <int CAP>
int node_rank_launch(hipStream_t st, int cus, int rows, const float* S, int lds, const float* L, int ldl, const int64_t* idx,
                     int64_t* stage, int* flags) {
  constexpr int bytes = (CAP + CAP / 32) * 8 + 256;
  const int per_cu = std::max(1, std::min(2048 / NODE_RANK_THREADS, NODE_RANK_LDS / bytes));
  const int grid = std::min(rows, cus * per_cu);
  k_node_rank<CAP><<<grid, NODE_RANK_THREADS, 0, st>>>(rows, S, lds, L, ldl, idx, stage, flags);
  MCGRA_KERNEL_CHECK();
  return 0;
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_node_rank_metrics(void* stream, int n, const float* labels, int ld_labels, const float* scores,
                                       int ld_scores, const int64_t* idx, int64_t n_idx, int64_t* out) {
  const char* who = "node_rank_metrics";
  if (!out) { set_error("%s: bad argument (out NULL)", who); return MCGRA_EINVAL; }
  // the cap: a row of more nodes does not fit one workgroup's LDS
  if (int rc = rank_check_args(who, n, {{labels, ld_labels, true}, {scores, ld_scores, true}}, idx, n_idx, 2,
                               MCGRA_NODE_RANK_MAX_NIDX))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const int rows = (int)n_idx;
  int dev = 0, cus = 0;
  MCGRA_HIP(hipGetDevice(&dev));
  MCGRA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  AucBufs b;
  int* flags = b.get<int>(1);
  int64_t* stage = b.get<int64_t>((size_t)rows * 5);
  if (!flags || !stage) { set_error("node_rank_metrics: hipMalloc of the scratch of %d rows failed", rows); return MCGRA_ENOMEM; }
  MCGRA_HIP(hipMemsetAsync(flags, 0, sizeof(int), st));
  int h = 0;
  if (int rc = rank_check_idx(who, st, b, n, idx, rows, flags)) return rc;
  const int c = rows - 1;
  int rc;
  if (c <= 1024) rc = node_rank_launch<1024>(st, cus, rows, scores, ld_scores, labels, ld_labels, idx, stage, flags);
  else if (c <= 2048) rc = node_rank_launch<2048>(st, cus, rows, scores, ld_scores, labels, ld_labels, idx, stage, flags);
  else if (c <= 4096) rc = node_rank_launch<4096>(st, cus, rows, scores, ld_scores, labels, ld_labels, idx, stage, flags);
  else if (c <= 8192) rc = node_rank_launch<8192>(st, cus, rows, scores, ld_scores, labels, ld_labels, idx, stage, flags);
  else rc = node_rank_launch<MCGRA_NODE_RANK_MAX_NIDX>(st, cus, rows, scores, ld_scores, labels, ld_labels, idx, stage, flags);
  if (rc) return rc;
  MCGRA_HIP(hipMemcpyAsync(&h, flags, sizeof(int), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (int rc = rank_flag_error(who, h)) return rc;
  MCGRA_HIP(hipMemcpyAsync(out, stage, sizeof(int64_t) * 5 * (size_t)rows, hipMemcpyDeviceToDevice, st));
  MCGRA_HIP(hipStreamSynchronize(st));                          // the scratch is freed on return
  return 0;
}
