// Exact binary ROC-AUC of a scored square matrix restricted to idx x idx: main.metric_pool (main.py:66-75), i.e.
// sklearn.metrics.roc_curve + auc on ori_adj[idx][:, idx] against inference_adj[idx][:, idx], without gathering the
// submatrix.  AUC = U / (P N) with 2U = sum over positives of (2 #negatives with a lower score + #negatives with an equal
// score) (Mann-Whitney, ties counted 1/2), which is exactly the area under the step curve roc_curve draws.
//
// Passes (DESIGN.md "Recovered-adjacency AUC"):
//   k_auc_index        idx only: range check, repeats; a repeat-free idx of all n nodes is the whole matrix in another
//                      order (the AUC depends on the multiset of (label, score) pairs only) and runs as idx = NULL
//   k_auc_classify     one read of the selected scores and labels: argument checks, per-block positive / negative counts
//   k_auc_emit         a second read: each entry's order-preserving 32-bit key, positives to one region of the
//                      scratch, negatives to another, at per-block offsets (the host's scan of the counts)
//   k_auc_digit_*      per region, a stable LSD radix sort of the keys: 4 passes of 8 bits, each a per-block digit
//                      count, one scan of the (digit, block) counts and a stable scatter
//   k_auc_pairs        each key of the smaller class looks up its lower and upper bound in the sorted larger class;
//                      the sum of the two is that key's share of 2U
// Counts and 2U are 64-bit integers merged with global integer atomics, so the result does not depend on the order in
// which blocks run; the one rounding is the final division (host, exact integer long division, nearest even).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/mcgra.h"
#include "common.h"

namespace mcgra {

namespace {
constexpr int AUC_THREADS = 256;
constexpr int AUC_ROW_BLOCKS = 1024;       // blocks of the two passes over the matrix (grid-stride over selected rows)
constexpr int AUC_SORT_TILE = 1024;        // keys staged per step of a sort block (256 lanes x one 16-byte load)
constexpr int AUC_SORT_BLOCKS = 1024;      // at most this many tiles of keys per sort pass
constexpr int64_t AUC_MAX_NIDX = 65535;    // 2 P N <= 2 (n_idx^2 / 2)^2 < 2^63

enum { AUC_BAD_SCORE = 1, AUC_BAD_LABEL = 2, AUC_BAD_INDEX = 4, AUC_REPEAT = 8 };

// float32 -> unsigned key with the same order; -0.0 and +0.0 are one value.  Bit tests throughout, so that no
// floating-point mode (denormal flushing) can merge a subnormal with zero.
__device__ __forceinline__ uint32_t auc_key(float s) {
  uint32_t u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ bool auc_finite(float s) { return (__float_as_uint(s) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool auc_pos(float l) { return __float_as_uint(l) == 0x3f800000u; }
__device__ __forceinline__ bool auc_neg(float l) { return (__float_as_uint(l) & 0x7fffffffu) == 0u; }

// f(score, label) for every selected entry this block owns: rows r = blockIdx.x, + gridDim.x, ... of the selection.
// idx == NULL: rows and columns 0 .. n-1, 16-byte loads when a row's scores and labels share their alignment;
// otherwise row idx[r], columns idx[0 .. rows).
template <class F>
__device__ __forceinline__ void auc_for_each(int rows, const float* __restrict__ S, int64_t lds, const float* __restrict__ L,
                                             int64_t ldl, const int64_t* __restrict__ idx, F&& f) {
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const int64_t i = idx ? idx[r] : r;
    const float* srow = S + i * lds;
    const float* lrow = L + i * ldl;
    if (idx) {
      for (int c = threadIdx.x; c < rows; c += blockDim.x) {
        const int64_t j = idx[c];
        f(srow[j], lrow[j]);
      }
      continue;
    }
    const uintptr_t as = (uintptr_t)srow, al = (uintptr_t)lrow;
    int head = rows;                                    // scalar prefix; the whole row when the alignments differ
    if (((as ^ al) & 15) == 0) head = min(rows, (int)(((16 - (as & 15)) & 15) >> 2));
    for (int c = threadIdx.x; c < head; c += blockDim.x) f(srow[c], lrow[c]);
    const int nv = (rows - head) >> 2;
    const float4* s4 = (const float4*)(srow + head);
    const float4* l4 = (const float4*)(lrow + head);
    for (int v = threadIdx.x; v < nv; v += blockDim.x) {
      const float4 a = s4[v], b = l4[v];
      f(a.x, b.x); f(a.y, b.y); f(a.z, b.z); f(a.w, b.w);
    }
    for (int c = head + 4 * nv + threadIdx.x; c < rows; c += blockDim.x) f(srow[c], lrow[c]);
  }
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the block (AUC_THREADS lanes), valid in thread 0
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t* sh) {
  v = wave_sum_u64(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < AUC_THREADS / 64; ++w) t += sh[w];
  return t;
}
}  // namespace

__global__ __launch_bounds__(AUC_THREADS) void k_auc_index(int n, int64_t n_idx, const int64_t* __restrict__ idx,
                                                           uint32_t* __restrict__ seen, int* __restrict__ flags) {
  int f = 0;
  for (int64_t a = (int64_t)blockIdx.x * AUC_THREADS + threadIdx.x; a < n_idx; a += (int64_t)gridDim.x * AUC_THREADS) {
    const int64_t v = idx[a];
    if (v < 0 || v >= n) f |= AUC_BAD_INDEX;
    else if (atomicAdd(&seen[v], 1u) != 0u) f |= AUC_REPEAT;
  }
  if (f) atomicOr(flags, f);
}

// counts[2 b] / counts[2 b + 1] = positives / negatives block b selects; flags |= the argument errors it meets
__global__ __launch_bounds__(AUC_THREADS) void k_auc_classify(int rows, const float* __restrict__ S, int64_t lds,
                                                              const float* __restrict__ L, int64_t ldl,
                                                              const int64_t* __restrict__ idx, uint64_t* __restrict__ counts,
                                                              int* __restrict__ flags) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  uint32_t pos = 0, tot = 0;
  int f = 0;
  auc_for_each(rows, S, lds, L, ldl, idx, [&](float s, float l) {
    if (!auc_finite(s)) f |= AUC_BAD_SCORE;
    if (auc_pos(l)) ++pos;
    else if (!auc_neg(l)) f |= AUC_BAD_LABEL;   // also NaN
    ++tot;
  });
  if (f) atomicOr(flags, f);
  const uint64_t p = block_sum_u64(pos, sh);
  __syncthreads();
  const uint64_t t = block_sum_u64(tot, sh);
  if (threadIdx.x == 0) { counts[2 * blockIdx.x] = p; counts[2 * blockIdx.x + 1] = t - p; }
}

// keys of block b's positives to keys[offs[2 b] ..), of its negatives to keys[offs[2 b + 1] ..) (any order inside a block)
__global__ __launch_bounds__(AUC_THREADS) void k_auc_emit(int rows, const float* __restrict__ S, int64_t lds,
                                                          const float* __restrict__ L, int64_t ldl,
                                                          const int64_t* __restrict__ idx, const uint64_t* __restrict__ offs,
                                                          uint32_t* __restrict__ keys) {
  __shared__ uint32_t cur[2];
  if (threadIdx.x < 2) cur[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t o_pos = offs[2 * blockIdx.x], o_neg = offs[2 * blockIdx.x + 1];
  const int lane = threadIdx.x & 63;
  const uint64_t below = (1ull << lane) - 1ull;
  auc_for_each(rows, S, lds, L, ldl, idx, [&](float s, float l) {
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
    const uint64_t at = p ? o_pos + bp + __popcll(mp & below) : o_neg + bn + __popcll(act & ~mp & below);
    keys[at] = auc_key(s);
  });
}

// cnt[d * nb + b] = keys of tile b whose digit (key >> shift) & 255 is d
__global__ __launch_bounds__(AUC_THREADS) void k_auc_digit_count(const uint32_t* __restrict__ keys, uint64_t count,
                                                                 uint64_t tile, int shift, int nb,
                                                                 uint32_t* __restrict__ cnt) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t beg = blockIdx.x * tile, end = min(count, beg + tile);
  for (uint64_t e = beg + 4 * threadIdx.x; e < end; e += 4 * AUC_THREADS) {
    if (e + 4 <= end) {
      const uint4 k = *(const uint4*)(keys + e);     // beg and the region start are multiples of 4 keys
      atomicAdd(&h[(k.x >> shift) & 255], 1u); atomicAdd(&h[(k.y >> shift) & 255], 1u);
      atomicAdd(&h[(k.z >> shift) & 255], 1u); atomicAdd(&h[(k.w >> shift) & 255], 1u);
    } else {
      for (uint64_t q = e; q < end; ++q) atomicAdd(&h[(keys[q] >> shift) & 255], 1u);
    }
  }
  __syncthreads();
  cnt[(size_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// off[i] = cnt[0] + ... + cnt[i - 1] over len entries, one block of 1024 lanes
__global__ __launch_bounds__(1024) void k_auc_digit_scan(const uint32_t* __restrict__ cnt, int len, uint64_t* __restrict__ off) {
  __shared__ uint64_t sh[1024];
  const int per = (len + 1023) / 1024;
  const int beg = min(len, (int)threadIdx.x * per), end = min(len, beg + per);
  uint64_t s = 0;
  for (int i = beg; i < end; ++i) s += cnt[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const uint64_t v = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  uint64_t run = sh[threadIdx.x] - s;
  for (int i = beg; i < end; ++i) { off[i] = run; run += cnt[i]; }
}

// stable scatter of tile b by digit: keys are ranked in index order, 256 at a time (8 ballots give each lane the lanes
// of its wave with the same digit; per-wave counts in LDS order the four waves)
__global__ __launch_bounds__(AUC_THREADS) void k_auc_digit_scatter(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                                   uint64_t count, uint64_t tile, int shift, int nb,
                                                                   const uint64_t* __restrict__ off) {
  __shared__ uint32_t stage[AUC_SORT_TILE];
  __shared__ uint32_t wc[AUC_THREADS / 64][256];
  __shared__ uint64_t run[256];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  run[t] = off[(size_t)t * nb + blockIdx.x];
  for (int q = 0; q < AUC_THREADS / 64; ++q) wc[q][t] = 0;
  const uint64_t beg = blockIdx.x * tile, end = min(count, beg + tile);
  for (uint64_t base = beg; base < end; base += AUC_SORT_TILE) {
    __syncthreads();
    const uint64_t e = base + 4 * t;
    if (e + 4 <= end) {
      *(uint4*)(stage + 4 * t) = *(const uint4*)(src + e);
    } else {
      for (int q = 0; q < 4; ++q) stage[4 * t + q] = e + q < end ? src[e + q] : 0u;
    }
    __syncthreads();
    for (int k = 0; k < AUC_SORT_TILE / AUC_THREADS; ++k) {
      const uint64_t el = base + (uint64_t)k * AUC_THREADS + t;
      const bool valid = el < end;
      const uint32_t key = stage[k * AUC_THREADS + t];
      const uint32_t d = (key >> shift) & 255u;
      uint64_t peers = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bb = __ballot(bit);
        peers &= bit ? bb : ~bb;
      }
      const int r = __popcll(peers & below);
      if (valid && r == 0) wc[w][d] = (uint32_t)__popcll(peers);
      __syncthreads();
      if (valid) {
        uint64_t at = run[d] + r;
        for (int q = 0; q < w; ++q) at += wc[q][d];
        dst[at] = key;
      }
      __syncthreads();
      uint32_t s = 0;
      for (int q = 0; q < AUC_THREADS / 64; ++q) { s += wc[q][t]; wc[q][t] = 0; }
      run[t] += s;
      __syncthreads();
    }
  }
}

// acc += for each key x of A: lower_bound(B, x) + upper_bound(B, x) (a_pos: A holds the positives), or, A holding the
// negatives, (|B| - upper_bound) + (|B| - lower_bound): the positives above x twice and those equal to x once
__global__ __launch_bounds__(AUC_THREADS) void k_auc_pairs(const uint32_t* __restrict__ A, uint64_t na,
                                                           const uint32_t* __restrict__ B, uint64_t nbk, int a_pos,
                                                           unsigned long long* __restrict__ acc) {
  __shared__ uint64_t sh[AUC_THREADS / 64];
  uint64_t s = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * AUC_THREADS + threadIdx.x; i < na; i += (uint64_t)gridDim.x * AUC_THREADS) {
    const uint32_t x = A[i];
    uint64_t lo = 0, hi = nbk;                      // first key >= x
    while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (B[m] < x) lo = m + 1; else hi = m; }
    const uint64_t lt = lo;
    hi = nbk;                                       // first key > x
    while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (B[m] <= x) lo = m + 1; else hi = m; }
    const uint64_t le = lo;
    s += a_pos ? lt + le : (nbk - le) + (nbk - lt);
  }
  const uint64_t tot = block_sum_u64(s, sh);
  if (threadIdx.x == 0 && tot) atomicAdd(acc, (unsigned long long)tot);
}

namespace {
struct AucBufs {
  std::vector<void*> p;
  ~AucBufs() { for (void* q : p) (void)hipFree(q); }
  template <typename T>
  T* get(size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) return nullptr;
    p.push_back(q);
    return (T*)q;
  }
};

// stable LSD radix sort of keys[0, count) (a multiple-of-4 aligned region), tmp the same size; result in keys
int auc_sort(hipStream_t st, uint32_t* keys, uint32_t* tmp, uint64_t count, uint32_t* cnt, uint64_t* off) {
  if (count < 2) return 0;
  uint64_t tile = (count + AUC_SORT_BLOCKS - 1) / AUC_SORT_BLOCKS;
  tile = (tile + AUC_SORT_TILE - 1) / AUC_SORT_TILE * AUC_SORT_TILE;
  const int nb = (int)((count + tile - 1) / tile);
  uint32_t* src = keys;
  uint32_t* dst = tmp;
  for (int shift = 0; shift < 32; shift += 8) {
    k_auc_digit_count<<<nb, AUC_THREADS, 0, st>>>(src, count, tile, shift, nb, cnt);
    k_auc_digit_scan<<<1, 1024, 0, st>>>(cnt, 256 * nb, off);
    k_auc_digit_scatter<<<nb, AUC_THREADS, 0, st>>>(src, dst, count, tile, shift, nb, off);
    uint32_t* x = src; src = dst; dst = x;
  }
  MCGRA_KERNEL_CHECK();
  return 0;                                         // four passes: the sorted keys are back in `keys`
}

// num / den rounded to the nearest double (ties to even), 0 < num <= den < 2^63
double auc_divide(uint64_t num, uint64_t den) {
  if (num == 0) return 0.0;
  typedef unsigned __int128 u128;
  const u128 N = num, D = den;
  int sh = 0;
  while ((N << sh) < (D << 53)) ++sh;               // 2^53 <= N 2^sh / D < 2^54 (N 2^sh < 2^117)
  const u128 x = N << sh;
  uint64_t q = (uint64_t)(x / D);
  const bool rest = (x % D) != 0;
  const bool half = q & 1u;
  q >>= 1;                                          // 53 bits; the dropped bit and the remainder decide the rounding
  if (half && (rest || (q & 1u))) ++q;
  return ldexp((double)q, 1 - sh);
}
}  // namespace

}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_roc_auc(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                             const int64_t* idx, int64_t n_idx, double* out) {
  if (n < 1 || !labels || !scores || !out || ld_labels < n || ld_scores < n || (idx && n_idx < 1)) {
    set_error("roc_auc: bad argument");
    return MCGRA_EINVAL;
  }
  if (!idx) n_idx = n;
  if (n_idx > AUC_MAX_NIDX) {
    set_error("roc_auc: %lld selected nodes; 2 P N of more than %lld does not fit 64 bits", (long long)n_idx,
              (long long)AUC_MAX_NIDX);
    return MCGRA_ENOSUP;
  }
  hipStream_t st = (hipStream_t)stream;
  AucBufs b;
  int* flags = b.get<int>(1);
  uint64_t* counts = b.get<uint64_t>(2 * AUC_ROW_BLOCKS);
  unsigned long long* acc = b.get<unsigned long long>(1);
  if (!flags || !counts || !acc) { set_error("hipMalloc failed"); return MCGRA_ENOMEM; }
  MCGRA_HIP(hipMemsetAsync(flags, 0, sizeof(int), st));
  MCGRA_HIP(hipMemsetAsync(acc, 0, sizeof(unsigned long long), st));
  int h_flags = 0;
  if (idx) {
    uint32_t* seen = b.get<uint32_t>(n);
    if (!seen) { set_error("hipMalloc failed"); return MCGRA_ENOMEM; }
    MCGRA_HIP(hipMemsetAsync(seen, 0, sizeof(uint32_t) * (size_t)n, st));
    const int g = (int)std::min<int64_t>(1024, (n_idx + AUC_THREADS - 1) / AUC_THREADS);
    k_auc_index<<<g, AUC_THREADS, 0, st>>>(n, n_idx, idx, seen, flags);
    MCGRA_KERNEL_CHECK();
    MCGRA_HIP(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
    MCGRA_HIP(hipStreamSynchronize(st));
    if (h_flags & AUC_BAD_INDEX) { set_error("roc_auc: a node id outside [0, %d)", n); return MCGRA_EINVAL; }
    if (!(h_flags & AUC_REPEAT) && n_idx == n) idx = nullptr;      // a permutation of all nodes: the same multiset
  }
  const int rows = (int)n_idx;
  const int g = std::min(rows, AUC_ROW_BLOCKS);
  k_auc_classify<<<g, AUC_THREADS, 0, st>>>(rows, scores, ld_scores, labels, ld_labels, idx, counts, flags);
  MCGRA_KERNEL_CHECK();
  std::vector<uint64_t> h(2 * (size_t)g);
  MCGRA_HIP(hipMemcpyAsync(h.data(), counts, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (h_flags & (AUC_BAD_SCORE | AUC_BAD_LABEL)) {
    set_error("roc_auc: %s%s", (h_flags & AUC_BAD_SCORE) ? "a selected score is NaN or infinite (sklearn: ValueError) " : "",
              (h_flags & AUC_BAD_LABEL) ? "a selected label is neither 0 nor 1 (sklearn: ValueError)" : "");
    return MCGRA_EINVAL;
  }
  uint64_t P = 0, N = 0;
  for (int i = 0; i < g; ++i) { P += h[2 * i]; N += h[2 * i + 1]; }
  if (P == 0 || N == 0) { *out = NAN; return 0; }     // roc_curve: tpr or fpr is 0 / 0 (sklearn warns), auc is NaN
  // positives at [0, P), negatives at [nbase, nbase + N): each region starts on a 16-byte boundary
  const uint64_t nbase = (P + 3) / 4 * 4;
  for (uint64_t op = 0, on = nbase, i = 0; i < (uint64_t)g; ++i) {
    const uint64_t p = h[2 * i], q = h[2 * i + 1];
    h[2 * i] = op; h[2 * i + 1] = on;
    op += p; on += q;
  }
  uint32_t* keys = b.get<uint32_t>(nbase + N);
  uint32_t* tmp = b.get<uint32_t>(nbase + N);
  uint32_t* cnt = b.get<uint32_t>(256 * AUC_SORT_BLOCKS);
  uint64_t* off = b.get<uint64_t>(256 * AUC_SORT_BLOCKS);
  if (!keys || !tmp || !cnt || !off) { set_error("roc_auc: hipMalloc of 2 x %llu keys failed", (unsigned long long)(nbase + N)); return MCGRA_ENOMEM; }
  MCGRA_HIP(hipMemcpyAsync(counts, h.data(), sizeof(uint64_t) * h.size(), hipMemcpyHostToDevice, st));
  k_auc_emit<<<g, AUC_THREADS, 0, st>>>(rows, scores, ld_scores, labels, ld_labels, idx, counts, keys);
  MCGRA_KERNEL_CHECK();
  if (int rc = auc_sort(st, keys, tmp, P, cnt, off)) return rc;
  if (int rc = auc_sort(st, keys + nbase, tmp + nbase, N, cnt, off)) return rc;
  const bool a_pos = P <= N;                        // look the smaller class up in the larger one
  const uint32_t* A = a_pos ? keys : keys + nbase;
  const uint32_t* B = a_pos ? keys + nbase : keys;
  const uint64_t na = a_pos ? P : N, nbk = a_pos ? N : P;
  const int gp = (int)std::min<uint64_t>(4096, (na + AUC_THREADS - 1) / AUC_THREADS);
  k_auc_pairs<<<gp, AUC_THREADS, 0, st>>>(A, na, B, nbk, a_pos ? 1 : 0, acc);
  MCGRA_KERNEL_CHECK();
  unsigned long long u2 = 0;
  MCGRA_HIP(hipMemcpyAsync(&u2, acc, sizeof(u2), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  *out = auc_divide((uint64_t)u2, 2 * P * N);
  return 0;
}
