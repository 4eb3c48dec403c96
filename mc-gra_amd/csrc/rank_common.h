// What the ranking entries share (auc.hip: AUC, average precision; topk.hip: the k best pairs; two_means.hip: the 2-means
// split and the threshold edge list): the order-preserving key of a float32 score, the argument predicates, the idx check,
// the pair of a packed position, integer block sums, and the stable LSD radix sort of 32-bit keys
// (optionally with a 32-bit payload) -- per-block digit counts, one scan, a stable scatter.  Everything here is integer
// work, so no result depends on the order in which blocks run.  Each translation unit gets its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/mcgra.h"
#include "common.h"

namespace mcgra {
namespace {
constexpr int AUC_THREADS = 256;
constexpr int AUC_SORT_TILE = 1024;        // keys staged per step of a sort block (256 lanes x one 16-byte load)
constexpr int AUC_SORT_BLOCKS = 1024;      // at most this many tiles of keys per sort pass
constexpr int64_t AUC_MAX_NIDX = 65535;    // 2 P N <= 2 (n_idx^2 / 2)^2 < 2^63; a packed pair position fits 32 bits

enum { AUC_BAD_SCORE = 1, AUC_BAD_LABEL = 2, AUC_BAD_INDEX = 4, AUC_REPEAT = 8, AUC_BAD_FACTOR = 16 };

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

// pair (a, b), a > b >= 0, of packed position p = a (a - 1) / 2 + b
__device__ __forceinline__ void topk_unpack(uint32_t p, uint32_t& a, uint32_t& b) {
  uint32_t x = (uint32_t)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
  while ((uint64_t)x * (x - 1) / 2 > p) --x;
  while ((uint64_t)x * (x + 1) / 2 <= p) ++x;
  a = x;
  b = p - (uint32_t)((uint64_t)x * (x - 1) / 2);
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
// of its wave with the same digit; per-wave counts in LDS order the four waves).  PAY: a 32-bit payload travels with
// each key (psrc -> pdst).
template <bool PAY>
__global__ __launch_bounds__(AUC_THREADS) void k_auc_digit_scatter(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                                   const uint32_t* __restrict__ psrc, uint32_t* __restrict__ pdst,
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
        if (PAY) pdst[at] = psrc[el];
      }
      __syncthreads();
      uint32_t s = 0;
      for (int q = 0; q < AUC_THREADS / 64; ++q) { s += wc[q][t]; wc[q][t] = 0; }
      run[t] += s;
      __syncthreads();
    }
  }
}

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

// stable LSD radix sort of keys[0, count) (a multiple-of-4 aligned region), tmp the same size; result in keys.  pay != NULL:
// pay[i] travels with keys[i] (ptmp the same size; result in pay).  cnt, off: 256 * AUC_SORT_BLOCKS entries each.
inline int auc_sort(hipStream_t st, uint32_t* keys, uint32_t* tmp, uint64_t count, uint32_t* cnt, uint64_t* off,
                    uint32_t* pay = nullptr, uint32_t* ptmp = nullptr) {
  if (count < 2) return 0;
  uint64_t tile = (count + AUC_SORT_BLOCKS - 1) / AUC_SORT_BLOCKS;
  tile = (tile + AUC_SORT_TILE - 1) / AUC_SORT_TILE * AUC_SORT_TILE;
  const int nb = (int)((count + tile - 1) / tile);
  uint32_t *src = keys, *dst = tmp, *psrc = pay, *pdst = ptmp;
  for (int shift = 0; shift < 32; shift += 8) {
    k_auc_digit_count<<<nb, AUC_THREADS, 0, st>>>(src, count, tile, shift, nb, cnt);
    k_auc_digit_scan<<<1, 1024, 0, st>>>(cnt, 256 * nb, off);
    if (pay) k_auc_digit_scatter<true><<<nb, AUC_THREADS, 0, st>>>(src, dst, psrc, pdst, count, tile, shift, nb, off);
    else k_auc_digit_scatter<false><<<nb, AUC_THREADS, 0, st>>>(src, dst, nullptr, nullptr, count, tile, shift, nb, off);
    uint32_t* x = src; src = dst; dst = x;
    x = psrc; psrc = pdst; pdst = x;
  }
  MCGRA_KERNEL_CHECK();
  return 0;                                         // four passes: the sorted keys are back in `keys`
}
}  // namespace
}  // namespace mcgra
