// The host side the ranking entries share (declared in rank_common.h), and its kernels:
//   k_auc_index        idx only: range check, repeats (rank_check_idx)
//   k_auc_digit_count  per tile of keys, the 256 counts of one 8-bit digit
//   k_auc_digit_scan   one block: the running sum of up to 2^18 counts (rank_scan; the sort's (digit, tile) counts)
//   k_auc_digit_scatter  the stable scatter of a tile by digit
// and the checks of the arguments, the table from flag bits to refusals and the tile rule.
#include "rank_common.h"

#include <algorithm>

namespace mcgra {

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

int rank_check_args(const char* who, int n, std::initializer_list<RankMat> mats, const int64_t* idx, int64_t& n_idx, int min_idx,
                    int64_t cap) {
  if (!idx) n_idx = n;
  bool ok = n >= 1 && n_idx >= min_idx;
  for (const RankMat& m : mats) ok = ok && (m.p ? m.ld >= n : !m.required);
  if (!ok) {
    set_error("%s: bad argument (n >= 1, the matrices not NULL, every ld >= n, at least %d selected nodes)", who, min_idx);
    return MCGRA_EINVAL;
  }
  if (n_idx > cap) {
    set_error("%s: %lld selected nodes; more than %lld are not supported", who, (long long)n_idx, (long long)cap);
    return MCGRA_ENOSUP;
  }
  return 0;
}

int rank_check_idx(const char* who, hipStream_t st, AucBufs& b, int n, const int64_t* idx, int64_t rows, int* flags,
                   bool allow_repeats, bool* repeated) {
  if (!idx) return 0;
  uint32_t* seen = b.get<uint32_t>(n);
  if (!seen) { set_error("%s: hipMalloc failed", who); return MCGRA_ENOMEM; }
  MCGRA_HIP(hipMemsetAsync(seen, 0, sizeof(uint32_t) * (size_t)n, st));
  const int g = (int)std::min<int64_t>(1024, (rows + AUC_THREADS - 1) / AUC_THREADS);
  k_auc_index<<<g, AUC_THREADS, 0, st>>>(n, rows, idx, seen, flags);
  MCGRA_KERNEL_CHECK();
  int f = 0;
  MCGRA_HIP(hipMemcpyAsync(&f, flags, sizeof(int), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  if (f & AUC_BAD_INDEX) { set_error("%s: a node id outside [0, %d)", who, n); return MCGRA_EINVAL; }
  if ((f & AUC_REPEAT) && !allow_repeats) {
    set_error("%s: idx names a node twice (a pair of a node with itself)", who);
    return MCGRA_EINVAL;
  }
  if (repeated) *repeated = (f & AUC_REPEAT) != 0;
  return 0;
}

int rank_flag_error(const char* who, int flags, bool paired) {
  if (flags & AUC_BAD_FACTOR) { set_error("%s: an entry of Z is NaN or infinite", who); return MCGRA_EINVAL; }
  const int bad = flags & (AUC_BAD_SCORE | AUC_BAD_LABEL | (paired ? DL_BAD_SCORE_B : 0));
  if (!bad) return 0;
  set_error("%s: %s%s%s", who,
            !(bad & AUC_BAD_SCORE) ? "" : paired ? "a selected score of scores_a is NaN or infinite "
                                                 : "a selected score is NaN or infinite ",
            (bad & DL_BAD_SCORE_B) ? "a selected score of scores_b is NaN or infinite " : "",
            (bad & AUC_BAD_LABEL) ? "a selected label is neither 0 nor 1" : "");
  return MCGRA_EINVAL;
}

RankTiles rank_tiles(uint64_t count, int max_blocks, int step) {
  uint64_t tile = (count + max_blocks - 1) / max_blocks;
  tile = std::max<uint64_t>(1, (tile + step - 1) / step) * step;
  return {tile, (int)((count + tile - 1) / tile)};
}

void rank_scan(hipStream_t st, const uint32_t* cnt, int len, uint64_t* off) {
  k_auc_digit_scan<<<1, 1024, 0, st>>>(cnt, len, off);
}

int auc_sort(hipStream_t st, uint32_t* keys, uint32_t* tmp, uint64_t count, const SortScratch& ss, uint32_t* pay, uint32_t* ptmp,
             int bits) {
  if (count < 2) return 0;
  const auto [tile, nb] = rank_tiles(count, AUC_SORT_BLOCKS, AUC_SORT_TILE);      // 256 nb <= AUC_SORT_COUNTS
  uint32_t* cnt = ss.cnt;
  uint64_t* off = ss.off;
  uint32_t *src = keys, *dst = tmp, *psrc = pay, *pdst = ptmp;
  for (int shift = 0; shift < bits; shift += 8) {
    k_auc_digit_count<<<nb, AUC_THREADS, 0, st>>>(src, count, tile, shift, nb, cnt);
    rank_scan(st, cnt, 256 * nb, off);
    if (pay) k_auc_digit_scatter<true><<<nb, AUC_THREADS, 0, st>>>(src, dst, psrc, pdst, count, tile, shift, nb, off);
    else k_auc_digit_scatter<false><<<nb, AUC_THREADS, 0, st>>>(src, dst, nullptr, nullptr, count, tile, shift, nb, off);
    uint32_t* x = src; src = dst; dst = x;
    x = psrc; psrc = pdst; pdst = x;
  }
  MCGRA_KERNEL_CHECK();
  return 0;                                         // bits = 32, four passes: the sorted keys are back in `keys`
}

}  // namespace mcgra
