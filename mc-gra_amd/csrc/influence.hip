// The LinkTeller influence attack (mcgra_influence_scores): Wu et al., "LinkTeller: Recovering Private Edges from Graph Neural
// Networks via Influence Analysis" (IEEE S&P 2022).  I[v -> u] = || O(X with row v scaled by 1 + Delta)_u - O(X)_u ||_2 / Delta for
// every ordered pair, O the victim's output (mcgra_gcn_forward), computed as a DIFFERENCE carried along the graph's support:
//   dT^0 = Delta (x_v W_0) on row v alone;  dP^l_u = sum_{w in F_l(v), ascending} a_uw dT^l_w;
//   dH^{l+1}_u = P > 0 ? max(dP, -P) : max(P + dP, 0)   (= relu(P + dP) - relu(P) with no cancellation, P the kept base value);
//   dT^{l+1} = dH^{l+1} W_{l+1};  dZ = dH^L Wlin^T;  dlogp_k = dZ_k - log1p(sum_j p_j expm1(dZ_j));  dp_k = p_k expm1(dlogp_k).
// F_0 = {v}, F_{l+1} = the nodes with a non-zero cell towards F_l: one source touches its L-hop neighbourhood only.
//
// Passes:
//   the base forward with the library's own products (sgemm, launch_bias_relu, launch_rowmat, launch_log_softmax), every P^l kept,
//     and T^0 = X W_0;  k_inf_finite over X, the weights, T^0, every P^l and the base output
//   k_inf_row_count / k_inf_row_fill   the row lists of adj (ids ascending, values): one wave a row, wave64 ballots; the first also
//     checks adj's finiteness and counts the non-zeros, the host scans the n counts in between
//   k_inf_sym_check  every listed (u, w) has (w, u) listed: a binary search in w's list
//   k_influence      persistent workgroups of 4 waves, workgroup g takes the sources g, g + G, ...; the frontier is two n-bit masks in
//     LDS (integer atomicOr), dT lives per node id in the workgroup's two slabs of global scratch [n][hs] (layer parity), read only at
//     members of F_l -- all written for this source -- so a slab is never cleaned; one wave computes one target row, lane c owns
//     hidden column c, the neighbour sum walks the row list of u in ascending w and keeps the members of F_l (a ballot per 64
//     entries); dH crosses lanes by __shfl; W_1 .. W_{L-1} and Wlin are staged in LDS when they fit INF_W_LDS_BYTES, else read in
//     place.  The source's output row is written once: +0.0 outside F_L, the value inside.
//   k_inf_symmax     s_ab = max(I[a -> b], I[b -> a]) in place, a 64 x 64 tile and its mirror per block through LDS
// Every sum has a fixed order (ascending w, c, k) and nothing but integers is merged atomically: the same bits on every call and
// every grid.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../include/mcgra.h"
#include "common.h"
#include "kernels.h"

namespace mcgra {
namespace {
constexpr int INF_THREADS = 256;                          // 4 waves
constexpr int INF_WAVES = INF_THREADS / 64;
constexpr int INF_MAX_N = 65535;
constexpr int INF_W_LDS_BYTES = 40 * 1024;                // W_1 .. W_{L-1} and Wlin in LDS up to this; beyond: read in place
constexpr size_t INF_SLAB_BUDGET = (size_t)512 << 20;     // the workgroups' slabs together stay below this
constexpr int INF_TILE = 64;

enum { INF_BAD_VALUE = 1, INF_BAD_SUPPORT = 2 };

struct InfState {
  unsigned long long reached;
  int max_reach;
  int flags;
};

struct InfBufs {
  std::vector<void*> p;
  ~InfBufs() { for (void* q : p) (void)hipFree(q); }
  template <typename T>
  T* get(size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    p.push_back(q);
    return (T*)q;
  }
};

struct InfParams {
  int n, nlayer, nclass, hs;                // hs: the slabs' row stride, the widest layer
  int dims[MCGRA_MAX_LAYERS + 1];
  const int64_t* rowptr;
  const int32_t* ids;
  const float* vals;
  const float* T0;                          // [n][ldh]
  const float* P[MCGRA_MAX_LAYERS];         // [n][ldh] each
  int ldh;
  const float* W[MCGRA_MAX_LAYERS];         // W[l], l >= 1: [dims[l]][dims[l + 1]]
  const float* Wlin;                        // [nclass][dims[nlayer]]
  const float* O;                           // [n][nclass] base log-posteriors
  float delta;
  int output;
  int w_in_lds;
  float* slab;                              // [G][2][n][hs]
  float* out;
  int64_t ldo;
  InfState* st;
};

// the rows x cols values of x (row stride ld)
__global__ void k_inf_finite(const float* __restrict__ x, size_t rows, size_t cols, size_t ld, InfState* __restrict__ st) {
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * cols; i += (size_t)gridDim.x * blockDim.x)
    bad |= !isfinite(x[(i / cols) * ld + i % cols]);
  if (bad) atomicOr(&st->flags, INF_BAD_VALUE);
}

// one wave a row: cnt[u] = the non-zero cells of row u
__global__ __launch_bounds__(INF_THREADS) void k_inf_row_count(int n, const float* __restrict__ adj, int64_t lda,
                                                               int32_t* __restrict__ cnt, InfState* __restrict__ st) {
  const int lane = threadIdx.x & 63, u = blockIdx.x * INF_WAVES + (threadIdx.x >> 6);
  if (u >= n) return;
  const float* row = adj + (int64_t)u * lda;
  int c = 0;
  bool bad = false;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    const float a = j < n ? row[j] : 0.f;
    bad |= !isfinite(a);
    c += __popcll(__ballot(a != 0.f));
  }
  if (bad) atomicOr(&st->flags, INF_BAD_VALUE);
  if (lane == 0) cnt[u] = c;
}

__global__ __launch_bounds__(INF_THREADS) void k_inf_row_fill(int n, const float* __restrict__ adj, int64_t lda,
                                                              const int64_t* __restrict__ rowptr, int32_t* __restrict__ ids,
                                                              float* __restrict__ vals) {
  const int lane = threadIdx.x & 63, u = blockIdx.x * INF_WAVES + (threadIdx.x >> 6);
  if (u >= n) return;
  const float* row = adj + (int64_t)u * lda;
  int64_t at = rowptr[u];
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    const float a = j < n ? row[j] : 0.f;
    const unsigned long long m = __ballot(a != 0.f);
    if (a != 0.f) {
      const int64_t k = at + __popcll(m & ((1ull << lane) - 1ull));
      ids[k] = j;
      vals[k] = a;
    }
    at += __popcll(m);
  }
}

__global__ __launch_bounds__(INF_THREADS) void k_inf_sym_check(int n, const int64_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ ids, InfState* __restrict__ st) {
  const int lane = threadIdx.x & 63, u = blockIdx.x * INF_WAVES + (threadIdx.x >> 6);
  if (u >= n) return;
  bool bad = false;
  for (int64_t k = rowptr[u] + lane; k < rowptr[u + 1]; k += 64) {
    const int w = ids[k];
    int64_t lo = rowptr[w], hi = rowptr[w + 1];      // u in ids[lo, hi)?
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (ids[mid] < u) lo = mid + 1; else hi = mid;
    }
    bad |= lo >= rowptr[w + 1] || ids[lo] != u;
  }
  if (bad) atomicOr(&st->flags, INF_BAD_SUPPORT);
}

// the floats of W_1 .. W_{L-1} and Wlin, in that order: the LDS copy's layout
__host__ __device__ inline int inf_w_offset(const int* dims, int l) {
  int o = 0;
  for (int i = 1; i < l; ++i) o += dims[i] * dims[i + 1];
  return o;
}

__device__ __forceinline__ bool inf_bit(const uint32_t* m, int i) { return (m[i >> 5] >> (i & 31)) & 1u; }

// the sum of t over lanes 0 .. count - 1 in ascending lane order, in every lane
__device__ __forceinline__ float inf_ordered_sum(float t, int count) {
  float s = 0.f;
  for (int j = 0; j < count; ++j) s += __shfl(t, j, 64);
  return s;
}

__global__ __launch_bounds__(INF_THREADS) void k_influence(const InfParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = p.n, L = p.nlayer, nc = p.nclass;
  const int nw = (n + 31) >> 5, nwp = (nw + 3) & ~3;
  uint32_t* cur = (uint32_t*)smem;
  uint32_t* nxt = cur + nwp;
  int* red = (int*)(nxt + nwp);                     // INF_WAVES ints
  float* wl = (float*)(red + INF_WAVES);            // the staged weights (w_in_lds)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wtot = inf_w_offset(p.dims, L) + nc * p.dims[L];
  if (p.w_in_lds) {
    for (int l = 1; l < L; ++l) {
      float* dst = wl + inf_w_offset(p.dims, l);
      for (int e = tid; e < p.dims[l] * p.dims[l + 1]; e += INF_THREADS) dst[e] = p.W[l][e];
    }
    float* dst = wl + inf_w_offset(p.dims, L);
    for (int e = tid; e < nc * p.dims[L]; e += INF_THREADS) dst[e] = p.Wlin[e];
  }
  (void)wtot;
  const float* Wlin = p.w_in_lds ? wl + inf_w_offset(p.dims, L) : p.Wlin;
  float* slab = p.slab + (size_t)blockIdx.x * 2 * (size_t)n * p.hs;
  unsigned long long reached = 0;
  int max_reach = 0;
  __syncthreads();

  for (int v = blockIdx.x; v < n; v += gridDim.x) {
    for (int i = tid; i < nw; i += INF_THREADS) cur[i] = 0u;
    __syncthreads();
    if (tid == 0) cur[v >> 5] = 1u << (v & 31);
    if (tid < p.dims[1]) slab[(size_t)v * p.hs + tid] = p.delta * p.T0[(size_t)v * p.ldh + tid];
    for (int l = 0; l < L; ++l) {
      const bool last = l + 1 == L;
      const int hw = p.dims[l + 1];
      const float* sc = slab + (size_t)(l & 1) * n * p.hs;
      float* sn = slab + (size_t)((l + 1) & 1) * n * p.hs;
      for (int i = tid; i < nw; i += INF_THREADS) nxt[i] = 0u;
      __syncthreads();                              // cur, this layer's dT and the cleared nxt are in place
      for (int wi = wave; wi < nw; wi += INF_WAVES) {
        uint32_t m = cur[wi];
        while (m) {
          const int w = wi * 32 + __ffs(m) - 1;
          m &= m - 1;
          for (int64_t k = p.rowptr[w] + lane; k < p.rowptr[w + 1]; k += 64) {
            const int u = p.ids[k];
            atomicOr(&nxt[u >> 5], 1u << (u & 31));
          }
        }
      }
      __syncthreads();                              // nxt = F_{l+1}
      if (last) {
        int c = 0;
        for (int i = tid; i < nw; i += INF_THREADS) c += __popc(nxt[i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) red[wave] = c;
        float* orow = p.out + (int64_t)v * p.ldo;
        for (int u = tid; u < n; u += INF_THREADS)
          if (!inf_bit(nxt, u)) orow[u] = 0.f;
      }
      const float* Wn = last ? Wlin : (p.w_in_lds ? wl + inf_w_offset(p.dims, l + 1) : p.W[l + 1]);
      for (int wi = wave; wi < nw; wi += INF_WAVES) {
        uint32_t m = nxt[wi];
        while (m) {
          const int u = wi * 32 + __ffs(m) - 1;
          m &= m - 1;
          // dP_u[lane] over the members of F_l in u's list, ascending
          float acc = 0.f;
          const int64_t r0 = p.rowptr[u], r1 = p.rowptr[u + 1];
          for (int64_t k0 = r0; k0 < r1; k0 += 64) {
            const int64_t k = k0 + lane;
            int w = 0;
            float a = 0.f;
            bool member = false;
            if (k < r1) {
              w = p.ids[k];
              a = p.vals[k];
              member = inf_bit(cur, w);
            }
            unsigned long long bm = __ballot(member);
            while (bm) {
              const int j = __ffsll((long long)bm) - 1;
              bm &= bm - 1;
              const int ww = __shfl(w, j, 64);
              const float aa = __shfl(a, j, 64);
              if (lane < hw) acc = fmaf(aa, sc[(size_t)ww * p.hs + lane], acc);
            }
          }
          float dh = 0.f;
          if (lane < hw) {
            const float P = p.P[l][(size_t)u * p.ldh + lane];
            dh = P > 0.f ? fmaxf(acc, -P) : fmaxf(P + acc, 0.f);
          }
          if (!last) {
            const int wn = p.dims[l + 2];
            float t = 0.f;
            for (int c = 0; c < hw; ++c) {
              const float hc = __shfl(dh, c, 64);
              if (lane < wn) t = fmaf(hc, Wn[c * wn + lane], t);
            }
            if (lane < wn) sn[(size_t)u * p.hs + lane] = t;
          } else {
            float dz = 0.f;
            for (int c = 0; c < hw; ++c) {
              const float hc = __shfl(dh, c, 64);
              if (lane < nc) dz = fmaf(hc, Wn[lane * hw + c], dz);
            }
            const float pk = lane < nc ? expf(p.O[(size_t)u * nc + lane]) : 0.f;
            const float s = inf_ordered_sum(lane < nc ? pk * expm1f(dz) : 0.f, nc);
            const float dl = dz - log1pf(s);
            const float val = p.output == 0 ? dl : pk * expm1f(dl);
            const float ss = inf_ordered_sum(lane < nc ? val * val : 0.f, nc);
            if (lane == 0) p.out[(int64_t)v * p.ldo + u] = sqrtf(ss) / p.delta;
          }
        }
      }
      __syncthreads();                              // the next layer's dT is written; cur and nxt are free to swap
      uint32_t* t = cur; cur = nxt; nxt = t;
    }
    if (tid == 0) {
      int c = 0;
      for (int i = 0; i < INF_WAVES; ++i) c += red[i];
      reached += (unsigned long long)c;
      max_reach = c > max_reach ? c : max_reach;
    }
  }
  if (tid == 0) {
    atomicAdd(&p.st->reached, reached);
    atomicMax(&p.st->max_reach, max_reach);
  }
}

// out[a][b] = out[b][a] = max of the two, tile (I, J), J <= I, and its mirror
__global__ __launch_bounds__(INF_THREADS) void k_inf_symmax(int n, float* __restrict__ out, int64_t ldo) {
  __shared__ float A[INF_TILE][INF_TILE + 1], B[INF_TILE][INF_TILE + 1];
  const int I = blockIdx.y, J = blockIdx.x;
  if (J > I) return;
  const int bi = I * INF_TILE, bj = J * INF_TILE;
  const int tx = threadIdx.x & (INF_TILE - 1), ty = threadIdx.x / INF_TILE;
  for (int r = ty; r < INF_TILE; r += INF_THREADS / INF_TILE) {
    A[r][tx] = (bi + r < n && bj + tx < n) ? out[(int64_t)(bi + r) * ldo + bj + tx] : 0.f;
    B[r][tx] = (bj + r < n && bi + tx < n) ? out[(int64_t)(bj + r) * ldo + bi + tx] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < INF_TILE; r += INF_THREADS / INF_TILE) {
    if (bi + r < n && bj + tx < n) out[(int64_t)(bi + r) * ldo + bj + tx] = fmaxf(A[r][tx], B[tx][r]);
    if (I != J && bj + r < n && bi + tx < n) out[(int64_t)(bj + r) * ldo + bi + tx] = fmaxf(B[r][tx], A[tx][r]);
  }
}

int inf_fetch(hipStream_t st, const InfState* dev, InfState& h) {
  MCGRA_HIP(hipMemcpyAsync(&h, dev, sizeof(InfState), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  return 0;
}

void inf_check_finite(hipStream_t st, const float* x, size_t rows, size_t cols, size_t ld, InfState* state) {
  const unsigned blocks = (unsigned)std::min<size_t>((rows * cols + 255) / 256, 1024);
  k_inf_finite<<<blocks, 256, 0, st>>>(x, rows, cols, ld, state);
}
}  // namespace
}  // namespace mcgra

using namespace mcgra;

#define INF_NEED(ptr) \
  if (!(ptr)) { set_error("%s: hipMalloc failed", who); return MCGRA_ENOMEM; }

extern "C" int mcgra_influence_scores(void* stream, int n, int nfeat, int nlayer, const int32_t* dims, const float* X,
                                      const float* adj, int ld_adj, const float* const* W, const float* const* b,
                                      const float* Wlin, const float* blin, int nclass, double delta, int output, int symmetrize,
                                      float* out, int ld_out, int64_t* counts) {
  const char* who = "influence_scores";
  const float dl = (float)delta;
  bool ok = n >= 1 && nfeat >= 1 && nclass >= 1 && nlayer >= 1 && nlayer <= MCGRA_MAX_LAYERS && dims && X && adj && W && b && Wlin &&
            blin && out && counts && ld_adj >= n && ld_out >= n && std::isfinite(dl) && dl != 0.f && fabsf(dl) < 1.f &&
            (output == 0 || output == 1) && (symmetrize == 0 || symmetrize == 1);
  if (ok) {
    ok = dims[0] == nfeat;
    for (int l = 0; l < nlayer && ok; ++l) ok = dims[l + 1] >= 1 && W[l] && b[l];
  }
  if (!ok) {
    set_error("%s: bad argument (n, nfeat, nclass >= 1, 1 <= nlayer <= %d, dims[0] = nfeat and every width >= 1, no NULL pointer, "
              "every ld >= n, float32(delta) finite, not 0 and below 1 in magnitude, output and symmetrize 0 or 1)", who,
              MCGRA_MAX_LAYERS);
    return MCGRA_EINVAL;
  }
  int hmax = 1;
  for (int l = 0; l < nlayer; ++l) hmax = std::max(hmax, (int)dims[l + 1]);
  if (n > INF_MAX_N || hmax > MCGRA_INFLUENCE_MAX_WIDTH || nclass > MCGRA_INFLUENCE_MAX_WIDTH) {
    set_error("%s: n = %d, widest layer %d, nclass = %d: up to %d nodes and %d columns (one lane a column)", who, n, hmax, nclass,
              INF_MAX_N, MCGRA_INFLUENCE_MAX_WIDTH);
    return MCGRA_ENOSUP;
  }
  hipStream_t st = (hipStream_t)stream;
  const int L = nlayer;
  const int ldh = (std::max(hmax, nclass) + 3) & ~3;
  InfBufs s;
  InfState* state = s.get<InfState>(1); INF_NEED(state);
  MCGRA_HIP(hipMemsetAsync(state, 0, sizeof(InfState), st));
  // ---- the base forward (mcgra_gcn_forward's launches), every P^l kept
  float* T0 = s.get<float>((size_t)n * ldh); INF_NEED(T0);
  float* T = s.get<float>((size_t)n * ldh); INF_NEED(T);
  float* Yb = s.get<float>((size_t)n * ldh); INF_NEED(Yb);
  float* H = s.get<float>((size_t)n * ldh); INF_NEED(H);
  float* Z = s.get<float>((size_t)n * nclass); INF_NEED(Z);
  float* O = s.get<float>((size_t)n * nclass); INF_NEED(O);
  float* P[MCGRA_MAX_LAYERS];
  for (int l = 0; l < L; ++l) { P[l] = s.get<float>((size_t)n * ldh); INF_NEED(P[l]); }
  const size_t wsb = (size_t)64 * n * ldh * sizeof(float);
  float* ws = s.get<float>(wsb / sizeof(float)); INF_NEED(ws);
  int32_t* cnt = s.get<int32_t>(n); INF_NEED(cnt);
  int64_t* rowptr = s.get<int64_t>((size_t)n + 1); INF_NEED(rowptr);

  inf_check_finite(st, X, n, nfeat, nfeat, state);
  for (int l = 0; l < L; ++l) {
    inf_check_finite(st, W[l], dims[l], dims[l + 1], dims[l + 1], state);
    inf_check_finite(st, b[l], 1, dims[l + 1], dims[l + 1], state);
  }
  inf_check_finite(st, Wlin, nclass, dims[L], dims[L], state);
  inf_check_finite(st, blin, 1, nclass, nclass, state);
  const unsigned row_blocks = (unsigned)((n + INF_WAVES - 1) / INF_WAVES);
  k_inf_row_count<<<row_blocks, INF_THREADS, 0, st>>>(n, adj, ld_adj, cnt, state);
  MCGRA_KERNEL_CHECK();

  MCGRA_HIP(sgemm(st, false, false, n, dims[1], nfeat, 1.f, X, nfeat, W[0], dims[1], 0.f, T0, ldh, ws, wsb));
  for (int l = 0; l < L; ++l) {
    const int w = dims[l + 1];
    MCGRA_HIP(sgemm(st, false, false, n, w, n, 1.f, adj, ld_adj, l == 0 ? T0 : T, ldh, 0.f, Yb, ldh, ws, wsb));
    launch_bias_relu(st, n, w, Yb, ldh, b[l], nullptr, 0, 0, P[l], H, ldh);
    if (l + 1 < L) launch_rowmat(st, n, w, dims[l + 2], H, ldh, W[l + 1], dims[l + 2], 1, nullptr, T, ldh);
  }
  launch_rowmat(st, n, dims[L], nclass, H, ldh, Wlin, 1, dims[L], blin, Z, nclass);
  launch_log_softmax(st, n, nclass, Z, nclass, O, nullptr, nclass, 0);
  MCGRA_KERNEL_CHECK();
  // the base output and what is kept of the way to it: relu would hide a NaN pre-activation
  inf_check_finite(st, T0, n, dims[1], ldh, state);
  for (int l = 0; l < L; ++l) inf_check_finite(st, P[l], n, dims[l + 1], ldh, state);
  inf_check_finite(st, O, n, nclass, nclass, state);
  MCGRA_KERNEL_CHECK();

  std::vector<int32_t> hcnt(n);
  std::vector<int64_t> hptr((size_t)n + 1);
  MCGRA_HIP(hipMemcpyAsync(hcnt.data(), cnt, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  InfState h{};
  if (int rc = inf_fetch(st, state, h)) return rc;
  if (h.flags & INF_BAD_VALUE) {
    set_error("%s: a NaN or an infinity in adj, X, the weights or the victim's base output", who);
    return MCGRA_EINVAL;
  }
  hptr[0] = 0;
  for (int u = 0; u < n; ++u) hptr[u + 1] = hptr[u] + hcnt[u];
  const int64_t nnz = hptr[n];
  int32_t* ids = s.get<int32_t>((size_t)nnz);
  float* vals = s.get<float>((size_t)nnz);
  if (!ids || !vals) { set_error("%s: hipMalloc of the row lists (%lld entries) failed", who, (long long)nnz); return MCGRA_ENOMEM; }
  MCGRA_HIP(hipMemcpyAsync(rowptr, hptr.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  k_inf_row_fill<<<row_blocks, INF_THREADS, 0, st>>>(n, adj, ld_adj, rowptr, ids, vals);
  k_inf_sym_check<<<row_blocks, INF_THREADS, 0, st>>>(n, rowptr, ids, state);
  MCGRA_KERNEL_CHECK();
  if (int rc = inf_fetch(st, state, h)) return rc;      // (hptr stays alive past the copy: the fetch synchronises)
  if (h.flags & INF_BAD_SUPPORT) {
    set_error("%s: adj's support is not symmetric (a_uw != 0 without a_wu != 0)", who);
    return MCGRA_EINVAL;
  }

  // ---- the sources
  int dev = 0, cus = 0;
  MCGRA_HIP(hipGetDevice(&dev));
  MCGRA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const size_t slab_bytes = (size_t)2 * n * hmax * sizeof(float);
  long long G = std::min<long long>(n, 2LL * std::max(cus, 1));
  G = std::max<long long>(1, std::min<long long>(G, (long long)(INF_SLAB_BUDGET / slab_bytes)));
  if (const char* e = getenv("MCGRA_INFLUENCE_GROUPS")) {
    const long long want = atoll(e);
    if (want >= 1) G = std::min<long long>(want, G);
  }
  float* slab = s.get<float>((size_t)G * 2 * n * hmax);
  if (!slab) { set_error("%s: hipMalloc of %lld slabs of %zu bytes failed", who, G, slab_bytes); return MCGRA_ENOMEM; }
  InfParams p{};
  p.n = n; p.nlayer = L; p.nclass = nclass; p.hs = hmax;
  for (int l = 0; l <= L; ++l) p.dims[l] = dims[l];
  p.rowptr = rowptr; p.ids = ids; p.vals = vals;
  p.T0 = T0; p.ldh = ldh;
  for (int l = 0; l < L; ++l) { p.P[l] = P[l]; p.W[l] = W[l]; }
  p.Wlin = Wlin; p.O = O;
  p.delta = dl; p.output = output;
  p.slab = slab; p.out = out; p.ldo = ld_out; p.st = state;
  const int nwp = (((n + 31) >> 5) + 3) & ~3;
  const size_t wbytes = ((size_t)inf_w_offset(p.dims, L) + (size_t)nclass * dims[L]) * sizeof(float);
  p.w_in_lds = wbytes <= (size_t)INF_W_LDS_BYTES;
  const size_t lds = (size_t)2 * nwp * sizeof(uint32_t) + INF_WAVES * sizeof(int) + (p.w_in_lds ? wbytes : 0);
  k_influence<<<(unsigned)G, INF_THREADS, lds, st>>>(p);
  MCGRA_KERNEL_CHECK();
  if (symmetrize) {
    const unsigned nt = (unsigned)((n + INF_TILE - 1) / INF_TILE);
    k_inf_symmax<<<dim3(nt, nt), INF_THREADS, 0, st>>>(n, out, ld_out);
    MCGRA_KERNEL_CHECK();
  }
  if (int rc = inf_fetch(st, state, h)) return rc;
  counts[0] = nnz;
  counts[1] = (int64_t)h.reached;
  counts[2] = (int64_t)h.max_reach;
  return 0;
}
