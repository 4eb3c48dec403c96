// Skinny products on the learnable adjacency, Y [n x c] = M V (c <= 48), in a form that runs BESIDE the N x N x N product
// of the fused step (split2_m16_kernel: 128 of 160 KB LDS and 384 of 512 VGPRs per SIMD lane slot, bound by the 16-bit
// matrix pipe).  gemm_f32_kernel, which the forward used before, has neither property: its blocks hold two 64 KB LDS stages
// and run on the fp32 matrix pipe at 1/16 of the 16-bit rate -- a block of it cannot sit beside a product block.
//
// Here both operands are split exactly into three bf16 planes, x = x0 + x1 + x2 (8 significant bits each, fp32's exponent
// range: no scale), and the six plane products with i + j <= 2 are summed in the fp32 accumulator of
// v_mfma_f32_16x16x32_bf16, smallest first (representation error 2^-24 per operand: the fp32 GEMM's error class).
//   - one block of 256 threads = one wave per SIMD, at most one block per CU (grid-stride over its tasks), no LDS,
//     <= 128 VGPRs (arch + acc) per lane: it fits beside a product block;
//   - the left operand streams from M (fp32, one pass over 4 bytes per entry -- HBM-bound), split in registers; the right
//     operand is packed once per product (k_sx_vpack) in the fragment order of the MFMA and read through L1 / L2;
//   - output: split-K slabs [ksplit][n][NC] in a fixed order, summed by their consumers in slab order (YView), as
//     sgemm / planes_mm leave them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace mcgra {

namespace {
typedef float f32x4s __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8s __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4s __attribute__((ext_vector_type(4)));

constexpr int SX_WAVES = 4;        // one wave per SIMD

__device__ __forceinline__ void sx_split(const float (&x)[8], bf16x8s& p0, bf16x8s& p1, bf16x8s& p2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 b0 = (__bf16)x[j];
    const float r1 = x[j] - (float)b0;              // exact
    const __bf16 b1 = (__bf16)r1;
    const float r2 = r1 - (float)b1;                // exact, and exactly a bf16
    p0[j] = b0; p1[j] = b1; p2[j] = (__bf16)r2;
  }
}

// V [n x nc] as three bf16 planes in fragment order: [k step of 32][plane (3)][k octet (4)][column (NC)][8 k]
__global__ __launch_bounds__(256) void k_sx_vpack(int n, int nc, int NC, const float* __restrict__ V, int ldv, char* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;              // (k octet, column)
  const int col = e % NC, oct = e / NC;
  if (oct >= ((n + 31) / 32) * 4) return;
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = oct * 8 + j;
    x[j] = (k < n && col < nc) ? V[(size_t)k * ldv + col] : 0.f;
  }
  bf16x8s p0, p1, p2;
  sx_split(x, p0, p1, p2);
  const int s = oct >> 2, g = oct & 3;
  char* base = out + (size_t)s * (3 * 4 * NC * 16) + (size_t)g * (NC * 16) + (size_t)col * 16;
  *reinterpret_cast<bf16x8s*>(base) = p0;
  *reinterpret_cast<bf16x8s*>(base + 4 * NC * 16) = p1;
  *reinterpret_cast<bf16x8s*>(base + 2 * 4 * NC * 16) = p2;
}

// A task: R 16-row tiles per wave (16 R SX_WAVES rows per block) x all NC = 16 NCT columns x the K steps [ks kper, ...).
// Lane (row l & 15, k octet l >> 4) of a tile loads its 8 consecutive k of M as two 16-byte loads; the next K step's
// left operand and right-hand side are in flight while this one's MFMAs issue.
template <int R, int NCT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_skinny_x3(
    int n, const float* __restrict__ M, int ldm, const char* __restrict__ Vp, float* __restrict__ slabs, size_t slab_stride,
    int nks, int kper, int ksplit, int ntask) {
  constexpr int NC = 16 * NCT, STEPV = 3 * 4 * NC * 16, PLANE = 4 * NC * 16, ROWS = 16 * R * SX_WAVES;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
  auto ldv = [](const char* p) { return __builtin_bit_cast(bf16x8s, *reinterpret_cast<const u32x4s*>(p)); };
  for (int task = blockIdx.x; task < ntask; task += gridDim.x) {
    const int ks = task % ksplit, rb = task / ksplit;
    const int s0 = ks * kper, s1 = min(nks, s0 + kper);
    const int row0 = rb * ROWS + wave * 16 * R;
    const float* arow[R];
#pragma unroll
    for (int i = 0; i < R; ++i) arow[i] = M + (size_t)min(row0 + i * 16 + l15, n - 1) * ldm + lg * 8;      // (rows past n: a valid row, not stored)
    const char* vbase = Vp + (size_t)lg * (NC * 16) + (size_t)l15 * 16;
    auto load_a = [&](int s, float (&a)[R][8]) {
      const int k0 = s * 32 + lg * 8;
      if (k0 + 8 <= n) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const float4 u = *reinterpret_cast<const float4*>(arow[i] + s * 32), v = *reinterpret_cast<const float4*>(arow[i] + s * 32 + 4);
          a[i][0] = u.x; a[i][1] = u.y; a[i][2] = u.z; a[i][3] = u.w; a[i][4] = v.x; a[i][5] = v.y; a[i][6] = v.z; a[i][7] = v.w;
        }
      } else {      // the ragged last K step: nothing at or past column n is read
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) a[i][j] = k0 + j < n ? arow[i][s * 32 + j] : 0.f;
      }
    };
    auto load_b = [&](int s, bf16x8s (&b)[3][NCT]) {
      const char* bp = vbase + (size_t)s * STEPV;
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int j = 0; j < NCT; ++j) b[p][j] = ldv(bp + p * PLANE + j * 256);
    };
    f32x4s acc[R][NCT];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < NCT; ++j) acc[i][j] = f32x4s{0.f, 0.f, 0.f, 0.f};
    float a[R][8];
    bf16x8s b[3][NCT];
    if (s0 < s1) { load_a(s0, a); load_b(s0, b); }
    for (int s = s0; s < s1; ++s) {
      // this step's left operand into its planes, then the next step's in flight in the same registers; each column
      // tile's right-hand side is reloaded for the next step as soon as its six products have issued
      bf16x8s ap[R][3];
#pragma unroll
      for (int i = 0; i < R; ++i) sx_split(a[i], ap[i][0], ap[i][1], ap[i][2]);
      const bool more = s + 1 < s1;
      if (more) load_a(s + 1, a);
      const char* bp = vbase + (size_t)(s + 1) * STEPV;
#pragma unroll
      for (int j = 0; j < NCT; ++j) {
#pragma unroll
        for (int i = 0; i < R; ++i) {      // x2 y0 + x1 y1 + x0 y2 (2^-16), x1 y0 + x0 y1 (2^-8), then x0 y0
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[i][2], b[0][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[i][1], b[1][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[i][0], b[2][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[i][1], b[0][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[i][0], b[1][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[i][0], b[0][j], acc[i][j], 0, 0, 0);
        }
        if (more)
#pragma unroll
          for (int p = 0; p < 3; ++p) b[p][j] = ldv(bp + p * PLANE + j * 256);
      }
    }
    // C/D layout: col = lane & 15, row = 4 (lane >> 4) + q
    float* o = slabs + (size_t)ks * slab_stride;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = row0 + i * 16 + 4 * lg + q;
        if (row >= n) continue;
#pragma unroll
        for (int j = 0; j < NCT; ++j) o[(size_t)row * NC + j * 16 + l15] = acc[i][j][q];
      }
  }
}

int sx_cus() {
  static int cus[64] = {0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  if (cus[dev] <= 0) {
    int c = 0;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    cus[dev] = c;
  }
  return cus[dev];
}
// Y = the slabs summed in slab order (YView::at's sum), for callers that want the product itself
__global__ __launch_bounds__(256) void k_sx_sum(int n, int nc, YView v, float* __restrict__ Y, int ldy) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)n * nc) return;
  const int i = (int)(e / nc), c = (int)(e - (size_t)i * nc);
  Y[(size_t)i * ldy + c] = v.at(i, c);
}
}  // namespace

void skinny_x3_sum(hipStream_t st, int n, int nc, const YView& v, float* Y, int ldy) {
  hipLaunchKernelGGL(k_sx_sum, dim3((unsigned)(((size_t)n * nc + 255) / 256)), dim3(256), 0, st, n, nc, v, Y, ldy);
}

size_t skinny_x3_scratch_bytes(int n) { return (size_t)((n + 31) / 32) * (3 * 4 * 48 * 16); }
bool skinny_x3_supported(int n, int nc, int ldm) { return nc >= 1 && nc <= 48 && n >= 1 && ldm >= n && ldm % 4 == 0; }

// Y = M V, M [n x n] fp32 (leading dimension ldm, 16-byte aligned rows), V [n x nc] fp32.  scratch: skinny_x3_scratch_bytes(n)
// for the packed right-hand side; ws receives the split-K slabs; *out describes them.
hipError_t skinny_x3(hipStream_t st, int n, const float* M, int ldm, const float* V, int ldv, int nc, float* ws, size_t ws_bytes,
                     YView* out, void* scratch) {
  if (!skinny_x3_supported(n, nc, ldm) || ((uintptr_t)M & 15) != 0) return hipErrorInvalidValue;
  const int NC = nc <= 16 ? 16 : (nc <= 32 ? 32 : 48);
  const int R = 2;
  const int nks = (n + 31) / 32, rows = 16 * R * SX_WAVES, rblocks = (n + rows - 1) / rows;
  const int grid_max = sx_cus();
  // about four tasks per block: the blocks' shares even out beside a product whose rounds do not
  int ksplit = (4 * grid_max + rblocks - 1) / rblocks;
  if (ksplit > 64) ksplit = 64;
  if (ksplit > nks) ksplit = nks;
  const size_t stride = (size_t)n * NC;
  while (ksplit > 1 && (size_t)ksplit * stride * sizeof(float) > ws_bytes) --ksplit;
  if ((size_t)ksplit * stride * sizeof(float) > ws_bytes) return hipErrorInvalidValue;
  const int kper = (nks + ksplit - 1) / ksplit;
  ksplit = (nks + kper - 1) / kper;      // (no empty slab: every slab is written in full)
  const int ntask = rblocks * ksplit, grid = ntask < grid_max ? ntask : grid_max;
  char* vp = (char*)scratch;
  const int octs = nks * 4;
  hipLaunchKernelGGL(k_sx_vpack, dim3((octs * NC + 255) / 256), dim3(256), 0, st, n, nc, NC, V, ldv, vp);
#define MCGRA_SX(R_, NCT_)                                                                                                         \
  hipLaunchKernelGGL((k_skinny_x3<R_, NCT_>), dim3(grid), dim3(64 * SX_WAVES), 0, st, n, M, ldm, (const char*)vp, ws, stride, nks, kper, \
                     ksplit, ntask)
  if (NC == 16) MCGRA_SX(2, 1);
  else if (NC == 32) MCGRA_SX(2, 2);
  else MCGRA_SX(2, 3);
#undef MCGRA_SX
  *out = YView{ws, NC, ksplit, stride};
  return hipGetLastError();
}

}  // namespace mcgra
