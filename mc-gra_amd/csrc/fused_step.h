// The fused step of attack_fused.hip as its stages see it: the context every stage takes, and the driver of a stage table.
#pragma once
#include "engine.h"

// ---- a row-block rank's exchange stage: the kernels that move own rows in and gathered rows out, the views, the descriptors
namespace mcgra {
// stage[i][c0 + k] = src[i][k] for rows [row0, row1), k < w      (own rows of an n-vector block into the exchange stage)
__global__ void k_rows_to_stage(int row0, int row1, int w, const float* __restrict__ src, int lds_, float* __restrict__ stage,
                                int sgw, int c0) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (row1 - row0) * w) return;
  const int i = row0 + e / w, k = e % w;
  stage[(size_t)i * sgw + c0 + k] = src[(size_t)i * lds_ + k];
}
__global__ void k_stage_to_rows(int n, int w, const float* __restrict__ stage, int sgw, int c0, float* __restrict__ dst, int ldd) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * w) return;
  const int i = e / w, k = e % w;
  dst[(size_t)i * ldd + k] = stage[(size_t)i * sgw + c0 + k];
}
// all-to-all of P1 tile blocks: block s of the send buffer = P1[rows of rank s][own columns] (a rank computed the column
// block P1[:, own rows]); block s of the receive buffer = P1[own rows][columns of rank s].  One launch each instead of
// `world` strided copies.  A2[s][q][c], q, c < rpr.
__global__ void k_a2a_pack(int n, int ld, int rpr, int R0, int R1, int self, const float* __restrict__ KX, float* __restrict__ A2) {
  const int s = blockIdx.z, q = blockIdx.y, row = s * rpr + q;
  if (row >= n || s == self) return;                     // (the own block stays where it is -- and may still be in the making)
  const float* src = KX + (size_t)row * ld + R0;
  float* dst = A2 + ((size_t)s * rpr + q) * rpr;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < R1 - R0; c += gridDim.x * blockDim.x) dst[c] = src[c];
}
__global__ void k_a2a_unpack(int n, int ld, int rpr, int R0, int R1, int self, const float* __restrict__ A2, float* __restrict__ KX) {
  const int s = blockIdx.z, q = blockIdx.y;
  if (s == self || R0 + q >= R1) return;                 // (the own block is already in place)
  const int c0 = s * rpr, cw = min(rpr, n - c0);
  if (cw <= 0) return;
  const float* src = A2 + ((size_t)s * rpr + q) * rpr;      // peer s packed its KX[my rows, its columns]
  float* dst = KX + (size_t)(R0 + q) * ld + c0;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < cw; c += gridDim.x * blockDim.x) dst[c] = src[c];
}
// two n-vector blocks in one launch each way (r | d; decode backward | |xc_i|^2): a row-block rank's step is a chain of
// launches of a few microseconds, every one of them on its critical path
__global__ void k_rows_to_stage2(int row0, int row1, int w0, const float* __restrict__ s0, int l0, int c0, int w1,
                                 const float* __restrict__ s1, int l1, int c1, float* __restrict__ stage, int sgw) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x, wt = w0 + w1;
  if (e >= (row1 - row0) * wt) return;
  const int i = row0 + e / wt, k = e % wt;
  stage[(size_t)i * sgw + (k < w0 ? c0 + k : c1 + k - w0)] = k < w0 ? s0[(size_t)i * l0 + k] : s1[(size_t)i * l1 + k - w0];
}
__global__ void k_stage_to_rows2(int n, const float* __restrict__ stage, int sgw, int w0, int c0, float* __restrict__ d0, int l0,
                                 int w1, int c1, float* __restrict__ d1, int l1) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x, wt = w0 + w1;
  if (e >= n * wt) return;
  const int i = e / wt, k = e % wt;
  if (k < w0) d0[(size_t)i * l0 + k] = stage[(size_t)i * sgw + c0 + k];
  else d1[(size_t)i * l1 + k - w0] = stage[(size_t)i * sgw + c1 + k - w0];
}
// The scalar lane of an exchanged node array: two float columns that hold one double per row.  Rank k leaves its partial
// sum q in row k * rpr + q of its own chunk; behind the all-gather every rank adds the `world` partials in rank order --
// the same bits on every rank, and no all-reduce.
__global__ void k_lane_sum(int world, int rpr, int ldw, const float* __restrict__ lane, int nq, double* __restrict__ out) {
  const int q = threadIdx.x;
  if (q >= nq) return;
  double s = 0.0;
  for (int k = 0; k < world; ++k) s += *reinterpret_cast<const double*>(lane + ((size_t)k * rpr + q) * ldw);
  out[q] = s;
}
}  // namespace mcgra

static inline dim3 g1(size_t count) { return dim3((unsigned)((count + 255) / 256)); }
// The two exchanged node arrays of a row-block rank (views into its arena): WIDE = [product columns (fcols) | n-vector
// columns | scalar lane], the result of a skinny product on M together with whatever n-vectors and partial scalars are
// ready at the same point of the step; NARROW = [n-vector columns | scalar lane] for the exchanges without a product.
struct Stage { float* base; int ld, vec0, lane0; };
static inline Stage wide_stage(const mcgra_attack* h) { return Stage{h->FY, h->p.fyw, h->p.fcols, h->p.fyw - 2}; }
static inline Stage narrow_stage(const mcgra_attack* h) { return Stage{h->SG, h->p.sgw, 0, h->p.sgw - 2}; }
static inline void rows_to_stage(mcgra_attack* h, hipStream_t st, const Stage& sg, int w, const float* src, int lds_, int c0) {
  if (h->p.row1 > h->p.row0)
    hipLaunchKernelGGL(mcgra::k_rows_to_stage, g1((size_t)(h->p.row1 - h->p.row0) * w), dim3(256), 0, st, h->p.row0, h->p.row1, w, src, lds_, sg.base, sg.ld,
                       sg.vec0 + c0);
}
static inline void rows_to_stage2(mcgra_attack* h, hipStream_t st, const Stage& sg, int w0, const float* s0, int l0, int c0, int w1,
                           const float* s1, int l1, int c1) {
  if (h->p.row1 > h->p.row0)
    hipLaunchKernelGGL(mcgra::k_rows_to_stage2, g1((size_t)(h->p.row1 - h->p.row0) * (w0 + w1)), dim3(256), 0, st, h->p.row0, h->p.row1, w0, s0, l0,
                       sg.vec0 + c0, w1, s1, l1, sg.vec0 + c1, sg.base, sg.ld);
}
static inline void stage_to_rows2(mcgra_attack* h, hipStream_t st, const Stage& sg, int w0, int c0, float* d0, int l0, int w1, int c1,
                           float* d1, int l1) {
  hipLaunchKernelGGL(mcgra::k_stage_to_rows2, g1((size_t)h->p.n * (w0 + w1)), dim3(256), 0, st, h->p.n, sg.base, sg.ld, w0, sg.vec0 + c0, d0, l0, w1,
                     sg.vec0 + c1, d1, l1);
}
static inline void stage_to_rows(mcgra_attack* h, hipStream_t st, const Stage& sg, int w, int c0, float* dst, int ldd) {
  hipLaunchKernelGGL(mcgra::k_stage_to_rows, g1((size_t)h->p.n * w), dim3(256), 0, st, h->p.n, w, sg.base, sg.ld, sg.vec0 + c0, dst, ldd);
}
// slot q of this rank's scalar lane (a double)
static inline double* lane_slot(const mcgra_attack* h, const Stage& sg, int q) {
  return reinterpret_cast<double*>(sg.base + ((size_t)h->p.rank * h->p.rpr + q) * sg.ld + sg.lane0);
}
static inline int lane_zero(mcgra_attack* h, hipStream_t st, const Stage& sg, int nq) {
  MCGRA_HIP(hipMemset2DAsync(lane_slot(h, sg, 0), (size_t)sg.ld * 4, 0, 8, nq, st));
  return 0;
}
static inline void lane_sum(mcgra_attack* h, hipStream_t st, const Stage& sg, int nq, double* out) {
  hipLaunchKernelGGL(mcgra::k_lane_sum, dim3(1), dim3(64), 0, st, h->p.world, h->p.rpr, sg.ld, sg.base + sg.lane0, nq, out);
}

// ---- exchange descriptors (all offsets are bytes from the arena base) ---------------------------------------------------
static inline void x_allgather(mcgra_exchange_t* ex, int64_t off, int64_t chunk_bytes) {
  ex->kind = MCGRA_XCHG_ALLGATHER; ex->count = 0; ex->offset = off; ex->offset2 = 0; ex->chunk_bytes = chunk_bytes;
}
static inline void x_allreduce(mcgra_exchange_t* ex, int64_t off, int count) {
  ex->kind = MCGRA_XCHG_ALLREDUCE_F64; ex->count = count; ex->offset = off; ex->offset2 = 0; ex->chunk_bytes = 0;
}
static inline void x_alltoall(mcgra_exchange_t* ex, int64_t off_send, int64_t off_recv, int64_t chunk_bytes) {
  ex->kind = MCGRA_XCHG_ALLTOALL; ex->count = 0; ex->offset = off_send; ex->offset2 = off_recv; ex->chunk_bytes = chunk_bytes;
}

// The constants of a step, for its stages.  Built at the top of every entry (fused_ctx: on a row-block rank once per
// exchange) and never carried across one: what must survive an exchange lives in the handle (engine.h, fs_*).
struct FusedStep {
  mcgra_attack* h;
  hipStream_t st;
  mcgra_exchange_t* ex;      // a row-block rank's stage that ends at an exchange describes it here (monolithic: NULL, never written)
  int n, ld, hs, L, Le, C, fc, R0, R1;
  mcgra::FusedKind kind;     // which fused step this is (the plan's p.fused): stated here once, read by every stage and passed to the launchers
  bool elementwise() const { return kind == mcgra::FUSED_MSE || kind == mcgra::FUSED_KL; }      // (the plan's wording: attack_plan.h)
  bool kl() const { return kind == mcgra::FUSED_KL; }
  bool use1, use2, use9, use10;
  double sg, k1, k2, k6, k7, k9, k10, n2;
  float kmse1, kmse2, a1, a2;
  const float* em;           // the embedding chain's last activations, width he
  int he, p_off, p_cnt, nt;
  bool pair, ovl, want_vals, zero_inline;
  hipStream_t s3;
};
static inline FusedStep fused_ctx(mcgra_attack* h, hipStream_t st, mcgra_exchange_t* ex) {
  const mcgra_attack_config_t& c = h->cfg;
  FusedStep s{};
  s.h = h; s.st = st; s.ex = ex;
  s.n = h->p.n; s.ld = h->p.ld; s.hs = h->p.hsum; s.L = h->p.L; s.Le = h->p.Le; s.C = h->p.C; s.fc = h->p.fcols; s.R0 = h->p.row0; s.R1 = h->p.row1;
  // measure == HSIC (sign -1: :217-220), or -- h->p.elementwise() -- MSELoss: no product (use1) and no low-rank factors (use2); its two
  // N x N terms are elementwise and live in the decode (d / d modified_adj1) and in the tail's first pass (d / d adj_norm)
  // -- h->p.kl() (also "an elementwise measure") -- calc_kl: the MSELoss step's data flow with per-row softmax
  // statistics in front of the decode (k_decode_stats: one more per-pair pass) and one more gather on a row-block rank
  s.kind = (mcgra::FusedKind)h->p.fused;
  const bool mse = s.elementwise(), kl = s.kl();
  s.sg = mse ? 1.0 : -1.0;
  const double w1 = c.w[0], w2 = c.w[1], w6 = c.w[5], w7 = c.w[6], w9 = c.w[8], w10 = c.w[9];
  s.k1 = w1 * 1000 * AP_C1; s.k2 = w2 * 100 * AP_C2; s.k6 = w6 * 100 * AP_C6; s.k7 = w7 * AP_C7;
  s.k9 = w9 * AP_C9; s.k10 = w10 * AP_C10; s.n2 = (double)s.n * s.n;
  s.use1 = !mse && w1 != 0; s.use2 = !mse && w2 != 0; s.use9 = w9 != 0; s.use10 = w10 != 0;
  // (TEST-ONLY mutation 3 drops the measure's per-pair terms c1 / c2 from the decode and the tail: both multipliers zero)
  const bool no_calc = h->test_mutate == 3;
  s.kmse1 = no_calc ? 0.f : kl ? (float)(s.k1 / s.n) : mse ? (float)(s.k1 * 2.0 / s.n2) : 0.f;      // k_loss_elem's multipliers; KL: k / batch (batchmean over rows)
  s.kmse2 = no_calc ? 0.f : kl ? (float)(s.k2 / s.n) : mse ? (float)(s.k2 * 2.0 / s.n2) : 0.f;
  s.em = h->Hu + h->p.off[s.Le - 1];
  s.he = h->p.wdt[s.Le - 1];
  s.a1 = s.use1 ? 2.f * (float)(s.sg * s.k1) : 0.f; s.a2 = s.use2 ? 2.f * (float)(s.sg * s.k2) : 0.f;
  const int P = mcgra::split3_panel();
  s.p_off = s.R0 / P; s.p_cnt = s.R1 > s.R0 ? (s.R1 - s.R0 + P - 1) / P : 0;
  s.nt = mcgra::fl_tail_tiles(s.n);
  s.pair = !h->p.sharded;
  // side streams: the product on st2, the small-operand terms on st3
  s.ovl = h->p.overlap;
  // reductions that only feed the returned loss terms are skipped when the caller did not ask for them (a row-block
  // rank keeps them: they ride in exchanges whose layout is fixed)
  s.want_vals = h->p.sharded || h->fs_want;
  // (the fused MSELoss step on a small graph: its small-operand terms are one launch each -- k_mse_small_fused -- and the fork and
  //  the join of a side stream cost the caller's stream more than the two launches do: Cora-shaped 0.214 -> 0.199 ms; KL's terms stay on
  //  their stream -- 0.270 against 0.284 inline as chains of four launches, 0.288 inline as one launch each (built, measured, removed);
  //  A/B MCGRA_MSE_SMALL_INLINE=0)
  s.s3 = (s.kind == mcgra::FUSED_MSE && !h->p.sharded && h->p.mse_small_inline && s.n < 4096) ? st : h->st3;
  s.zero_inline = s.s3 == st && !h->p.sharded;      // (see launch_row_normalize in fs_decode_stats)
  return s;
}

// A stage runs without interruption.  It returns GO, AT_XCHG (it ended at an exchange point: a row-block rank hands the
// collective it described to its caller and resumes with the next stage; a monolithic engine just goes on), REDO or an error.
// The next stage is the one behind it in the table unless the stage names another (`next` is h->fs_state or h->fw_state).
enum { GO = 0, AT_XCHG = 1, REDO = 2 };
typedef int (*FusedStage)(FusedStep&);
static inline int run_stages(FusedStep& s, const FusedStage* table, int count, int& next) {
  while (next < count) {
    const int rc = table[next++](s);
    if (rc == AT_XCHG ? s.h->p.sharded : rc != GO) return rc;
  }
  return GO;
}
// the two all-gathers a stage may end at: of the wide and of the narrow exchanged node array (attack_fused.hip: Stage)
static inline int xchg_fy(const FusedStep& s) {      // all-gather of the wide node array
  if (s.h->p.sharded) x_allgather(s.ex, s.h->off_fy, (int64_t)s.h->p.rpr * s.h->p.fyw * 4);
  return AT_XCHG;
}
static inline int xchg_sg(const FusedStep& s) {      // all-gather of the narrow node array
  if (s.h->p.sharded) x_allgather(s.ex, s.h->off_sg, (int64_t)s.h->p.rpr * s.h->p.sgw * 4);
  return AT_XCHG;
}
