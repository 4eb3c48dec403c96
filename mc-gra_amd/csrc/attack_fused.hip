// The low-rank HSIC step of the attack loop (topology_attack.py:161-298) evaluated from the learnable adjacency M and
// n-vectors only, monolithic or as one of `world` row-block ranks (section 6).  Same
// mathematics as the general step of attack.hip on a low-rank step (section 1b), different data flow: adj_norm =
// R (M + I) R, its centred copy Xc, modified_adj1 = offdiag relu(Zn Zn^T) and d loss / d adj_norm are never in HBM.
//
//   forward     one product Y = M [r o Tv_l | Tu_l (| r)] per GCN layer serves the victim chain on adj_norm, the
//               embedding / victim chain on M and (layer 0) the row sums of adj_norm, i.e. the centring means
//   product     P1 = (H Kf H) Xc from planes packed straight from M (split_symm_bf16.hip), forked onto the side stream
//   decode      mask count, entropy term of modified_adj1 and its backward from Zn (k_decode_fly)
//   low rank    T = Xc^T Vc and Q = Xc [W | W2] as products on M with column-centred right-hand sides
//   tail        k_tail_reduce (Gs = G + G^T per tile pair, reductions of the normalisation backward) and k_tail_adam
//
// The step is an ordered table of stages (FS_STAGES; the forward's: FW_STAGES) over a FusedStep context that is rebuilt on
// every entry; fs_state / fw_state hold the index of the next stage, and what lives across an exchange point lives in the
// handle.  A stage that ends at a collective describes it (x_allgather / x_alltoall): a row-block rank returns to the host
// layer there (mcgra_attack_shard_next) and continues with the next stage behind it; the monolithic engine runs the same
// stages straight through with the full row range.  Every N x N pass touches rows [row0, row1) only; node-level
// (n x h) work is replicated on all ranks.
// A step whose decode masks a pair (S_ij <= 0 off the diagonal) is handed back to the general path.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "engine.h"
#include "fused_step.h"

using namespace mcgra;

namespace mcgra {
// rowsum of per-block partial sums (float) in fp64: out[i] = sum_p part[i][p], rows [row0, row1)
__global__ __launch_bounds__(256) void k_rsq_fin(int row0, int row1, int np, const float* __restrict__ part, double* __restrict__ out) {
  const int i = row0 + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= row1) return;
  double s = 0.0;
  for (int p = lane; p < np; p += 64) s += (double)part[(size_t)i * np + p];
  s = wave_sum_d(s);
  if (lane == 0) out[i] = s;
}
// |xc_i|^2 of rows [row0, row1) from the per-block partials of an UNCENTRED pack (row sums psum, sums of squares psq) and the
// column means the forward left: sum_k (a_ik - m_i)^2 = sum a^2 - 2 m_i sum a + n m_i^2 -- an identity in m_i, whichever
// evaluation of the mean it is (fp64)
__global__ __launch_bounds__(256) void k_rsq_fin_unc(int row0, int row1, int n, int np, const float* __restrict__ psq,
                                                     const float* __restrict__ psum, const float* __restrict__ mean,
                                                     double* __restrict__ out) {
  const int i = row0 + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= row1) return;
  double s = 0.0, q = 0.0;
  for (int p = lane; p < np; p += 64) { s += (double)psum[(size_t)i * np + p]; q += (double)psq[(size_t)i * np + p]; }
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  const double m = (double)mean[i];
  if (lane == 0) out[i] = q - 2.0 * m * s + (double)n * m * m;
}
__global__ void k_u32_to_f64(const unsigned int* __restrict__ a, double* __restrict__ out) { out[0] = (double)a[0]; }
__global__ void k_u32x2_to_f64(const unsigned int* __restrict__ a, double* __restrict__ o0, double* __restrict__ o1) {
  o0[0] = (double)a[0]; o1[0] = (double)a[1];
}
// late mean: from the pack's per-block row sums / sums of squares of adj_norm (uncentred): rowsum_i = sum_p psum[i][p],
// mean_i = rowsum_i / n, |xc_i|^2 = sum_p psq[i][p] - rowsum_i^2 / n        (fp64)
__global__ __launch_bounds__(256) void k_mean_fin(int n, int np, const float* __restrict__ psum, const float* __restrict__ psq,
                                                  float* __restrict__ mean, double* __restrict__ rowsum, double* __restrict__ rsq) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  double s = 0.0, q = 0.0;
  for (int p = lane; p < np; p += 64) { s += (double)psum[(size_t)i * np + p]; if (psq) q += (double)psq[(size_t)i * np + p]; }
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  if (lane == 0) {
    rowsum[i] = s;
    mean[i] = (float)(s / (double)n);
    if (rsq) rsq[i] = q - s * s / (double)n;
  }
}
// operand-scale bound of the uncentred adj_norm: |r_i (M_ij + [i == j]) r_j| <= max r^2   (M in [0, 1], zero diagonal)
// (one block of 1024 threads, 16-byte loads: two or three loads per thread.  As 256 threads with one float per iteration it was
//  forty dependent round trips -- 80 us beside the forward's first product, in front of the pack on the product's stream.)
__global__ __launch_bounds__(1024) void k_rmax2(int n, const float* __restrict__ r, float* __restrict__ out) {
  __shared__ float shm[16];
  float m = 0.f;
  const int n4 = n >> 2;
  for (int i = threadIdx.x; i < n4; i += 1024) {
    const float4 v = reinterpret_cast<const float4*>(r)[i];
    m = fmaxf(fmaxf(m, fmaxf(v.x * v.x, v.y * v.y)), fmaxf(v.z * v.z, v.w * v.w));
  }
  for (int i = (n4 << 2) + threadIdx.x; i < n; i += 1024) m = fmaxf(m, r[i] * r[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = shm[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) t = fmaxf(t, shm[w]);
    out[0] = t;
  }
}
}  // namespace mcgra

bool fused_step_possible(const mcgra_attack* h) { return fused_ok(h); }

int64_t fused_exchange_bytes(const mcgra_attack* h) {
  if (!h->p.sharded) return 0;
  const int64_t a = 256;
  auto up = [&](int64_t x) { return (x + a - 1) / a * a; };
  return up((int64_t)h->p.npad * h->p.fyw * 4) + up((int64_t)h->p.npad * h->p.sgw * 4) + up(16 * 8) +
         2 * up((int64_t)h->p.world * h->p.rpr * h->p.rpr * 4) + up((int64_t)h->p.npad * h->p.ld * 4);
}

// Y rows [row0, row1) = M[rows, :] V      (V = FV [n x ncol]).  A row-block rank needs the result in FY (it is exchanged);
// a monolithic engine leaves a split-K product as its slabs and hands its consumers a view of them (h->fy).  fwd: one of the
// forward's products, which run beside the N x N x N product when it is forked behind the early pack (fwd_x3).
static int mm_rows(mcgra_attack* h, hipStream_t st, int ncol, bool fwd = false) {
  const int rows = h->p.row1 - h->p.row0;
  h->fy = YView{h->FY, h->p.sharded ? h->p.fyw : h->p.fcols, 1, 0};
  if (rows <= 0) return 0;
  if (h->p.sharded)      // into the product columns of the wide exchange stage
    return eg(h, st, false, false, rows, ncol, h->p.n, 1.f, h->M + (size_t)h->p.row0 * h->p.ld, h->p.ld, h->FV, h->p.fcols, 0.f,
              h->FY + (size_t)h->p.row0 * h->p.fyw, h->p.fyw);
  if (h->step.planes_valid && planes_mm_supported(h->p.n, ncol)) {      // beside the N x N x N product: from its own operand planes
    MCGRA_HIP(planes_mm(st, h->p.n, h->Bpack, split3_chunks(h->p.n, 2), h->amax + 1, h->FV, h->p.fcols, ncol, h->r, h->ws, h->ws_bytes, &h->fy,
                        h->pm_scratch));
    return 0;
  }
  if (fwd && h->p.fwd_x3 && late_mean(h)) {      // (a configuration decision, not a run-time one: monitor and step adoption stay bit-identical)
    MCGRA_HIP(skinny_x3(st, h->p.n, h->M, h->p.ld, h->FV, h->p.fcols, ncol, h->ws, h->ws_bytes, &h->fy, h->sx_scratch));
    return 0;
  }
  MCGRA_HIP(sgemm(st, false, false, rows, ncol, h->p.n, 1.f, h->M, h->p.ld, h->FV, h->p.fcols, 0.f, h->FY, h->p.fcols, h->ws, h->ws_bytes,
                  &h->fy));
  return 0;
}

static int fork_p1_early(const FusedStep& s);
// ---- the transitions of Carry (engine.h).  Nothing in flight: no HIP call.
// Everything a forward forked and left running is ordered in front of whatever the caller's stream does next.  (Kx and a rank's
// product never coexist: one is a monolithic engine's, the other a row-block rank's.)
int carry_wait(mcgra_attack* h, hipStream_t st) {
  const Carry& c = h->carry;
  if (c.early_pack) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_pack, 0));
  if (c.kx_early && h->p.gram_ovl && h->st2) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_first, 0));
  if (c.p1_early) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
  return 0;
}
// ... and its results dropped: forked by a forward whose step never came, or comes by another path
int carry_drop(mcgra_attack* h, hipStream_t st) {
  CHK(carry_wait(h, st));
  Carry& c = h->carry;
  c.early_pack = c.kx_early = c.p1_early = c.p1_first = false;
  c.p1_early_cut = c.p1_early_split = 0;
  h->step.p1_inflight = false;      // (the exception of StepScratch: it stands for the same product as p1_early)
  return 0;
}
void carry_forget(mcgra_attack* h, bool keep_skip_fused) {
  Carry& c = h->carry;
  c.fwd_cached = c.fused_fwd_valid = c.prep_valid = false;
  if (!keep_skip_fused) c.skip_fused = false;
}

// The operand pack on the product's stream, forked behind r (ev_r) and marked by ev_pack: the planes of panels [p_off, p_off +
// p_cnt) (-1: all) with their scale bound max r^2 and the per-block row partials psq / psum.  sums: |adj_changes|^2 and
// sum(modified_adj) ride on that stream as well, in front of ev_pack.
static int pack_on_side_stream(mcgra_attack* h, hipStream_t st, int p_off, int p_cnt, float* psq, float* psum, bool sums) {
  MCGRA_HIP(hipEventRecord(h->ev_r, st));
  MCGRA_HIP(hipStreamWaitEvent(h->st2, h->ev_r, 0));
  if (h->amax) hipLaunchKernelGGL(k_rmax2, dim3(1), dim3(1024), 0, h->st2, h->p.n, h->r, h->amax + 1);
  split3_pack_from_m(h->st2, h->p.n, h->p.ld, h->M, h->r, nullptr, h->Bpack, h->p.split_planes, h->amax ? h->amax + 1 : nullptr, p_off, p_cnt,
                     psq, psum);
  // (|adj_changes|^2 and sum(modified_adj): nothing of the forward needs them -- off the caller's stream too)
  if (sums) launch_reduce_rows(h->st2, h->rowsq, h->p.n, 2, h->scal + S_SQ);
  MCGRA_HIP(hipEventRecord(h->ev_pack, h->st2));
  return 0;
}

// ---- the forward's stages (FW_STAGES): d, r, both chains, heads, the means of adj_norm's columns and the operand-scale
//      bound of the current M
enum { FW_PREP, FW_R_DONE, FW_LAYER_PRODUCT, FW_LAYER_POST, FW_HEADS, FW_COUNT };
// d and r; the early pack (monolithic) or the gather of r | d (row-block rank)
static int fw_prep(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, ld = s.ld, R0 = s.R0, R1 = s.R1;
  if (h->carry.prep_valid) {
    prep_from_partials(st, n, h->G_A, adam_row_sums(h, (size_t)n * fl_tail_tiles(n)), h->d, h->r, h->rowsq, h->rowsum, R0, R1);
  } else {
    launch_prep(st, false, n, ld, h->M, nullptr, nullptr, 0.f, nullptr, nullptr, h->d, h->r, h->rowsq, h->rowsum, R0, R1);
  }
  if (!h->p.sharded) {
    // Early pack: the planes of the N x N x N product's operand need r only, and the pack is a pure streaming pass
    // (read M, write planes) while the forward's two skinny products keep the fp32 matrix pipe busy at 3 - 4 TB/s: the
    // pack runs on the product's stream beside them instead of behind them (0.16 ms off the path in front of the product).
    // The product is forked behind the pack on that stream (p1_behind_pack_on) when the forward's products run on
    // skinny_x3.hip, whose blocks fit beside a product block; beside a gemm_f32 forward it was measured a wash, and the
    // product then waits for the forward (ev_fork).
    h->carry.early_pack = false;
    if (late_mean(h) && h->p.overlap && h->st2 && h->p.early_pack_on) {
      CHK(pack_on_side_stream(h, st, 0, -1, h->cfg.w[1] != 0 ? h->A1 : nullptr,
                              pack_row_sums(h, split3_pack_rsq_parts(n, h->p.split_planes)), !h->p.p1_behind_pack_on));
      h->carry.early_pack = true;
      // With the product behind the pack, the pack is on the path: it streams M alone and the product follows it directly;
      // the forward (and the sums above) follow it on the caller's stream, beside the product.
      if (h->p.p1_behind_pack_on) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_pack, 0));
    }
    if (!h->carry.early_pack || h->p.p1_behind_pack_on) launch_reduce_rows(st, h->rowsq, n, 2, h->scal + S_SQ);      // rowsq | rowsum are adjacent, and so are S_SQ | S_SUM
  } else {
    // own rows of r and d, and this rank's share of |adj_changes|^2 and sum(modified_adj) in the scalar lane: ONE gather
    const Stage sg = narrow_stage(h);
    if (R1 > R0) {      // (the slots are written in full; only a rank without rows has to clear them)
      launch_reduce_rows(st, h->rowsq + R0, R1 - R0, 1, lane_slot(h, sg, 0));
      launch_reduce_rows(st, h->rowsum + R0, R1 - R0, 1, lane_slot(h, sg, 1));
    } else CHK(lane_zero(h, st, sg, 2));
    rows_to_stage2(h, st, sg, 1, h->r, 1, 0, 1, h->d, 1, 1);
  }
  return xchg_sg(s);
}
// r is complete (a row-block rank: gathered, and its product forked); the layers start
static int fw_r_done(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  if (h->p.sharded) {
    const Stage sg = narrow_stage(h);
    stage_to_rows2(h, st, sg, 1, 0, h->r, 1, 1, 1, h->d, 1);
    lane_sum(h, st, sg, 2, h->scal + S_SQ);          // S_SQ | S_SUM are adjacent
    // r is complete: the N x N x N product needs nothing else of this forward (uncentred planes: KFC 1 = 0)
    if (h->p.early_p1_on && s.R1 > s.R0 && !(h->fs_active && h->fs_what == MCGRA_SHARD_MONITOR && h->fs_last)) CHK(fork_p1_early(s));
  }
  h->step.fs_l = 0;
  return GO;
}
// layer fs_l: the product Y = M [r o Tv | Tu (| r)]; its post pass loops back until the last layer is done
static int fw_layer_product(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, hs = s.hs, fc = s.fc;
  const bool fused_post = h->p.fused_post;
  const int l = h->step.fs_l, w = h->p.wdt[l];
  const float* Xs[3] = {h->Tv + h->p.off[l], h->Tu + h->p.off[l], h->r};
  const float* rs[3] = {h->r, nullptr, nullptr};
  const int lds[3] = {hs, hs, 1}, ws[3] = {w, w, 1};
  const bool with_r = l == 0 && !late_mean(h) && !h->p.elementwise();   // (late mean: the means come out of the pack; MSELoss: no means)
  // [r o Tv | Tu (| r)] -- already in FV when the previous layer's post pass wrote it (fl_layer_post_next)
  if (!(l >= 1 && fused_post && fl_layer_post_fused_supported(h->p.wdt[l - 1], w)))
    fl_cat_segs(st, n, with_r ? 3 : 2, Xs, lds, rs, ws, h->FV, fc);
  CHK(mm_rows(h, st, 2 * w + (with_r ? 1 : 0), true));
  return xchg_fy(s);
}
static int fw_layer_post(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, hs = s.hs, L = s.L, C = s.C, fc = s.fc;
  const bool fused_post = h->p.fused_post;
  const int l = h->step.fs_l, w = h->p.wdt[l];
  const bool wr = l == 0 && !late_mean(h) && !h->p.elementwise();
  // the post pass and what follows it on the same rows in ONE launch where the widths allow (<= 32): the next
  // layer's T of both chains + the next product's right-hand side, or -- last layer -- both linear heads with their
  // log-softmax (same operations in the same order as the separate kernels)
  if (l + 1 < L && fused_post && fl_layer_post_fused_supported(w, h->p.wdt[l + 1])) {
    fl_layer_post_next(st, n, w, h->fy, h->FV, fc, h->r, h->b[l], h->Pv + h->p.off[l], h->Hv + h->p.off[l], h->Pu + h->p.off[l],
                       h->Hu + h->p.off[l], hs, wr, h->cmean, h->rowsx, h->p.wdt[l + 1], h->W[l + 1], h->Tv + h->p.off[l + 1],
                       h->Tu + h->p.off[l + 1]);
  } else if (l + 1 == L && fused_post && fl_layer_post_fused_supported(w, C)) {
    fl_layer_post_head(st, n, w, h->fy, h->FV, fc, h->r, h->b[l], h->Pv + h->p.off[l], h->Hv + h->p.off[l], h->Pu + h->p.off[l],
                       h->Hu + h->p.off[l], hs, wr, h->cmean, h->rowsx, C, h->Wlin, h->blin, h->Z, h->logp, h->sm, h->Z2, h->sm2,
                       h->cfg.head_act);
  } else {
    fl_layer_post(st, n, w, h->fy, h->FV, fc, h->r, h->b[l], h->Pv + h->p.off[l], h->Hv + h->p.off[l], h->Pu + h->p.off[l],
                  h->Hu + h->p.off[l], hs, wr, h->cmean, h->rowsx);
    if (l + 1 < L) {
      launch_rowmat(st, n, w, h->p.wdt[l + 1], h->Hv + h->p.off[l], hs, h->W[l + 1], h->p.wdt[l + 1], 1, nullptr, h->Tv + h->p.off[l + 1], hs);
      launch_rowmat(st, n, w, h->p.wdt[l + 1], h->Hu + h->p.off[l], hs, h->W[l + 1], h->p.wdt[l + 1], 1, nullptr, h->Tu + h->p.off[l + 1], hs);
    }
  }
  if (++h->step.fs_l < L) h->fw_state = FW_LAYER_PRODUCT;
  return GO;
}
// heads (where the last post pass did not take them), the operand-scale bound and the mean's statistics
static int fw_heads(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, L = s.L, C = s.C;
  if (!(h->p.fused_post && fl_layer_post_fused_supported(h->p.wdt[L - 1], C))) {
    CHK(head_forward(h, st, h->Hv, h->Z, h->logp, h->sm));
    CHK(head_forward(h, st, h->Hu, h->Z2, nullptr, h->sm2));
  }
  if (late_mean(h)) { if (h->amax && !h->carry.early_pack) hipLaunchKernelGGL(k_rmax2, dim3(1), dim3(1024), 0, st, n, h->r, h->amax + 1); }
  else if (!h->p.elementwise())      // (p1_early: the operand-scale bound is k_rmax2's, and the product in flight reads it)
    fl_mean_stats(st, n, h->cmean, h->r, h->fstat + 192, (h->amax && !h->carry.p1_early) ? h->amax + 1 : h->mm + 3);
  MCGRA_KERNEL_CHECK();
  return GO;
}
static const FusedStage FW_STAGES[FW_COUNT] = {fw_prep, fw_r_done, fw_layer_product, fw_layer_post, fw_heads};

// Returns 1 at an exchange point (s.ex filled), 0 when done, < 0 on error.
static int forward_stages(FusedStep& s) {
  const int rc = run_stages(s, FW_STAGES, FW_COUNT, s.h->fw_state);
  if (rc == GO) s.h->fw_state = 0;
  return rc;
}
static int fused_forward_pt(mcgra_attack* h, hipStream_t st, mcgra_exchange_t* ex) {      // the monitor call's forward
  FusedStep s = fused_ctx(h, st, ex);
  return forward_stages(s);
}

int fused_forward(mcgra_attack* h, hipStream_t st) {      // monolithic engines only
  h->fw_state = 0;
  h->step.planes_valid = false;      // (mm_rows reads it; a step sets it behind its own pack only)
  return fused_forward_pt(h, st, nullptr);
}

// host-side bookkeeping of a fused step that went through (the Adam pass is enqueued)
static void fused_commit(mcgra_attack* h) {
  h->step.planes_valid = false;          // the Adam pass is enqueued: Bpack no longer describes M
  h->step.lr_step = !h->p.elementwise();
  if (!h->p.elementwise()) ++h->lr_steps;      // (the fused MSELoss step has no low-rank form: it counts as a fused step only)
  ++h->fused_steps;
  h->t += 1;
  h->carry.prep_valid = adam_emits_partials(h, (size_t)h->p.n * fl_tail_tiles(h->p.n));
  h->have_step = true;
  h->carry.fused_last = true;
}

// A fused step that did not reach one of its regular exits (a HIP error, or a row-block step the caller abandoned after a
// failed collective and began again) leaves work on the side streams, a forked product / decode nobody joined and
// possibly a masked-pair post the host never looked at.  Everything such a step wrote is scratch (the Adam pass is its
// last kernel), so the next step only has to drain the streams and take the device's post counter.
static int fused_resync(mcgra_attack* h, hipStream_t st) {
  (void)hipStreamSynchronize(st);
  if (h->st2) (void)hipStreamSynchronize(h->st2);
  if (h->st3) (void)hipStreamSynchronize(h->st3);
  if (h->st4) (void)hipStreamSynchronize(h->st4);
  (void)hipGetLastError();
  unsigned int seq = 0;
  MCGRA_HIP(hipMemcpy(&seq, h->mask_seq_dev, sizeof(seq), hipMemcpyDeviceToHost));
  h->mask_seq = h->mask_want = seq;
  // (the streams were drained above, but st2 is non-blocking and shared with other engines: what was forked for the abandoned
  // step is ordered in front of this stream's next launches explicitly, as at every other site that drops it)
  CHK(carry_drop(h, st));
  carry_forget(h, true);      // (skip_fused stands: the abandoned step wrote scratch only, M and the model are the ones it was counted on)
  h->step = StepScratch{};
  h->fs_open = false;
  return 0;
}

// Row partials [n][nt] and value partials of the tail's first pass: the END of KY.  (Its start holds the split-K slabs of the
// product's ragged rounds, and the second part of a cut product writes them while the early pass over the finished rows runs.)
static size_t tail_ps_floats(const mcgra_attack* h) {
  const size_t nt = fl_tail_tiles(h->p.n);
  return ((((size_t)h->p.n * nt + 1) & ~(size_t)1) + 6 * nt * nt + 3) & ~(size_t)3;      // (value partials: up to three per block, fp64)
}
static float* tail_ps(const mcgra_attack* h) { return (h->KY ? h->KY : h->KX) + (size_t)h->p.n * h->p.ld - tail_ps_floats(h); }      // (MSELoss engines keep no KY; KX is idle there)

static double* tail_vpart(const mcgra_attack* h) {
  return reinterpret_cast<double*>(tail_ps(h) + (((size_t)h->p.n * fl_tail_tiles(h->p.n) + 1) & ~(size_t)1));
}

// k_tail_reduce of the step over rows [R0, R1) (phase 1: only its rank-k panels are packed -- their inputs are ready before
// the N x N x N product is joined; 2: the pass itself).  Returns the number of blocks (partials of the loss-term values).
static int tail_reduce_call(const FusedStep& s, int phase, int R0, int R1, bool want_vals) {
  mcgra_attack* h = s.h;
  const int hs = s.hs, he = s.he;
  const bool no_rk = h->test_mutate == 2;      // (TEST-ONLY mutation, see the join below)
  TailOperands t{};
  t.gs[0] = RankK{h->GPv, hs, h->Tv, hs, hs, no_rk ? 0.f : 1.f};
  t.u = RankK{h->GPu, hs, h->Tu, hs, no_rk ? 0 : hs, 1.f};
  t.M = h->M; t.r = h->r;
  t.a1 = s.a1; t.a2 = s.a2; t.k1 = s.kmse1; t.k2 = s.kmse2; t.kie6 = (float)(s.k6 / s.n2);      // (a1, a2 | k1, k2: zero for the other kinds)
  t.G2 = h->G_ADJN; t.ps = tail_ps(h); t.vpart = want_vals ? tail_vpart(h) : nullptr; t.rkbuf = h->rkbuf;
  switch (s.kind) {
    case FUSED_KL:      // calc = calc_kl
      t.P = h->XC; t.rowa = h->klA; t.rowb = h->kl1; t.rowc = h->klv;
      t.Zn = h->Zn; t.ldz = h->p.hmax; t.hz = he;
      break;
    case FUSED_MSE:     // calc = MSELoss
      t.P = h->FADJ; t.rowa = h->cmean;
      t.Zn = h->Zn; t.ldz = h->p.hmax; t.hz = he;
      break;
    default:            // linear_HSIC in its low-rank form
      if (s.use1) t.P = h->KX;
      t.rowa = h->cmean;
      if (s.use2) {
        t.gs[1] = RankK{h->lrL, 2 * he, h->lrR, 2 * he, 2 * he, no_rk ? 0.f : s.a2};
        t.rowb = h->lrDelta; t.rowc = h->lrC;
      }
  }
  return fl_tail_reduce(s.st, s.kind, s.n, h->p.ld, s.pair, R0, R1, t, phase);
}

// The N x N x N product P1 = KFC Xc^T[:, own rows] (c1) on the side stream -- forked here: the caller's stream is recorded, the side
// stream waits for it, ev_join marks the product's end (ev_first / ev_second the cuts).  Sets p1_inflight (and p1_first / tail_rows).
// behind_pack: the planes were packed on the side stream by this M's early pack, and nothing else on the caller's stream feeds
// the product (Apack: the graph's; Bpack, amax[1]: the pack's; KX, KY, small_slab: last read by the previous step's tail, which
// precedes the pack's ev_r) -- the product goes straight behind the pack, beside the forward and whatever follows it.
static int fork_p1(mcgra_attack* h, hipStream_t st, bool want_vals, bool behind_pack = false) {
  const int n = h->p.n, ld = h->p.ld, R0 = h->p.row0, R1 = h->p.row1;
  const int P = split3_panel(), p_off = R0 / P, p_cnt = R1 > R0 ? (R1 - R0 + P - 1) / P : 0;
  const bool ovl = h->p.overlap;
  const int sflag = h->p.split_single ? 8 : 0;      // MCGRA_SPLIT_BF16=1: the single-plane product of the same operands (split_symm_bf16.hip)
  h->step.p1_inflight = false;
  if (p_cnt <= 0) return 0;
  hipStream_t sp = ovl ? h->st2 : st;
  if (ovl && !behind_pack) {
    MCGRA_HIP(hipEventRecord(h->ev_fork, st));
    MCGRA_HIP(hipStreamWaitEvent(h->st2, h->ev_fork, 0));
  }
  CHK(timer_begin(h, sp, h->profile));
  h->carry.p1_first = false;
  if (h->p.sharded && h->p.a2a_overlap && ovl && h->p.world > 1 && h->test_mutate != 1) {
    // Row panels of the peers first (rotated start: the panel behind the own ones, wrapping), own panels last, the launch
    // cut behind the peers' tiles: the all-to-all that hands them over waits for ev_first only and runs beside the rest.
    // The cut sits on a whole round of the chip when that still leaves own tiles behind it (a cut costs a ragged round).
    const int tiles_all = (n + P - 1) / P, rot = (p_off + p_cnt) % tiles_all;
    const int span = min(tiles_all, (tiles_all - p_cnt + 3) & ~3) * p_cnt, total = tiles_all * p_cnt;
    const int slots = split3_slots();
    int first = (span + slots - 1) / slots * slots;
    // (no whole round left behind the peers' tiles: a cut there costs a second ragged round -- taken while the own
    // panels are at least a quarter of the product, world <= 4, or when forced)
    if (first >= total) first = (h->p.world <= 4 || h->p.a2a_overlap == 2) ? span : 0;
    if (first > 0 && first < total) {
      MCGRA_HIP(split3_symm(sp, n, h->Apack, h->Bpack, h->KX, ld, rot, -1, h->KY, sizeof(float) * (size_t)n * ld, h->p.split_planes,
                            h->amax, p_off, p_cnt, 4 | sflag, first, h->ev_first));
      h->carry.p1_first = true;
      ++h->cut_product_steps;
    }
  }
  h->step.tail_rows = h->step.tail_rows2 = 0;
  if (!h->carry.p1_first && !h->p.sharded && ovl && h->p.early_tail_on && n >= 8192 && !want_vals && h->test_mutate != 1) {
    // The tail's first pass needs P1_ij and P1_ji: the rows the product has finished in BOTH orientations.  Its tiles run
    // in groups of four row panels, so behind a cut on whole rounds of the chip at ~0.8 of the launch the first
    // `tail_rows` rows are complete, and the pass over them runs beside the product's last rounds (N = 10 000: the cut
    // at 1 280 of 1 600 tiles = five rounds = eight groups = 8 192 rows, two thirds of the pass).
    const int tiles_all = (n + P - 1) / P, total = tiles_all * tiles_all, group = 4 * tiles_all;
    const int slots = split3_slots();
    const int cut = (int)(0.8 * total) / slots * slots;
    const int rows = min(n, cut / group * 4 * P);
    // ... and a second cut behind the last whole round: the rows that one completes, beside the ragged rest
    int cut2 = total / slots * slots, rows2 = min(n, cut2 / group * 4 * P);
    if (cut2 <= cut || cut2 >= total || rows2 <= rows) { cut2 = 0; rows2 = 0; }
    if (cut >= slots && cut < total && rows >= n / 2) {
      MCGRA_HIP(split3_symm(sp, n, h->Apack, h->Bpack, h->KX, ld, 0, -1, h->KY, sizeof(float) * ((size_t)n * ld - tail_ps_floats(h)),
                            h->p.split_planes, h->amax, p_off, p_cnt, sflag, cut, h->ev_first, cut2, cut2 ? h->ev_second : nullptr));
      h->step.tail_rows = rows;
      h->step.tail_rows2 = rows2;
      ++h->cut_product_steps;
    }
  }
  if (!h->carry.p1_first && h->step.tail_rows == 0)
  MCGRA_HIP(split3_symm(sp, n, h->Apack, h->Bpack, h->KX, ld, 0, -1, h->small_slab ? h->small_slab : h->KY,
                        h->small_slab ? h->small_slab_bytes : sizeof(float) * (size_t)n * ld, h->p.split_planes, h->amax, p_off, p_cnt, sflag));
  CHK(timer_end(h, sp, h->profile, 2.0 * (double)n * n * (double)(R1 - R0)));
  ++h->split_steps;
  if (ovl) MCGRA_HIP(hipEventRecord(h->ev_join, h->st2));
  h->step.p1_inflight = true;
  return 0;
}

// Row-block rank: pack and product forked by the FORWARD (a monitor call's, adopted by the next step, or the step's own) as
// soon as r is complete.  On a rank the forward is a chain of ~25 short launches and three gathers -- 0.16 ms at N = 10 000,
// world 8, a quarter of the rank's product -- and nothing in it feeds the product: the planes are packed UNCENTRED (the product
// does not see the centring vector: KFC 1 = 0; the monolithic step packs the same way), their scale bound is max r^2, and the
// rows' |xc_i|^2 come from the pack's partials once the forward has the means (k_rsq_fin_unc).  The step finds p1_early set.
// A forward whose step never comes (the last monitor call of a run) leaves a product nobody reads: carry_drop.
static int fork_p1_early(const FusedStep& s) {      // (called with R1 > R0: p_cnt > 0)
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  CHK(carry_drop(h, st));      // (two forwards in a row)
  if (!s.use1 || !h->p.overlap || !h->st2 || h->test_mutate == 1) return 0;
  CHK(pack_on_side_stream(h, st, s.p_off, s.p_cnt, s.use2 ? h->A1 : nullptr,
                          s.use2 ? pack_row_sums(h, split3_pack_rsq_parts(s.n, h->p.split_planes)) : nullptr, false));
  const auto cut0 = h->cut_product_steps, split0 = h->split_steps;
  CHK(fork_p1(h, st, true));
  h->carry.p1_early = h->step.p1_inflight;
  // (the counters move with the step that takes the product, not with a forward whose step may never come)
  h->carry.p1_early_cut = (int)(h->cut_product_steps - cut0); h->cut_product_steps = cut0;
  h->carry.p1_early_split = (int)(h->split_steps - split0); h->split_steps = split0;
  return 0;
}

// ---- the step's stages (FS_STAGES, in program order; h->fs_state is the index of the next one)
enum {
  FS_BEGIN, FS_FORWARD, FS_PACK_FORK, FS_HEAD_BWD, FS_DECODE_STATS, FS_DECODE, FS_LR_PREP, FS_SMALL_TERMS, FS_LR_T, FS_LR_Q, FS_DECODE_BWD,
  FS_BWD_PRODUCT, FS_BWD_POST, FS_TAIL_FRONT, FS_TAIL_REDUCE, FS_DECIDE, FS_GATHER_SEND, FS_GATHER_RECV, FS_ADAM, FS_SCALARS, FS_COUNT
};
static int join_p1(const FusedStep& s) {      // the forked product, in front of its first reader on the caller's stream
  if (s.h->step.p1_inflight) {
    if (s.ovl) MCGRA_HIP(hipStreamWaitEvent(s.st, s.h->ev_join, 0));
    s.h->step.p1_inflight = false;
  }
  return 0;
}

// what an abandoned step left is dropped; a forward the monitor call left for this M is adopted
static int fs_begin(FusedStep& s) {
  mcgra_attack* h = s.h;
  if (h->fs_open) CHK(fused_resync(h, s.st));
  h->fs_open = true;
  h->step.planes_valid = false;
  h->step.fs_adopted = h->carry.fused_fwd_valid;
  h->carry.fused_fwd_valid = false;
  h->carry.fwd_cached = false;
  h->fw_state = 0;
  return GO;
}
// the step's own forward: this stage is the next one until FW_STAGES has run through
static int fs_forward(FusedStep& s) {
  if (s.h->step.fs_adopted) return GO;
  const int rc = forward_stages(s);
  if (rc == AT_XCHG) s.h->fs_state = FS_FORWARD;
  return rc;
}
// the operand pack (where no forward did it), the product P1 forked, the late means, the third stream forked
static int fs_pack_fork(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, ld = s.ld, hs = s.hs, Le = s.Le, R0 = s.R0, R1 = s.R1, he = s.he, p_off = s.p_off, p_cnt = s.p_cnt;
  const bool mse = s.elementwise(), use1 = s.use1, use2 = s.use2, want_vals = s.want_vals;
  const int np = split3_pack_rsq_parts(n, h->p.split_planes);      // (the pack's per-block row partials: sums of squares in A1, pack_row_sums)
  bool behind_pack = false;      // (the product forked behind the early pack: fork_p1)
  // planes of Xc^T rows straight from M, |xc_i|^2 from the same pass
  if (late_mean(h)) {
    // uncentred planes ((H Kf H) 1 = 0: the product does not see the centring vector), row sums and sums of squares of
    // adj_norm from the same pass -> the column means (adj_norm is symmetric) and |xc_i|^2
    if (h->carry.early_pack) {
      // packed on the product's stream beside this M's forward (fused_forward_pt): everything on the caller's stream that
      // reads the planes or the pack's row partials (k_mean_fin, planes_mm) waits for it here
      MCGRA_HIP(hipStreamWaitEvent(st, h->ev_pack, 0));
      h->carry.early_pack = false;
      behind_pack = h->p.p1_behind_pack_on;
    } else
      split3_pack_from_m(st, n, ld, h->M, h->r, nullptr, h->Bpack, h->p.split_planes, h->amax ? h->amax + 1 : nullptr, 0, -1,
                         use2 ? h->A1 : nullptr, pack_row_sums(h, np));
    h->step.planes_valid = planes_mm_on(h);          // (the means themselves: behind the fork, below)
  } else
  if (p_cnt > 0 && !mse && !h->carry.p1_early) {
    split3_pack_from_m(st, n, ld, h->M, h->r, h->cmean, h->Bpack, h->p.split_planes, h->amax ? h->amax + 1 : nullptr, p_off, p_cnt,
                       use2 ? h->A1 : nullptr);
    if (use2)
      hipLaunchKernelGGL(k_rsq_fin, dim3((R1 - R0 + 3) / 4), dim3(256), 0, st, R0, R1, np, h->A1, h->lrRs);
  }

  // ---- P1 (column block of the own rows: Xc^T rows = adj_norm rows by symmetry) forked onto the side stream
  if (h->carry.p1_early) {
    // a row-block rank's forward forked pack and product as soon as r was complete (fork_p1_early): in flight since then.
    // The pack's row partials (|xc_i|^2 below) are ready at ev_pack.
    MCGRA_HIP(hipStreamWaitEvent(st, h->ev_pack, 0));
    h->carry.p1_early = false;
    h->cut_product_steps += h->carry.p1_early_cut; h->split_steps += h->carry.p1_early_split;
    if (use2)
      hipLaunchKernelGGL(k_rsq_fin_unc, dim3((R1 - R0 + 3) / 4), dim3(256), 0, st, R0, R1, n, np, h->A1, pack_row_sums(h, np), h->cmean, h->lrRs);
  } else {
    h->step.p1_inflight = false;
    if (p_cnt > 0 && use1) CHK(fork_p1(h, st, want_vals, behind_pack));
  }

  // (behind the fork: nothing in front of the product needs them)
  if (late_mean(h)) {
    hipLaunchKernelGGL(k_mean_fin, dim3((n + 3) / 4), dim3(256), 0, st, n, np, pack_row_sums(h, np), use2 ? h->A1 : nullptr, h->cmean, h->rowsx,
                       use2 ? h->lrRs : nullptr);
    fl_mean_stats(st, n, h->cmean, h->r, h->fstat + 192, h->mm + 3);      // sum(mean); (the operand-scale bound stays max r^2)
  }
  if (want_vals) MCGRA_HIP(hipMemsetAsync(h->scal + 2, 0, sizeof(double) * (S_COUNT - 2), st));
  // embedding(features, adj_norm) of this iteration (= the victim chain's activations: shared weights, main.py:190),
  // kept for the post-loop decode (:300): adj_norm itself is never stored
  MCGRA_HIP(hipMemcpy2DAsync(h->em_last, (size_t)h->p.hmax * 4, h->Hv + h->p.off[Le - 1], (size_t)hs * 4, (size_t)he * 4, n,
                             hipMemcpyDeviceToDevice, st));

  // (the small-operand terms c9 / c10 pick up here on a third stream; their ~16 tiny launches are ENQUEUED further down: the
  // host needs ~0.1 ms for them, during which the caller's stream -- the critical path of a short step: a row-block rank at
  // world 8, a small graph -- would sit idle with the head backward, the decode and the factor chain still to come)
  if (s.s3 != st) {
    MCGRA_HIP(hipEventRecord(h->ev_fork3, st));
    MCGRA_HIP(hipStreamWaitEvent(s.s3, h->ev_fork3, 0));
  }
  return GO;
}
// CE loss (:172) and its gradient into the victim chain
static int fs_head_bwd(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const mcgra_attack_config_t& c = h->cfg;
  const int n = s.n, ld = s.ld, hs = s.hs, L = s.L, C = s.C, he = s.he;
  const bool want_vals = s.want_vals;
  if (h->p.fused_post && fl_head_bwd_supported(C, h->p.wdt[L - 1], he)) {      // k_nll_grad + k_rowmat_mask in one launch
    fl_head_bwd_nll(st, n, C, h->p.wdt[L - 1], h->Wlin, h->Pv + h->p.off[L - 1], h->GPv + h->p.off[L - 1], hs, h->logp, h->sm, h->labels,
                    h->cnt, (float)(c.weight_sup / h->p.na), h->GZ, h->rowvals + 6 * (size_t)ld);
    if (want_vals) launch_reduce_rows(st, h->rowvals + 6 * (size_t)ld, n, 1, h->scal + S_NLL);
  } else {
    launch_nll_grad(st, n, C, h->logp, h->sm, C, h->labels, h->cnt, (float)(c.weight_sup / h->p.na), h->GZ, h->rowvals + 6 * (size_t)ld);
    if (want_vals) launch_reduce_rows(st, h->rowvals + 6 * (size_t)ld, n, 1, h->scal + S_NLL);
    launch_rowmat_mask(st, n, C, h->p.wdt[L - 1], h->GZ, C, h->Wlin, h->p.wdt[L - 1], 1, nullptr, 0, 0, nullptr, 0, 0,
                       h->Pv + h->p.off[L - 1], hs, h->cfg.act, nullptr, 0, h->GPv + h->p.off[L - 1], hs);
  }
  return GO;
}
// dot_product_decode + get_modified_adj_after (:187-188), recomputed per pair from Zn, own rows: the row normalisation and
// -- KL -- the row statistics, which a row-block rank gathers
static int fs_decode_stats(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, ld = s.ld, hs = s.hs, C = s.C, R0 = s.R0, R1 = s.R1, he = s.he;
  const bool zero_inline = s.zero_inline;
  // (small-operand terms on the caller's stream -- the fused MSELoss step of a small graph: the zero fills of what they and the
  //  decode accumulate into ride in this launch instead of three launches of their own)
  {
    const ZeroFill zf{h->Gem, (size_t)n * h->p.hmax, s.use10 ? h->Gsm : nullptr, s.use10 ? (size_t)n * C : 0, h->nmask, 2};
    launch_row_normalize(st, n, he, s.em, hs, h->Zn, h->p.hmax, h->nrm, 2.f, h->Zpair, zero_inline ? &zf : nullptr);
    if (zero_inline) h->step.nmask_zero = true;
  }
  if (s.kl()) {
    // calc_kl's row statistics (logsumexp of adj_norm's and of modified_adj1's rows) from M, r and Zn: the decode backward and
    // the tail need those of EVERY row (d c2 / d A1_ij + d c2 / d A1_ji), so a row-block rank gathers its peers' first
    (void)fl_decode_stats(st, n, R0, R1, he, h->Zn, h->p.hmax, h->Zpair, h->M, ld, h->r, h->klpart, h->klA, h->kl1);
    if (h->test_mutate == 4) {      // TEST-ONLY mutation: the row statistics wiped before the decode and the tail read them
      MCGRA_HIP(hipMemsetAsync(h->klA, 0, sizeof(float) * (size_t)n, st));
      MCGRA_HIP(hipMemsetAsync(h->kl1, 0, sizeof(float) * (size_t)n, st));
    }
    if (h->p.sharded) rows_to_stage2(h, st, narrow_stage(h), 1, h->klA, 1, 0, 1, h->kl1, 1, 1);
  }
  return s.kl() ? xchg_sg(s) : GO;
}
// What both decodes share: the fork onto s4 (forked: s4 is the fourth stream), the masked-pair counter cleared, k_decode_fly
// over the own rows with its row partials in rowvals (fs_np of them) ...
static int decode_fly(const FusedStep& s, hipStream_t s4, bool forked, bool zero, float* slabs, double* rowvals, bool want_vals) {
  mcgra_attack* h = s.h;
  if (forked) {
    MCGRA_HIP(hipEventRecord(h->ev_fork4, s.st));
    MCGRA_HIP(hipStreamWaitEvent(s4, h->ev_fork4, 0));
  }
  if (zero) MCGRA_HIP(hipMemsetAsync(h->nmask, 0, 2 * sizeof(unsigned int), s4));
  h->step.nmask_zero = false;
  DecodeOperands d{};
  d.Z = h->Zn; d.ldz = h->p.hmax; d.zpair = h->Zpair; d.kie7 = (float)(s.k7 / s.n2);
  d.slabs = slabs; d.v7part = rowvals; d.GZn = h->GZn; d.ldg = h->p.hmax; d.nmask = h->nmask;
  if (s.elementwise()) { d.M = h->M; d.ldm = s.ld; d.r = h->r; d.k2 = s.kmse2; }
  if (s.kl()) { d.lseA = h->klA; d.lse1 = h->kl1; d.vrow = h->klpart; }
  h->step.fs_np = fl_decode_fly(s4, s.kind, s.n, s.R0, s.R1, s.he, d, want_vals);
  return 0;
}
// ... and its end on s4, behind whatever the variant put there: fs_dec_forked asks the first reader of its results to join
static int decode_end(const FusedStep& s, hipStream_t s4, bool forked) {
  if (forked) MCGRA_HIP(hipEventRecord(s.h->ev_join4, s4));
  s.h->step.fs_dec_forked = forked;
  return 0;
}
// monolithic: the results go to scal, the masked-pair count is posted from the decode's stream
static int decode_monolithic(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, R0 = s.R0, R1 = s.R1;
  const bool mse = s.elementwise(), kl = s.kl(), use2 = s.use2, want_vals = s.want_vals;
  // monolithic, small graphs (where the step is bound by its chain of dependent node-level kernels): the decode -- the
  // longest of them, and it needs only Zn -- on a fourth stream with its own slabs, beside the low-rank factor chain;
  // joined in front of the first consumer of G_Zn (n = 2708: 0.60 -> 0.54 ms per step).  At N = 10 000 the chain hides
  // behind the product anyway and a decode that runs beside more of it only slows the product (6.4 -> 6.9 ms).
  // The masked-pair count is posted from the decode's stream (see below).
  // (an elementwise measure -- MSELoss, KL -- has no factor chain: the caller's stream would only wait for the decode, and the
  //  fork and the join cost it two event round trips (~17 us each): the decode stays on the caller's stream there -- Cora-shaped
  //  MSELoss 0.248 -> 0.214 ms, KL 0.307 -> 0.271; A/B MCGRA_MSE_DECODE_SIDE=1)
  hipStream_t s4 = (h->st3 != st && n < 4096 && (!mse || h->p.mse_decode_side)) ? h->st4 : st;
  // (with c2, k_post_mask leaves the counter at zero for the next fused step; the general path does not)
  CHK(decode_fly(s, s4, s4 != st, !h->step.nmask_zero, h->ws_dec, h->rowvals, want_vals));
  if (want_vals) launch_reduce_rows(s4, h->rowvals, h->step.fs_np, 1, h->scal + S_V7);
  if (kl) {      // v_i for the tail; their sum / n is the value of c2 (k_kl_rows' slot)
    fl_kl_v_fin(s4, n, R0, R1, h->klpart, h->klvsum, h->klv);
    if (want_vals) launch_reduce_rows(s4, h->klvsum, n, 1, h->scal + S_H2);
  }
  if (use2) {
    hipLaunchKernelGGL(k_post_mask, dim3(1), dim3(1), 0, s4, h->nmask, nullptr, h->mask_seq_dev, h->mask_host_dev);
    h->mask_want = ++h->mask_seq;      // the host's count moves with the enqueue: an abandoned step cannot skew it
    h->step.nmask_zero = true;
  }
  return decode_end(s, s4, s4 != st);
}
// row-block rank: the results go to the exchange stage of the next gather
static int decode_rank(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, ld = s.ld, R0 = s.R0, R1 = s.R1, he = s.he;
  const bool kl = s.kl(), use2 = s.use2;
  // row-block rank: the decode of the own rows -- the longest node-level kernel of a rank's step, and at world 8 that
  // chain, not the product, is the rank's critical path -- on the fourth stream with its own slabs, beside the column
  // statistics, the factor prep and the first low-rank product; joined in front of the gather its results ride in
  const bool dec_side = use2 && s.s3 != st && h->ws_dec != nullptr;
  hipStream_t s4 = dec_side ? h->st4 : st;
  CHK(decode_fly(s, s4, dec_side, true, dec_side ? h->ws_dec : h->ws, h->rowvals + 6 * (size_t)ld, true));
  // own rows of the decode backward and of |xc_i|^2, the rank's masked-pair and dead-row counts and its entropy partial:
  // they ride in the gather of the first low-rank product below (or, without c2, in a gather of their own)
  const Stage sg = use2 ? wide_stage(h) : narrow_stage(h);
  hipLaunchKernelGGL(k_u32x2_to_f64, dim3(1), dim3(1), 0, s4, h->nmask, lane_slot(h, sg, 0), lane_slot(h, sg, 1));
  if (h->step.fs_np > 0) launch_reduce_rows(s4, h->rowvals + 6 * (size_t)ld, h->step.fs_np, 1, lane_slot(h, sg, 2));
  else MCGRA_HIP(hipMemsetAsync(lane_slot(h, sg, 2), 0, sizeof(double), s4));
  if (use2) rows_to_stage2(h, s4, sg, he, h->GZn, h->p.hmax, 0, 2, reinterpret_cast<const float*>(h->lrRs), 2, he);     // |xc_i|^2 (double) as two words
  else if (kl) {      // + the own rows' v_i, and the rank's share of c2's value in a fourth lane slot
    fl_kl_v_fin(s4, n, R0, R1, h->klpart, h->klvsum, h->klv);
    if (R1 > R0) launch_reduce_rows(s4, h->klvsum + R0, R1 - R0, 1, lane_slot(h, sg, 3));
    else MCGRA_HIP(hipMemsetAsync(lane_slot(h, sg, 3), 0, sizeof(double), s4));
    rows_to_stage2(h, s4, sg, he, h->GZn, h->p.hmax, 0, 1, h->klv, 1, he);
  }
  else rows_to_stage(h, s4, sg, he, h->GZn, h->p.hmax, 0);
  return decode_end(s, s4, dec_side);
}
static int fs_decode(FusedStep& s) {
  mcgra_attack* h = s.h;
  if (s.kl() && h->p.sharded) stage_to_rows2(h, s.st, narrow_stage(h), 1, 0, h->klA, 1, 1, 1, h->kl1, 1);
  CHK(h->p.sharded ? decode_rank(s) : decode_monolithic(s));
  MCGRA_KERNEL_CHECK();
  return s.use2 ? GO : xchg_sg(s);
}
// Low-rank factors (section 1b) with the products on M (section 1c).  T = Xc^T Vc without the delta^2 column
// of V: on a low-rank step every row of Zn has unit norm (a dead row would have masked its pairs), so that
// column is constant, its centred copy is rounding noise and t3 = Xc^T (delta^2 - mean) is taken as 0 --
// which keeps the product at 32 columns (one column tile of the skinny kernel)
static int fs_lr_prep(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, fc = s.fc, he = s.he;
  if (!s.use2) return GO;
  // (the dense form where this chain is the critical path -- a row-block rank, a graph whose product is short -- and the
  // slow one beside the long product of a large monolithic graph, which the dense one holds up: lowrank_kernels.hip)
  launch_lr_colstats(st, n, he, h->Zn, h->p.hmax, h->lrStats, (h->p.sharded && h->p.world > 1) || n < 8192);
  // (the right-hand side r o V of the product below comes out of the same launch: fl_cat_scaled's values)
  launch_lr_prep(st, n, he, h->Zn, h->p.hmax, h->lrStats, h->lrL, h->lrV, h->p.lr_ldv, h->lrDelta, h->p.fused_post ? h->r : nullptr,
                 h->p.fused_post ? h->FV : nullptr, fc);
  fl_wcolsum(st, n, 2 * he, h->lrV, h->p.lr_ldv, nullptr, h->fstat, nullptr, h->fstat + 256);
  if (!h->p.fused_post) fl_cat_scaled(st, n, 2 * he, 2 * he, h->lrV, h->p.lr_ldv, h->r, h->FV, fc, 0);
  CHK(mm_rows(h, st, 2 * he));
  return GO;
}
// Small-operand terms c9 (:237-258) and c10 (:259-272): they need only the forward, and at small n their ~16
// tiny launches are a tenth of the step -- on a third stream (forked behind the forward: fs_pack_fork), joined in front of the
// backward of em.  ENQUEUED here, behind the decode and the first low-rank product: while the host spends its ~0.1 ms on
// them the caller's stream has the column statistics, the factor prep and that product to run.
// With c2 the stage ends at the gather of that product.
static int fs_small_terms(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st, s3 = s.s3;
  const int n = s.n, hs = s.hs, C = s.C, he = s.he;
  const bool zero_inline = s.zero_inline, want_vals = s.want_vals;
  if (!zero_inline) MCGRA_HIP(hipMemsetAsync(h->Gem, 0, sizeof(float) * (size_t)n * h->p.hmax, s3));
  if (s.use9) CHK(small_term(h, s3, he, s.em, hs, h->HAg, h->HAc, s.sg * s.k9, h->Gem, h->p.hmax, S_C9, want_vals));
  if (s.use10) {
    if (!zero_inline) MCGRA_HIP(hipMemsetAsync(h->Gsm, 0, sizeof(float) * (size_t)n * C, s3));
    CHK(small_term(h, s3, C, h->sm2, C, h->YAg, h->YAc, s.sg * s.k10, h->Gsm, C, S_C10, want_vals));
    launch_softmax_bwd(s3, n, C, h->sm2, h->Gsm, C, h->GZ2);
  }
  if (s3 != st) MCGRA_HIP(hipEventRecord(h->ev_join3, s3));

  if (h->p.sharded && h->step.fs_dec_forked) {      // the decode's rows and lane slots ride in the gather below
    MCGRA_HIP(hipStreamWaitEvent(st, h->ev_join4, 0));
    h->step.fs_dec_forked = false;
  }
  return s.use2 ? xchg_fy(s) : GO;
}
// a row-block rank takes the decode's gathered results and posts its masked-pair count; [W | W2] = Xc^T Vc, and the product for Q
static int fs_lr_t(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, ld = s.ld, fc = s.fc, he = s.he;
  const bool kl = s.kl(), use2 = s.use2;
  if (h->p.sharded) {
    const Stage sg = use2 ? wide_stage(h) : narrow_stage(h);
    if (use2) stage_to_rows2(h, st, sg, he, 0, h->GZn, h->p.hmax, 2, he, reinterpret_cast<float*>(h->lrRs), 2);
    else if (kl) stage_to_rows2(h, st, sg, he, 0, h->GZn, h->p.hmax, 1, he, h->klv, 1);
    else stage_to_rows(h, st, sg, he, 0, h->GZn, h->p.hmax);
    lane_sum(h, st, sg, kl ? 4 : 3, h->SC + 8);              // SC[8] masked pairs, SC[9] dead rows, SC[10] entropy term of modified_adj1 (KL: SC[11] the value of c2)
    MCGRA_HIP(hipMemcpyAsync(h->scal + S_V7, h->SC + 10, sizeof(double), hipMemcpyDeviceToDevice, st));
    // A dead embedding row voids the low-rank algebra (k_post_mask).  The counts are posted to mapped host memory now and
    // looked at only in front of the Adam pass, the first kernel that changes persistent state: by then the post has
    // long landed, so the host never waits with an empty queue behind it (a readback + sync here cost 0.14 of the
    // 0.87 ms Cora-size step).  Everything in between writes scratch only; on such a step it is thrown away.
    if (use2) {
      hipLaunchKernelGGL(k_post_mask, dim3(1), dim3(1), 0, st, nullptr, h->SC + 8, h->mask_seq_dev, h->mask_host_dev);
      h->mask_want = ++h->mask_seq;
    }
  }
  if (use2) {
    if (!h->step.t3_zero) {                                                                        // t3 = 0
      MCGRA_HIP(hipMemset2DAsync(h->lrT + 2 * he, (size_t)h->p.lr_ldv * 4, 0, 4, n, st));
      h->step.t3_zero = true;
    }
    if (h->p.fused_post && he <= 32) {      // [W | W2] = Xc^T Vc and the per-column terms behind it in one launch
      launch_lrt_lr_post(st, n, he, h->fy, h->FV, fc, h->r, h->cmean, h->fstat, h->lrT, h->p.lr_ldv, h->lrStats, h->lrR, h->lrC,
                         h->rowvals + 7 * (size_t)ld);
    } else {
      fl_lrt_post(st, n, 2 * he, h->fy, h->FV, fc, h->r, h->cmean, h->fstat, h->lrT, h->p.lr_ldv);  // [W | W2] = Xc^T Vc
      launch_lr_post(st, n, he, h->lrT, h->p.lr_ldv, h->lrStats, h->lrR, h->lrC, h->rowvals + 7 * (size_t)ld);
    }
    // [Q | Q2] = Xc [W | W2]
    fl_wcolsum(st, n, 2 * he, h->lrT, h->p.lr_ldv, h->cmean, h->fstat + 64, h->fstat + 128, h->fstat + 256);
    fl_lrq_pre(st, n, 2 * he, h->lrT, h->p.lr_ldv, h->r, h->fstat + 64, h->FV, fc);
    CHK(mm_rows(h, st, 2 * he));
  }
  return use2 ? xchg_fy(s) : GO;
}
// [Q | Q2] = Xc [W | W2]
static int fs_lr_q(FusedStep& s) {
  mcgra_attack* h = s.h;
  const int he = s.he;
  if (s.use2)
    fl_lrq_post(s.st, s.n, 2 * he, h->fy, h->FV, s.fc, h->r, h->cmean, h->fstat + 64, h->fstat + 128, h->fstat + 192, h->lrQ, 2 * he);
  MCGRA_KERNEL_CHECK();
  return GO;
}
// decode backward (the entropy part is already in GZn), normalisation of em, and the head of the modified_adj chain
// (embedding + output2); the levels of both chains' backward are counted from here
static int fs_decode_bwd(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, ld = s.ld, hs = s.hs, L = s.L, Le = s.Le, C = s.C, he = s.he;
  const bool use2 = s.use2, want_vals = s.want_vals, use10 = s.use10;
  const double sg = s.sg, k2 = s.k2;
  if (h->step.fs_dec_forked) { MCGRA_HIP(hipStreamWaitEvent(st, h->ev_join4, 0)); h->step.fs_dec_forked = false; }
  if (use2) {
    launch_lr_xtz(st, n, he, h->lrQ, h->Zn, h->p.hmax, h->lrQtZ);
    launch_lr_part2(st, n, he, h->lrQ, h->Zn, h->p.hmax, h->lrDelta, h->lrRs, -2.f * (float)(sg * k2), h->GZn, h->p.hmax,
                    h->rowvals + 7 * (size_t)ld, h->rowvals + 5 * (size_t)ld, h->lrStats + 2 * he, h->lrQtZ, 2.f * (float)(sg * k2));
    if (want_vals) launch_reduce_rows(st, h->rowvals + 5 * (size_t)ld, n, 1, h->scal + S_H2);
  }
  if (s.s3 != st) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_join3, 0));       // c9 / c10: Gem, GZ2 and their scalars
  // ---- backward: modified_adj chain (embedding + output2), products on M
  if (use10 && h->p.fused_post && fl_head_bwd_supported(C, h->p.wdt[L - 1], he)) {
    // k_row_normalize_bwd (G_em += ...) + the head's mask pass in one launch
    fl_head_bwd_em(st, n, C, h->p.wdt[L - 1], h->Wlin, h->Pu + h->p.off[L - 1], h->GPu + h->p.off[L - 1], hs, h->GZ2, he, h->GZn, h->Zn,
                   h->p.hmax, h->nrm, h->Gem, h->p.hmax, L - 1 == Le - 1);
  } else {
    launch_row_normalize_bwd(st, n, he, h->GZn, h->Zn, h->p.hmax, h->nrm, h->Gem, h->p.hmax);
    if (use10) {
      launch_rowmat_mask(st, n, C, h->p.wdt[L - 1], h->GZ2, C, h->Wlin, h->p.wdt[L - 1], 1, nullptr, 0, 0, nullptr, 0, 0,
                         h->Pu + h->p.off[L - 1], hs, h->cfg.act, (L - 1 == Le - 1) ? h->Gem : nullptr, h->p.hmax, h->GPu + h->p.off[L - 1], hs);
    } else {
      if (L > Le) MCGRA_HIP(hipMemsetAsync(h->GPu, 0, sizeof(float) * (size_t)n * hs, st));
      launch_rowmat_mask(st, n, 0, he, h->Gem, h->p.hmax, h->Wlin, 0, 0, nullptr, 0, 0, nullptr, 0, 0, h->Pu + h->p.off[Le - 1], hs,
                         h->cfg.act, h->Gem, h->p.hmax, h->GPu + h->p.off[Le - 1], hs);
    }
  }
  // Backward of both chains, one product on M per level: columns [r o G_P_lv of the victim(adj_norm) chain | G_P_lu of
  // the modified_adj chain] (M symmetric: M^T G = M G; adj_norm^T G = r o (M (r o G) + r o G)), then
  // G_P_{l-1} = (G_T_l W_l^T) o relu'(P_{l-1}) for each chain.  fs_l / fs_l2: the levels still to do.
  h->step.fs_l = L - 1;
  h->step.fs_l2 = (use10 ? L - 1 : Le - 1);
  return GO;
}
// one level of that backward: the product, while fs_l / fs_l2 have levels left ...
static int fs_bwd_product(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, hs = s.hs, fc = s.fc;
  if (!(h->step.fs_l >= 1 || h->step.fs_l2 >= 1)) { h->fs_state = FS_TAIL_FRONT; return GO; }
  const int lv = h->step.fs_l, lu = h->step.fs_l2;
  const int wv = lv >= 1 ? h->p.wdt[lv] : 0, wu = lu >= 1 ? h->p.wdt[lu] : 0;
  const float* Xs[2] = {h->GPv + h->p.off[lv >= 1 ? lv : 0], h->GPu + h->p.off[lu >= 1 ? lu : 0]};
  const float* rs[2] = {h->r, nullptr};
  const int lds[2] = {hs, hs}, ws[2] = {wv, wu};
  if (lv >= 1) fl_cat_segs(st, n, lu >= 1 ? 2 : 1, Xs, lds, rs, ws, h->FV, fc);      // [r o G_P_lv | G_P_lu]
  else fl_cat_scaled(st, n, wu, wu, h->GPu + h->p.off[lu], hs, nullptr, h->FV, fc, 0);
  CHK(mm_rows(h, st, wv + wu));
  return xchg_fy(s);
}
// ... and what follows it on each chain; back to the product
static int fs_bwd_post(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, hs = s.hs, Le = s.Le, fc = s.fc;
  const int lv = h->step.fs_l, lu = h->step.fs_l2;
  const int wv = lv >= 1 ? h->p.wdt[lv] : 0;
  if (lv >= 1 && lu >= 1 && h->p.fused_post && fl_bwd_level_supported(wv, h->p.wdt[lu], h->p.wdt[lv - 1], h->p.wdt[lu - 1])) {
    // both chains' level in one launch (k_an_post + k_copy_cols + two k_rowmat_mask: same operations, same order)
    fl_bwd_level(st, n, wv, h->p.wdt[lu], h->fy, h->FV, fc, h->r, h->p.wdt[lv - 1], h->W[lv], h->Pv + h->p.off[lv - 1],
                 h->GPv + h->p.off[lv - 1], h->p.wdt[lu - 1], h->W[lu], h->Pu + h->p.off[lu - 1], h->GPu + h->p.off[lu - 1], hs,
                 (lu - 1 == Le - 1) ? h->Gem : nullptr, h->p.hmax);
  } else {
    if (lv >= 1) {
      fl_an_post(st, n, wv, h->fy, h->FV, fc, 0, h->r, h->GT, h->p.hmax);
      launch_rowmat_mask(st, n, h->p.wdt[lv], h->p.wdt[lv - 1], h->GT, h->p.hmax, h->W[lv], 1, h->p.wdt[lv], nullptr, 0, 0, nullptr, 0, 0,
                         h->Pv + h->p.off[lv - 1], hs, h->cfg.act, nullptr, 0, h->GPv + h->p.off[lv - 1], hs);
    }
    if (lu >= 1) {
      fl_copy_cols(st, n, h->p.wdt[lu], h->fy, wv, h->GT, h->p.hmax);
      launch_rowmat_mask(st, n, h->p.wdt[lu], h->p.wdt[lu - 1], h->GT, h->p.hmax, h->W[lu], 1, h->p.wdt[lu], nullptr, 0, 0, nullptr, 0, 0,
                         h->Pu + h->p.off[lu - 1], hs, h->cfg.act, (lu - 1 == Le - 1) ? h->Gem : nullptr, h->p.hmax,
                         h->GPu + h->p.off[lu - 1], hs);
    }
  }
  if (lv >= 1) --h->step.fs_l;
  if (lu >= 1) --h->step.fs_l2;
  h->fs_state = FS_BWD_PRODUCT;
  return GO;
}
// Tail: everything above ran beside the forked product; so do the two tiny launches of the tail that need
// nothing of it (the rank-k panels, the coefficient of the norm term), and the early passes over a cut product's finished
// rows run beside its rest.  A row-block rank holds the column block P1[:, rows]; the all-to-all of tile blocks hands it
// the row block P1[rows, :] as well.
static int fs_tail_front(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const mcgra_attack_config_t& c = h->cfg;
  const int n = s.n, ld = s.ld, R0 = s.R0, R1 = s.R1;
  const bool use1 = s.use1;
  MCGRA_KERNEL_CHECK();
  (void)tail_reduce_call(s, 1, R0, R1, s.want_vals);
  // (the coefficient of the norm term comes out of k_tail_gd's launch; a rank without rows has no Adam pass to feed)
  if (!(h->p.fused_post && R1 > R0)) hipLaunchKernelGGL(k_cn, dim3(1), dim3(1), 0, st, h->scal, (float)(c.weight_sup * 0.001), h->mm + 2);
  // (a cut product: the peers' row panels are done at ev_first; the own ones are joined behind the all-to-all)
  if (h->carry.p1_first && h->step.p1_inflight) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_first, 0));
  else {
    if (h->step.p1_inflight && h->step.tail_rows > 0) {      // the pass over the rows that are complete, beside the product's last rounds
      MCGRA_HIP(hipStreamWaitEvent(st, h->ev_first, 0));
      (void)tail_reduce_call(s, 2, 0, h->step.tail_rows, false);
      if (h->step.tail_rows2 > h->step.tail_rows) {
        MCGRA_HIP(hipStreamWaitEvent(st, h->ev_second, 0));
        (void)tail_reduce_call(s, 2, h->step.tail_rows, h->step.tail_rows2, false);
        h->step.tail_rows = h->step.tail_rows2;
      }
    } else h->step.tail_rows = 0;
    CHK(join_p1(s));
  }
  // TEST-ONLY mutation guard (tests/test_gpu_fullsize.py; armed by mcgra_attack_test_mutate, which says so on stderr): 1
  // wipes the product's result, 2 drops the rank-k terms of the tail (both GCN chains' backward and the low-rank term of
  // c2) from the gradient -- a parity test that stays green under either is blind to split2_m16_kernel / the fp16-split
  // rank-k rounds of k_tail_reduce
  if (h->test_mutate == 1 && use1) MCGRA_HIP(hipMemsetAsync(h->KX, 0, sizeof(float) * (size_t)n * ld, st));
  if (h->p.sharded && use1 && R1 > R0)
    hipLaunchKernelGGL(k_a2a_pack, dim3(2, h->p.rpr, h->p.world), dim3(256), 0, st, n, ld, h->p.rpr, R0, R1, h->p.rank, h->KX, h->A2S);
  if (!use1) return GO;
  if (h->p.sharded) x_alltoall(s.ex, h->off_a2s, h->off_a2r, (int64_t)h->p.rpr * h->p.rpr * 4);
  return AT_XCHG;
}
// The values of the loss terms that the tail's first pass sums, by FusedKind: `count` groups of partials in vpart, the slots of
// scal they belong to, and where a row-block rank's sums over the ranks stand in SC (sc0 ...: fs_decide puts them there).
//   HSIC: sum P1 o Xc | the entropy term of adj_norm;  MSELoss: sum (F - adj_norm)^2 | entropy | sum (adj_norm - A1)^2
//   (k_loss_elem's slots);  KL: calc_kl(feature_adj, adj_norm) (k_kl_rows' slot) | entropy -- c2's value came out of the decode
struct TailVals { int count, slot[3], sc0; };
static const TailVals TAIL_VALS[] = {{0, {0, 0, 0}, 0}, {2, {S_H1, S_V6, 0}, 4}, {3, {S_V1, S_V6, S_V2}, 12}, {2, {S_H1, S_V6, 0}, 12}};
// the product joined, the tail's first pass over the rows still to do, the loss terms' values and gd; a rank gathers gd
static int fs_tail_reduce(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const mcgra_attack_config_t& c = h->cfg;
  const int n = s.n, ld = s.ld, R0 = s.R0, R1 = s.R1;
  const bool use1 = s.use1, want_vals = s.want_vals;
  const TailVals& tv = TAIL_VALS[s.kind];
  CHK(join_p1(s));
  h->carry.p1_first = false;
  if (h->p.sharded && use1 && R1 > R0)
    hipLaunchKernelGGL(k_a2a_unpack, dim3(2, h->p.rpr, h->p.world), dim3(256), 0, st, n, ld, h->p.rpr, R0, R1, h->p.rank, h->A2R, h->KX);
  {
    float* ps1 = tail_ps(h);
    double* vpart = tail_vpart(h);
    h->step.fs_nblk = tail_reduce_call(s, 2, h->p.sharded ? R0 : h->step.tail_rows, R1, want_vals);
    h->step.tail_rows = 0;
    const Stage sgt = narrow_stage(h);
    if (h->p.sharded && !(h->step.fs_nblk > 0 && want_vals)) CHK(lane_zero(h, st, sgt, tv.count));
    if (h->step.fs_nblk > 0 && want_vals)
      for (int q = 0; q < tv.count; ++q)
        launch_reduce_rows(st, vpart + q * (size_t)h->step.fs_nblk, h->step.fs_nblk, 1, h->p.sharded ? lane_slot(h, sgt, q) : h->scal + tv.slot[q]);
    {
      const bool cn_in_gd = h->p.fused_post && R1 > R0;
      fl_tail_gd(st, n, R0, R1, ps1, h->d, h->gd, cn_in_gd ? h->scal + S_SQ : nullptr, (float)(c.weight_sup * 0.001),
                 cn_in_gd ? h->mm + 2 : nullptr);
    }
    if (h->p.sharded) rows_to_stage(h, st, sgt, 1, h->gd, 1, 0);
  }
  return xchg_sg(s);
}
// The decision, on the host: the masked-pair post of the decode.  A dead row hands the step to the general path (behind
// three gathers on a row-block rank); otherwise the Adam pass is next.
static int fs_decide(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  bool masked = false;
  if (h->p.sharded) {
    const Stage sgt = narrow_stage(h);
    stage_to_rows(h, st, sgt, 1, 0, h->gd, 1);
    lane_sum(h, st, sgt, TAIL_VALS[s.kind].count, h->SC + TAIL_VALS[s.kind].sc0);      // HSIC: SC[4], SC[5]; MSELoss: SC[12 .. 14]; KL: SC[12], SC[13]
  }
  if (s.use2) {
    const unsigned int want = h->mask_want;
    unsigned int spins = 0;
    while (__atomic_load_n(&h->mask_host[0], __ATOMIC_ACQUIRE) != want) {
      if ((++spins & 0xFFFF) == 0) {
        const hipError_t q = hipStreamQuery(st);       // an idle stream without the post: something was lost
        if (q != hipErrorNotReady && __atomic_load_n(&h->mask_host[0], __ATOMIC_ACQUIRE) != want) {
          set_error("masked-pair post %u never arrived (stream: %s)", want, hipGetErrorString(q));
          return MCGRA_EHIP;
        }
      }
    }
    const unsigned int code = h->mask_host[1];      // 0: no masked pair, 1: masked pairs of live rows (the step stands), 2: a dead row
    masked = code >= 2u;
    if (code == 1u) ++h->masked_fused_steps;
  }
  if (masked) h->step.fs_l = 0;      // (the gathers below count in it)
  else h->fs_state = FS_ADAM;
  return GO;
}
// relu'(0) = 0 masks a pair in the reference's backward: the low-rank algebra does not apply.  A row-block
// rank first collects the full M / am / av (own rows through the N x N stage: gather fs_l of three), then every rank
// redoes the step.
static int fs_gather_send(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int ld = s.ld, R0 = s.R0, R1 = s.R1;
  if (h->step.fs_l >= 3) {
    h->fs_state = 0;
    h->fs_open = false;
    h->step.planes_valid = false;
    return REDO;
  }
  if (h->p.sharded && R1 > R0) {
    float* src = h->step.fs_l == 0 ? h->M : (h->step.fs_l == 1 ? h->am : h->av);
    MCGRA_HIP(hipMemcpyAsync(h->NXS + (size_t)R0 * ld, src + (size_t)R0 * ld, sizeof(float) * (size_t)(R1 - R0) * ld,
                             hipMemcpyDeviceToDevice, st));
  }
  if (h->p.sharded) x_allgather(s.ex, h->off_nxn, (int64_t)h->p.rpr * ld * 4);
  return AT_XCHG;
}
static int fs_gather_recv(FusedStep& s) {
  mcgra_attack* h = s.h;
  if (h->p.sharded) {
    float* dst = h->step.fs_l == 0 ? h->M : (h->step.fs_l == 1 ? h->am : h->av);
    MCGRA_HIP(hipMemcpyAsync(dst, h->NXS, sizeof(float) * (size_t)s.n * s.ld, hipMemcpyDeviceToDevice, s.st));
  }
  ++h->step.fs_l;
  h->fs_state = FS_GATHER_SEND;
  return GO;
}
// the Adam pass -- the first kernel of the step that changes persistent state -- and the host's bookkeeping; a rank that
// was asked for scalars gathers its share of the clamp sum
static int fs_adam(FusedStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st;
  const int n = s.n, ld = s.ld, R0 = s.R0, R1 = s.R1;
  const size_t cnt = (size_t)n * s.nt;      // (the Adam pass's row partials of the new M: adam_row_sums)
  // step t + 1: the host's count moves in fused_commit, whose prep_valid is the same adam_emits_partials
  fl_tail_adam(st, n, ld, s.pair, R0, R1, h->G_ADJN, h->gd, adam_update(h, h->t + 1, adam_emits_partials(h, cnt) ? cnt : 0),
               /* the Adam moments are only ever read back through the lower tile pairs (by this kernel and by the general
                  path's tail kernels): their mirrored halves are not written */ 0);
  MCGRA_KERNEL_CHECK();
  fused_commit(h);
  if (may_project(h)) { CHK(project(h, st)); h->carry.prep_valid = false; }      // (monolithic only: refused at create otherwise)
  if (h->p.sharded && h->fs_want) {
    // sum(clamp(adj_changes, 0, 1)) after the update = the row sums the Adam pass just left behind, own rows
    prep_from_partials(st, n, h->G_A, adam_row_sums(h, cnt), h->d, h->r, h->rowsq, h->rowsum, R0, R1);
    const Stage sgc = narrow_stage(h);
    if (R1 > R0) launch_reduce_rows(st, h->rowsum + R0, R1 - R0, 1, lane_slot(h, sgc, 0));
    else CHK(lane_zero(h, st, sgc, 1));
  }
  return h->fs_want ? xchg_sg(s) : GO;
}
// A row-block rank's returned loss terms: summed over the ranks into SC (fs_lr_t, fs_decide, below), then to their slots of scal:
// the tail's values (TAIL_VALS), KL's c2 (SC[11], from the decode) and the clamp sum
static int fs_scalars(FusedStep& s) {
  mcgra_attack* h = s.h;
  if (!(h->p.sharded && h->fs_want)) return GO;
  lane_sum(h, s.st, narrow_stage(h), 1, h->SC + 6);
  const TailVals& tv = TAIL_VALS[s.kind];
  auto copy = [&](int slot, int sc) { return hipMemcpyAsync(h->scal + slot, h->SC + sc, sizeof(double), hipMemcpyDeviceToDevice, s.st); };
  for (int q = 0; q < tv.count; ++q) MCGRA_HIP(copy(tv.slot[q], tv.sc0 + q));
  if (s.kl()) MCGRA_HIP(copy(S_H2, 11));
  MCGRA_HIP(copy(S_CLAMPSUM, 6));
  return GO;
}
static const FusedStage FS_STAGES[FS_COUNT] = {
    fs_begin,       fs_forward,  fs_pack_fork,  fs_head_bwd,   fs_decode_stats, fs_decode, fs_lr_prep,     fs_small_terms,
    fs_lr_t,        fs_lr_q,     fs_decode_bwd, fs_bwd_product, fs_bwd_post,    fs_tail_front, fs_tail_reduce, fs_decide,
    fs_gather_send, fs_gather_recv, fs_adam,    fs_scalars};

// Returns 1 at an exchange point, 0 when the step is done, 2 when the step must be redone by the general path (a
// relu-masked pair in the decode; every rank then holds the full M / am / av), < 0 on error.
static int fused_step_pt(mcgra_attack* h, hipStream_t st, mcgra_exchange_t* ex) {
  FusedStep s = fused_ctx(h, st, ex);
  const int rc = run_stages(s, FS_STAGES, FS_COUNT, h->fs_state);
  if (rc != GO) return rc;
  h->fs_state = 0;
  h->fs_open = false;
  return 0;
}

int fused_step(mcgra_attack* h, hipStream_t st, double* scalars_out) {      // monolithic engines only
  h->fs_state = 0;
  h->fs_want = scalars_out ? 1 : 0;
  const int rc = fused_step_pt(h, st, nullptr);
  if (rc == 2) return 1;
  if (rc != 0) return rc;
  if (scalars_out) CHK(collect_scalars(h, st, scalars_out));
  return 0;
}

extern "C" {

int64_t mcgra_attack_exchange_bytes(mcgra_attack_t* h) { return h ? fused_exchange_bytes(h) : 0; }

int mcgra_attack_bind_exchange(mcgra_attack_t* h, void* arena, int64_t bytes) {
  if (!h || !arena) { set_error("null argument"); return MCGRA_EINVAL; }
  if (!h->p.sharded) { set_error("not a row-block rank (shard_world == 0)"); return MCGRA_EINVAL; }
  if (bytes < fused_exchange_bytes(h) || ((uintptr_t)arena & 255)) { set_error("exchange arena too small or not 256-byte aligned"); return MCGRA_EINVAL; }
  const int64_t a = 256;
  auto up = [&](int64_t x) { return (x + a - 1) / a * a; };
  h->arena = (char*)arena; h->arena_bytes = bytes;
  int64_t o = 0;
  h->off_fy = o; o += up((int64_t)h->p.npad * h->p.fyw * 4);
  h->off_sg = o; o += up((int64_t)h->p.npad * h->p.sgw * 4);
  h->off_sc = o; o += up(16 * 8);
  h->off_a2s = o; o += up((int64_t)h->p.world * h->p.rpr * h->p.rpr * 4);
  h->off_a2r = o; o += up((int64_t)h->p.world * h->p.rpr * h->p.rpr * 4);
  h->off_nxn = o;
  h->FY = (float*)(h->arena + h->off_fy); h->SG = (float*)(h->arena + h->off_sg); h->SC = (double*)(h->arena + h->off_sc);
  h->A2S = (float*)(h->arena + h->off_a2s); h->A2R = (float*)(h->arena + h->off_a2r); h->NXS = (float*)(h->arena + h->off_nxn);
  MCGRA_HIP(hipMemset(arena, 0, (size_t)fused_exchange_bytes(h)));
  return 0;
}

int mcgra_attack_shard_begin(mcgra_attack_t* h, void* stream, int what, int want_scalars) {
  (void)stream;
  if (!h || !h->graph_set) { set_error("engine not set up"); return MCGRA_EINVAL; }
  if (!h->p.sharded || !h->arena) { set_error("not a row-block rank, or no exchange arena bound"); return MCGRA_EINVAL; }
  if (what != MCGRA_SHARD_STEP && what != MCGRA_SHARD_MONITOR && what != MCGRA_SHARD_MONITOR_LAST) { set_error("what = %d", what); return MCGRA_EINVAL; }
  // a step that was begun and never ran to XCHG_DONE (the caller gave up on a collective): its leftovers are dropped
  // by fused_resync at the top of the next step (fs_open is still set); a monitor call holds no such state
  // Rule: none (no stream work).  An abandoned monitoring forward overwrote part of what the last one left:
  if (h->fs_active && h->fs_what == MCGRA_SHARD_MONITOR) h->carry.fused_fwd_valid = false;
  h->fs_last = what == MCGRA_SHARD_MONITOR_LAST;
  if (h->fs_last) what = MCGRA_SHARD_MONITOR;
  h->fs_what = what; h->fs_want = want_scalars ? 1 : 0;
  h->fs_state = 0; h->fw_state = 0;
  h->fs_active = true;
  if (what == MCGRA_SHARD_STEP && h->p.world > 1) h->m_is_full = false;      // from here on only the own rows of M are kept current
  return 0;
}

int mcgra_attack_shard_next(mcgra_attack_t* h, void* stream, mcgra_exchange_t* ex) {
  if (!h || !ex) { set_error("null argument"); return MCGRA_EINVAL; }
  if (!h->fs_active) { set_error("mcgra_attack_shard_begin first"); return MCGRA_EINVAL; }
  // Rule: as monitor (none; fork_p1_early drops in front of a second fork) / as step (fs_begin and fs_pack_fork take, step_general drops)
  hipStream_t st = (hipStream_t)stream;
  ex->kind = MCGRA_XCHG_DONE; ex->count = 0; ex->offset = ex->offset2 = ex->chunk_bytes = 0;
  int rc;
  if (h->fs_what == MCGRA_SHARD_MONITOR) {
    rc = fused_forward_pt(h, st, ex);
    if (rc == 1) return 0;
    h->fs_active = false;
    if (rc < 0) return rc;
    h->carry.fused_fwd_valid = true;
    return 0;
  }
  rc = fused_step_pt(h, st, ex);
  if (rc == 1) return 0;
  if (rc == 2) {      // every rank holds the full state now: the general path redoes the step, replicated
    rc = step_general(h, stream, nullptr, h->fs_want ? h->fs_scalars : nullptr);
    if (rc == 0) h->m_is_full = true;      // (shard_begin cleared it; the replicated step left every row of M current on every rank)
    h->fs_active = false;
    h->fs_want = h->fs_want ? 2 : 0;       // scalars already collected
    return rc;
  }
  h->fs_active = false;
  return rc;
}

int mcgra_attack_shard_scalars(mcgra_attack_t* h, void* stream, double* out) {      // Rule: none.  It reads scalar slots the caller's stream wrote.
  if (!h || !out) { set_error("null argument"); return MCGRA_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  if (h->fs_what == MCGRA_SHARD_MONITOR) {
    double s;
    MCGRA_HIP(hipMemcpyAsync(&s, h->scal + S_SUM, sizeof(double), hipMemcpyDeviceToHost, st));
    MCGRA_HIP(hipStreamSynchronize(st));
    out[0] = s / ((double)h->p.n * h->p.n);
    return 0;
  }
  if (h->fs_want == 2) { for (int i = 0; i < 10; ++i) out[i] = h->fs_scalars[i]; return 0; }
  if (h->fs_want != 1) { set_error("the step was begun without want_scalars"); return MCGRA_EINVAL; }
  return collect_scalars(h, st, out, true);
}

int mcgra_attack_test_mutate(mcgra_attack_t* h, int what) {
  if (!h || what < 0 || what > 4) { set_error("test_mutate: what = %d", what); return MCGRA_EINVAL; }
  if (what && !h->p.testing) {
    set_error("mcgra_attack_test_mutate: refused -- this engine was not created under MCGRA_TESTING=1 (a defect injector for the "
              "parity suite's mutation guards, never part of a real run)");
    return MCGRA_EINVAL;
  }
  h->test_mutate = what;
  if (what)
    fprintf(stderr, "[mcgra] TEST MUTATION ARMED on engine %p: the fused step now %s -- its gradients are WRONG on purpose\n", (void*)h,
            what == 1   ? "wipes the N x N x N product's result"
            : what == 2 ? "drops the rank-k terms of its tail"
            : what == 3 ? "drops the measure's per-pair terms (MSELoss / KL c1, c2)"
                        : "wipes the KL row statistics");
  return 0;
}

int mcgra_attack_product_replay(mcgra_attack_t* h, void* stream, int reps, double* ms_per_launch) {
  if (!h || reps < 1) { set_error("bad argument"); return MCGRA_EINVAL; }
  if (!fused_ok(h) || h->p.elementwise() || !h->carry.fused_last || h->cfg.w[0] == 0.f) {
    set_error("product_replay: the last step must have been a fused low-rank step with the c1 term (w1 != 0)");
    return MCGRA_EINVAL;
  }
  // the operand planes of the last step's product are still in Apack / Bpack (Bpack no longer describes M, which does not
  // matter here); KX and KY are scratch between steps
  hipStream_t st = (hipStream_t)stream;
  const int P = split3_panel(), p_off = h->p.row0 / P, p_cnt = h->p.row1 > h->p.row0 ? (h->p.row1 - h->p.row0 + P - 1) / P : 0;
  if (p_cnt == 0) { if (ms_per_launch) *ms_per_launch = 0.0; return 0; }
  // Rule: wait.  Planes a monitor call is still packing are equally valid operands, and a product a row-block rank's forward forked
  // writes the same scratch.  (The Kx wait it includes never fires here: kx_early_on requires !lr_ok, this call a fused low-rank step.)
  CHK(carry_wait(h, st));
  hipEvent_t e0, e1;
  MCGRA_HIP(hipEventCreate(&e0));
  MCGRA_HIP(hipEventCreate(&e1));
  MCGRA_HIP(hipEventRecord(e0, st));
  for (int i = 0; i < reps; ++i)
    MCGRA_HIP(split3_symm(st, h->p.n, h->Apack, h->Bpack, h->KX, h->p.ld, 0, -1, h->KY, sizeof(float) * (size_t)h->p.n * h->p.ld, h->p.split_planes,
                          h->amax, p_off, p_cnt, h->p.split_single ? 8 : 0));
  MCGRA_HIP(hipEventRecord(e1, st));
  MCGRA_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  MCGRA_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (ms_per_launch) *ms_per_launch = (double)ms / reps;
  // (no engine state is touched: the next step packs its own planes)
  return 0;
}

int mcgra_attack_get_rows(mcgra_attack_t* h, void* stream, float* out) {      // Rule: none.  It reads M, which whatever is in flight also only reads.
  if (!h || !out) { set_error("null argument"); return MCGRA_EINVAL; }
  const int r0 = h->p.sharded ? h->p.row0 : 0, r1 = h->p.sharded ? h->p.row1 : h->p.n;
  if (r1 > r0)
    MCGRA_HIP(hipMemcpy2DAsync(out, (size_t)h->p.n * 4, h->M + (size_t)r0 * h->p.ld, (size_t)h->p.ld * 4, (size_t)h->p.n * 4, r1 - r0,
                               hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
