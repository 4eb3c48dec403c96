// Attack engine: one iteration of PGDAttack.attack's loop
// (topology_attack.py:161-298) as a fixed sequence of HIP launches on one
// stream, with a hand-derived backward (no autograd).  Host code only enqueues;
// nothing here reads device memory back unless the caller asks for scalars.
//
// State layout in HBM (all fp32, leading dimension ld = round_up(n, 32)):
//   M            learnable adjacency, dense symmetric, zero diagonal
//                (adj_changes of the reference is its strict lower triangle)
//   am, av       Adam moments, same layout (mirrored halves stay identical
//                because the packed gradient is mirrored)
//   ADJN, A1     adj_norm and modified_adj1 of the current step
//   G_ADJN, G_A1, G_A   gradients w.r.t. those and w.r.t. modified_adj
//   KX, KY, KFC  Gram matrices of linear_HSIC on N x N operands
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <mutex>
#include <vector>

#include "../../include/mcgra.h"
#include "common.h"
#include "kernels.h"

namespace mcgra {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_err; }

}  // namespace mcgra

#include "engine.h"

using namespace mcgra;

template <typename T>
static int dalloc(mcgra_attack* h, T** p, size_t count) {
  void* q = nullptr;
  if (count == 0) count = 1;
  hipError_t e = hipMalloc(&q, count * sizeof(T));
  if (e != hipSuccess) {
    set_error("hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    return MCGRA_ENOMEM;
  }
  e = hipMemset(q, 0, count * sizeof(T));
  if (e != hipSuccess) { set_error("hipMemset: %s", hipGetErrorString(e)); return MCGRA_EHIP; }
  h->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

// HIP-event bracket around the N x N x N launches of the MFMA GEMM (roofline numbers of bench.py)
int timer_begin(mcgra_attack* h, hipStream_t st, bool big) {
  if (!big) return 0;
  GemmTimer& T = h->timer;
  if (T.used + 2 > T.ev.size()) {
    for (int i = 0; i < 2; ++i) { hipEvent_t e; MCGRA_HIP(hipEventCreate(&e)); T.ev.push_back(e); }
  }
  MCGRA_HIP(hipEventRecord(T.ev[T.used], st));
  return 0;
}
int timer_end(mcgra_attack* h, hipStream_t st, bool big, double flops) {
  if (!big) return 0;
  GemmTimer& T = h->timer;
  MCGRA_HIP(hipEventRecord(T.ev[T.used + 1], st));
  T.used += 2;
  T.launches += 1;
  T.flops += flops;     // multiply-adds actually issued (a SYRK launch counts its lower tiles only)
  return 0;
}

// every GEMM of the engine goes through here (timed when profiling)
int eg(mcgra_attack* h, hipStream_t st, bool ta, bool tb, int M, int N, int K, float alpha, const float* A,
              int lda, const float* B, int ldb, float beta, float* C, int ldc, YView* keep) {
  const bool big = h->profile && (double)M * N * K >= 0.25 * (double)h->p.n * h->p.n * h->p.n;
  CHK(timer_begin(h, st, big));
  MCGRA_HIP(sgemm(st, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, h->ws, h->ws_bytes, keep));
  return timer_end(h, st, big, 2.0 * M * N * K);
}
// C = A A^T (A is [n x k]) on lower tile storage.  (A2, C2): second Gram in the same launch.
static int eg_syrk(mcgra_attack* h, hipStream_t st, int n, int k, const float* A, int lda, float* C, int ldc,
                   const float* A2 = nullptr, float* C2 = nullptr) {
  CHK(timer_begin(h, st, h->profile));
  MCGRA_HIP(ssyrk_lower(st, n, k, 1.f, A, lda, 0.f, C, ldc, A2, C2));
  const double tb = (n + SYM_TILE - 1) / SYM_TILE;      // tile rows: tb (tb + 1) / 2 lower tiles
  return timer_end(h, st, h->profile, (C2 ? 2.0 : 1.0) * 2.0 * (tb * (tb + 1) / 2) * SYM_TILE * SYM_TILE * k);
}
// C = S B + beta C (S symmetric [n x n] in lower tile storage, B [n x m]).  (S2, B2, C2): second product in the same launch.
static int eg_symm(mcgra_attack* h, hipStream_t st, int n, int m, const float* S, int lds_, const float* B, int ldb, float beta,
                   float* C, int ldc, const float* S2 = nullptr, const float* B2 = nullptr, float* C2 = nullptr) {
  CHK(timer_begin(h, st, h->profile));
  MCGRA_HIP(ssymm_lower(st, n, m, 1.f, S, lds_, B, ldb, beta, C, ldc, S2, B2, C2));
  return timer_end(h, st, h->profile, (C2 ? 2.0 : 1.0) * 2.0 * n * (double)m * n);
}

// x = relu(adj @ (x W_l) + b_l) for `depth` layers (models/gcn.py:71-76,164-172).
// T[:, off[0]..] must already hold T_0 = X W_0.
int chain_forward(mcgra_attack* h, hipStream_t st, const float* adj, int adj_ld, int depth, float* T, float* P,
                         float* H, float* S) {
  const int n = h->p.n, hs = h->p.hsum;
  for (int l = 0; l < depth; ++l) {
    const bool next = l + 1 < h->p.L;
    if (!h->cfg.has_self && chain_post_fits(h->p.wdt[l], next ? h->p.wdt[l + 1] : 0)) {
      // the product stays in its split-K slabs and ONE launch sums them, adds the bias, applies the activation and forms the
      // next layer's T = H W_{l+1} (sum_slabs_kernel + k_bias_relu + k_rowmat: the same operations in the same order)
      YView y{nullptr, 0, 1, 0};
      CHK(eg(h, st, false, false, n, h->p.wdt[l], n, 1.f, adj, adj_ld, T + h->p.off[l], hs, 0.f, h->Y, h->p.hmax, &y));
      launch_chain_post(st, n, h->p.wdt[l], y, h->b[l], h->cfg.act, P + h->p.off[l], H + h->p.off[l], hs, next ? h->p.wdt[l + 1] : 0,
                        next ? h->W[l + 1] : nullptr, next ? h->p.wdt[l + 1] : 0, 1, nullptr, next ? T + h->p.off[l + 1] : nullptr, hs);
      continue;
    }
    CHK(eg(h, st, false, false, n, h->p.wdt[l], n, 1.f, adj, adj_ld, T + h->p.off[l], hs, 0.f, h->Y, h->p.hmax));
    const float* self = !h->cfg.has_self ? nullptr : (l == 0 ? h->S0 : S + h->p.off[l]);
    launch_bias_relu(st, n, h->p.wdt[l], h->Y, h->p.hmax, h->b[l], self, l == 0 ? h->p.hmax : hs, h->cfg.act, P + h->p.off[l],
                     H + h->p.off[l], hs);
    if (l + 1 < h->p.L) {
      launch_rowmat(st, n, h->p.wdt[l], h->p.wdt[l + 1], H + h->p.off[l], hs, h->W[l + 1], h->p.wdt[l + 1], 1, nullptr,
                    T + h->p.off[l + 1], hs);
      if (h->cfg.has_self)   // x W_top of the next GraphSAGE layer (graphsage.py:44-45)
        launch_rowmat(st, n, h->p.wdt[l], h->p.wdt[l + 1], H + h->p.off[l], hs, h->Ws[l + 1], h->p.wdt[l + 1], 1, nullptr,
                      S + h->p.off[l + 1], hs);
    }
  }
  MCGRA_KERNEL_CHECK();
  return 0;
}

// linear1 + log_softmax (models/gcn.py:173-174)
int head_forward(mcgra_attack* h, hipStream_t st, const float* H, float* Z, float* logp, float* sm) {
  const int l = h->p.L - 1;
  launch_rowmat(st, h->p.n, h->p.wdt[l], h->p.C, H + h->p.off[l], h->p.hsum, h->Wlin, 1, h->p.wdt[l], h->blin, Z, h->p.C);
  launch_log_softmax(st, h->p.n, h->p.C, Z, h->p.C, logp, sm, h->p.C, h->cfg.head_act);   // Z keeps the linear output
  MCGRA_KERNEL_CHECK();
  return 0;
}

// Backward through layers ltop..0 of a chain.  GP[:, off[ltop]] holds G_P_ltop on
// entry.  add_at/Add: extra gradient w.r.t. H_{add_at} (e.g. d loss / d em).
int chain_backward(mcgra_attack* h, hipStream_t st, const float* adj, int adj_ld, int ltop, const float* P,
                          float* GP, int add_at, const float* Add, int add_ld) {
  const int n = h->p.n, hs = h->p.hsum;
  for (int l = ltop; l >= 1; --l) {
    if (!h->cfg.has_self && chain_post_fits(h->p.wdt[l], h->p.wdt[l - 1])) {
      // G_T_l left in its split-K slabs, summed by the linear backward that reads it (one launch less per level)
      YView y{nullptr, 0, 1, 0};
      CHK(eg(h, st, true, false, n, h->p.wdt[l], n, 1.f, adj, adj_ld, GP + h->p.off[l], hs, 0.f, h->GT, h->p.hmax, &y));
      launch_rowmat_mask_view(st, n, h->p.wdt[l], h->p.wdt[l - 1], y, h->W[l], 1, h->p.wdt[l], P + h->p.off[l - 1], hs, h->cfg.act,
                              (l - 1 == add_at) ? Add : nullptr, add_ld, GP + h->p.off[l - 1], hs);
      continue;
    }
    // G_T_l = adj^T @ G_P_l
    CHK(eg(h, st, true, false, n, h->p.wdt[l], n, 1.f, adj, adj_ld, GP + h->p.off[l], hs, 0.f, h->GT, h->p.hmax));
    // G_P_{l-1} = (G_T_l @ W_l^T [+ Add]) * (P_{l-1} > 0)
    // (+ G_P_l @ Ws_l^T: the self path of a GraphSAGE layer)
    launch_rowmat_mask(st, n, h->p.wdt[l], h->p.wdt[l - 1], h->GT, h->p.hmax, h->W[l], 1, h->p.wdt[l],
                       h->cfg.has_self ? GP + h->p.off[l] : nullptr, hs, h->p.wdt[l], h->Ws[l], 1, h->p.wdt[l],
                       P + h->p.off[l - 1], hs, h->cfg.act, (l - 1 == add_at) ? Add : nullptr, add_ld, GP + h->p.off[l - 1], hs);
  }
  MCGRA_KERNEL_CHECK();
  return 0;
}

double sign_of(const mcgra_attack* h) { return h->cfg.measure == MCGRA_MEASURE_HSIC ? -1.0 : 1.0; }

extern "C" {

const char* mcgra_version(void) { return "mcgra-hip 0.1 (gfx950)"; }
const char* mcgra_last_error(void) { return mcgra::last_error(); }
int mcgra_device_count(void) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) { set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return MCGRA_EHIP; }
  return c;
}

// the engine's own events (all without timing)
static hipEvent_t mcgra_attack::* const ENGINE_EVENTS[] = {
    &mcgra_attack::ev_fork4, &mcgra_attack::ev_join4, &mcgra_attack::ev_fork,  &mcgra_attack::ev_join,  &mcgra_attack::ev_first,
    &mcgra_attack::ev_second, &mcgra_attack::ev_r,    &mcgra_attack::ev_pack,  &mcgra_attack::ev_fork3, &mcgra_attack::ev_join3};

// plan (attack_plan.hip: every decision, no device), then allocate what the plan asks for, then streams and events
int mcgra_attack_create(mcgra_attack_t** out, const mcgra_attack_config_t* cfg) {
  if (!out || !cfg) { set_error("null argument"); return MCGRA_EINVAL; }
  AttackPlan plan;
  CHK(plan_attack(*cfg, read_plan_env(), &plan));
  mcgra_attack* h = new mcgra_attack(*cfg, plan);
  const AttackPlan& p = h->p;
  const size_t n = h->p.n, ld = h->p.ld, nn = n * ld;
  const int he = h->p.wdt[h->p.Le - 1];
  const bool hsic = cfg->measure == MCGRA_MEASURE_HSIC, cka = cfg->measure == MCGRA_MEASURE_CKA;
  int rc = 0;
#define A_(f, cnt) if (!rc) rc = dalloc(h, &h->f, (cnt))
  A_(M, nn); A_(am, nn); A_(av, nn); A_(ADJN, nn); A_(A1, nn); A_(G_ADJN, nn); A_(G_A1, nn); A_(G_A, nn);
  A_(KX, nn); A_(FADJ, nn);
  if (p.keep_gsym) { A_(GSYM, nn); }
  if (hsic || cka) { A_(KY, nn); A_(KFC, nn); A_(XC, nn); A_(YC, nn); }
  if (cfg->measure == MCGRA_MEASURE_KL) { A_(XC, nn); }      // XC holds softmax(feature_adj) rows
  if (cfg->measure == MCGRA_MEASURE_DP) { A_(KY, nn); A_(XC, nn); }
  if (cfg->measure == MCGRA_MEASURE_KDE) { A_(kde, kde_scratch_doubles((int)n)); }
  A_(cmean, ld); A_(d, ld); A_(r, ld); A_(rowpart, ld); A_(colpart, (size_t)h->nstrips * ld); A_(gd, ld); A_(nrm, ld); A_(cnt, ld);
  A_(rowmin, ld); A_(rowmax, ld); A_(mm, 4);
  A_(mask_seq_dev, 1);
  A_(rowsq, 2 * ld); h->rowsum = h->rowsq ? h->rowsq + n : nullptr;
  A_(rowvals, 8 * ld); A_(rowsx, ld); A_(rowsy, ld); A_(scal, S_COUNT);
  A_(labels, n); A_(idx, (size_t)h->p.na); A_(correct, 4);
  for (int l = 0; l < h->p.L && !rc; ++l) {
    rc = dalloc(h, &h->W[l], (size_t)cfg->dims[l] * cfg->dims[l + 1]);
    if (!rc) rc = dalloc(h, &h->b[l], (size_t)cfg->dims[l + 1]);
  }
  A_(Wlin, (size_t)h->p.C * h->p.wdt[h->p.L - 1]); A_(blin, (size_t)h->p.C);
  if (h->cfg.has_self) {
    for (int l = 0; l < h->p.L && !rc; ++l) rc = dalloc(h, &h->Ws[l], (size_t)cfg->dims[l] * cfg->dims[l + 1]);
    A_(S0, n * (size_t)h->p.hmax); A_(Sv, n * (size_t)h->p.hsum); A_(Su, n * (size_t)h->p.hsum);
  }
  const size_t nh = n * h->p.hsum, nm = n * h->p.hmax, nc = n * h->p.C;
  A_(Tv, nh); A_(Pv, nh); A_(Hv, nh); A_(GPv, nh); A_(Tu, nh); A_(Pu, nh); A_(Hu, nh); A_(GPu, nh);
  A_(Y, nm); A_(GT, nm); A_(Z, nc); A_(logp, nc); A_(sm, nc); A_(Z2, nc); A_(sm2, nc); A_(GZ, nc); A_(GZ2, nc); A_(Gsm, nc);
  A_(Zn, nm); A_(GZn, nm); A_(Gem, nm);
  const size_t am_ = (size_t)h->p.na * h->p.hmax;
  A_(HA, nm); A_(YA, nc); A_(HAg, am_); A_(HAc, am_); A_(YAg, am_); A_(YAc, am_); A_(Yg, am_); A_(Gg, am_);
  if (cfg->eps != 0.f) { A_(Abuf, nn); A_(gate, nn); A_(colpart_d, (size_t)h->nstrips * ld); }
  if (p.fwd_reuse) { A_(ADJN_next, nn); }
  A_(cm_part, (size_t)64 * 256);      // column-sum partials of launch_colmean_center (small-operand terms)
  if (hsic) { A_(Yg8, am_); }
  A_(Q, (size_t)h->p.hmax * h->p.hmax); A_(Q2, (size_t)h->p.hmax * h->p.hmax); A_(Gg2, am_); A_(coef, 16); A_(cst, 8);
  if (p.lr_ok) {
    A_(lrL, n * 2 * he); A_(lrR, n * 2 * he); A_(lrQ, n * 2 * he); A_(lrV, n * (size_t)h->p.lr_ldv);
    A_(lrT, n * (size_t)h->p.lr_ldv); A_(lrDelta, ld); A_(lrC, ld); A_(lrStats, lr_stats_doubles(he)); A_(lrRs, ld); A_(lrQtZ, lr_qtz_doubles(he));
  }
  A_(nmask, 4);
  // packed planes of the split products: the low-rank step's (Apack: H Kf H, per graph; Bpack: Xc) and the Gram evaluation's
  if (p.split_on) { A_(Apack, split3_pack_bytes((int)n, p.split_planes)); }
  if (p.split_on || p.gram_split) { A_(Bpack, split3_pack_bytes((int)n, p.split_planes)); A_(amax, 16); }
  if (p.gram_split) {
    const size_t pb = split3_pack_bytes((int)n, 2);
    A_(Gp0, pb); A_(Gp1, pb); A_(Gp2, pb); A_(gram_diag, 2 * ld);
  }
  if (p.planes_mm_on) { A_(pm_scratch, planes_mm_scratch_bytes((int)n)); }
  if (p.fwd_x3) { A_(sx_scratch, skinny_x3_scratch_bytes((int)n)); }
  if (p.fused) {
    const size_t fc = (size_t)p.fcols;
    A_(FV, n * fc); A_(em_last, nm); A_(fstat, 256 + fl_wcolsum_scratch_doubles());
    if (!p.sharded) { A_(FY, n * fc); }      // a row-block rank keeps FY in the exchange arena
    A_(rkbuf, fl_tail_pack_bytes((int)n));           // packed fp16 planes of the tail's rank-k panels
    A_(Zpair, (n + 2) * (size_t)h->p.hmax);
    // (a row-block rank cuts the columns of its rows' decode into up to 64 slices: fused_lowrank.hip: fl_decode_slabs)
    A_(ws_dec, (size_t)((p.sharded || p.fused != FUSED_HSIC) ? 64 : lr_decode_slabs((int)n)) * n * he);      // (MSELoss, KL: up to 64 slices too, nothing runs beside their decode)
    if (p.fused == FUSED_KL) { A_(klA, ld); A_(kl1, ld); A_(klv, ld); A_(klvsum, ld); A_(klpart, (size_t)64 * n * 2); }
  }
  if (p.split_on || p.gram_split) {      // a small graph's split products: room to cut them along K (its N x N buffers are too small)
    const size_t want = split3_small_slab_bytes((int)n);
    if (want > sizeof(float) * nn) {
      A_(small_slab, want / sizeof(float));
      if (!rc) h->small_slab_bytes = want;
    }
  }
  h->ws_bytes = (size_t)64 * n * 64 * sizeof(float);
  A_(ws, h->ws_bytes / sizeof(float));
  h->ws_small_bytes = (size_t)64 * (h->p.na > h->p.hmax ? h->p.na : h->p.hmax) * h->p.hmax * sizeof(float);
  A_(ws_small, h->ws_small_bytes / sizeof(float));
#undef A_
  if (!rc && p.side_streams) {
    int pr_least = 0, pr_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest);
    // The side streams are shared by all engines of a device in this process: a process has few hardware queues
    // (four by default), and engines beyond the first would otherwise multiplex their side streams onto the ones in
    // use (measured: a second live engine's Cora-size step went from 0.63 to 2.4 ms).  Engines of one process run
    // one after another, so sharing only adds ordering that is there anyway.
    static hipStream_t side2[64] = {nullptr}, side3[64] = {nullptr}, side4[64] = {nullptr};
    static std::mutex side_mu;                        // creation from several host threads (include/mcgra.h: "Threads")
    std::lock_guard<std::mutex> side_lock(side_mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) dev = 0;
    // the product's stream: normal priority (A/B at N = 10 000, same box: low 153.8, normal 154.8, high 154.4 steps/s;
    // round 1's fp32 SYMM, which left no room beside itself, wanted the lowest)
    const int pr2 = (pr_least + pr_greatest) / 2;
    if (!side2[dev] && hipStreamCreateWithPriority(&side2[dev], hipStreamNonBlocking, pr2) != hipSuccess) side2[dev] = nullptr;
    if (!side3[dev] && hipStreamCreateWithFlags(&side3[dev], hipStreamNonBlocking) != hipSuccess) side3[dev] = nullptr;
    if (!side4[dev] && hipStreamCreateWithFlags(&side4[dev], hipStreamNonBlocking) != hipSuccess) side4[dev] = nullptr;
    h->st2 = side2[dev]; h->st3 = side3[dev]; h->st4 = side4[dev];
    bool ok = h->st2 && h->st3 && h->st4;
    for (auto ev : ENGINE_EVENTS) ok = ok && hipEventCreateWithFlags(&(h->*ev), hipEventDisableTiming) == hipSuccess;
    // (the fused step's masked-pair count is posted to mapped host memory: engine.h: mask_host)
    if (!ok || hipHostMalloc((void**)&h->mask_host, 8, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&h->mask_host_dev, (void*)h->mask_host, 0) != hipSuccess) {
      set_error("stream / event creation failed"); rc = MCGRA_EHIP;
    }
    if (h->mask_host) { h->mask_host[0] = 0u; h->mask_host[1] = 0u; }
  }
  // the zero fills of dalloc ran on the null stream: order them in front of whatever stream the caller uses next
  if (!rc && hipDeviceSynchronize() != hipSuccess) { set_error("hipDeviceSynchronize failed after allocation"); rc = MCGRA_EHIP; }
  if (rc) { mcgra_attack_destroy(h); return rc; }
  *out = h;
  return 0;
}

int mcgra_attack_destroy(mcgra_attack_t* h) {
  if (!h) return 0;
  for (void* p : h->allocs) (void)hipFree(p);
  for (hipEvent_t e : h->timer.ev) (void)hipEventDestroy(e);
  for (hipStream_t st : {h->st2, h->st3, h->st4}) if (st) (void)hipStreamSynchronize(st);      // (shared side streams: drained, not destroyed)
  for (auto ev : ENGINE_EVENTS) if (h->*ev) (void)hipEventDestroy(h->*ev);
  if (h->mask_host) (void)hipHostFree((void*)h->mask_host);
  delete h;
  return 0;
}

int mcgra_attack_set_model(mcgra_attack_t* h, void* stream, const float* const* W, const float* const* b,
                           const float* Wlin, const float* blin, const float* const* Ws) {
  if (h) carry_forget(h);      // Rule: forget.  Nothing in flight reads the model.
  if (!h || !W || !b || !Wlin || !blin) { set_error("null argument"); return MCGRA_EINVAL; }
  if ((h->cfg.has_self != 0) != (Ws != nullptr)) { set_error("Ws must be given exactly when has_self is set"); return MCGRA_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  for (int l = 0; l < h->p.L; ++l) {
    if (Ws) MCGRA_HIP(hipMemcpyAsync(h->Ws[l], Ws[l], sizeof(float) * h->cfg.dims[l] * h->cfg.dims[l + 1], hipMemcpyDeviceToDevice, st));
    MCGRA_HIP(hipMemcpyAsync(h->W[l], W[l], sizeof(float) * h->cfg.dims[l] * h->cfg.dims[l + 1], hipMemcpyDeviceToDevice, st));
    MCGRA_HIP(hipMemcpyAsync(h->b[l], b[l], sizeof(float) * h->cfg.dims[l + 1], hipMemcpyDeviceToDevice, st));
  }
  MCGRA_HIP(hipMemcpyAsync(h->Wlin, Wlin, sizeof(float) * h->p.C * h->p.wdt[h->p.L - 1], hipMemcpyDeviceToDevice, st));
  MCGRA_HIP(hipMemcpyAsync(h->blin, blin, sizeof(float) * h->p.C, hipMemcpyDeviceToDevice, st));
  h->model_set = true;
  return 0;
}

int mcgra_attack_set_graph(mcgra_attack_t* h, void* stream, const float* features, const float* adj,
                           const float* ori_adj, const float* feature_adj, const int32_t* labels,
                           const int32_t* idx_attack) {
  if (h) carry_forget(h, true);      // Rule: drop (below, once the arguments stand) + forget.  skip_fused is kept: it only says which path goes first
  if (!h || !features || !adj || !feature_adj || !labels || !idx_attack) { set_error("null argument"); return MCGRA_EINVAL; }
  if (!h->model_set) { set_error("mcgra_attack_set_model must be called first"); return MCGRA_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  CHK(carry_drop(h, st));
  const int n = h->p.n, ld = h->p.ld, hs = h->p.hsum;
  if (ori_adj) {
    // (general path only: engine.h, has_ori)
    if (h->p.sharded) { set_error("a non-zero ori_adj is not supported on a row-block rank"); return MCGRA_ENOSUP; }
    const size_t nn = (size_t)n * ld, nh = (size_t)n * hs;
    int rc = 0;
#define A1_(f, cnt) if (!rc && !h->f) rc = dalloc(h, &h->f, (cnt))
    A1_(ORI, nn); A1_(Bbuf, nn); A1_(Abuf, nn); A1_(gate, nn); A1_(Te, nh); A1_(Pe, nh); A1_(He, nh); A1_(GPe, nh);
    if (h->cfg.has_self) { A1_(Se, nh); }
#undef A1_
    if (rc) return rc;
    MCGRA_HIP(hipMemcpy2DAsync(h->ORI, (size_t)ld * 4, ori_adj, (size_t)n * 4, (size_t)n * 4, n, hipMemcpyDeviceToDevice, st));
  }
  h->has_ori = ori_adj != nullptr;
  MCGRA_HIP(hipMemcpy2DAsync(h->FADJ, (size_t)ld * 4, feature_adj, (size_t)n * 4, (size_t)n * 4, n, hipMemcpyDeviceToDevice, st));
  MCGRA_HIP(hipMemcpyAsync(h->labels, labels, sizeof(int) * n, hipMemcpyDeviceToDevice, st));
  MCGRA_HIP(hipMemcpyAsync(h->idx, idx_attack, sizeof(int) * h->p.na, hipMemcpyDeviceToDevice, st));
  MCGRA_HIP(hipMemsetAsync(h->cnt, 0, sizeof(float) * ld, st));
  launch_count_idx(st, h->p.na, h->idx, h->cnt);
  // T0 = X @ W_0 : the only use of the features inside the loop (models/gcn.py:41)
  CHK(eg(h, st, false, false, n, h->p.wdt[0], h->cfg.dims[0], 1.f, features, h->cfg.dims[0], h->W[0], h->p.wdt[0], 0.f, h->Tv, hs));
  MCGRA_HIP(hipMemcpy2DAsync(h->Tu, (size_t)hs * 4, h->Tv, (size_t)hs * 4, (size_t)h->p.wdt[0] * 4, n, hipMemcpyDeviceToDevice, st));
  if (h->has_ori)
    MCGRA_HIP(hipMemcpy2DAsync(h->Te, (size_t)hs * 4, h->Tv, (size_t)hs * 4, (size_t)h->p.wdt[0] * 4, n, hipMemcpyDeviceToDevice, st));
  if (h->cfg.has_self)   // S0 = X @ Ws_0: the self half of the first GraphSAGE layer, adjacency independent
    CHK(eg(h, st, false, false, n, h->p.wdt[0], h->cfg.dims[0], 1.f, features, h->cfg.dims[0], h->Ws[0], h->p.wdt[0], 0.f, h->S0,
           h->p.hmax));
  // priors on the TRUE, un-normalised adjacency (topology_attack.py:177-182, :243)
  CHK(chain_forward(h, st, adj, n, h->p.L, h->Tu, h->Pu, h->Hu, h->Su));
  CHK(head_forward(h, st, h->Hu, h->Z2, h->YA, nullptr));                                  // Y_A (log-probs)
  const int le = h->p.Le - 1;
  MCGRA_HIP(hipMemcpy2DAsync(h->HA, (size_t)h->p.hmax * 4, h->Hu + h->p.off[le], (size_t)hs * 4, (size_t)h->p.wdt[le] * 4, n,
                             hipMemcpyDeviceToDevice, st));                                // H_A_cur
  launch_gather_rows(st, h->p.na, h->p.wdt[le], h->HA, h->p.hmax, h->idx, h->HAg, h->p.hmax);
  launch_gather_rows(st, h->p.na, h->p.wdt[le], h->HA, h->p.hmax, h->idx, h->HAc, h->p.hmax);
  launch_colmean_center(st, h->p.na, h->p.wdt[le], h->HAc, h->p.hmax);
  launch_gather_rows(st, h->p.na, h->p.C, h->YA, h->p.C, h->idx, h->YAg, h->p.hmax);
  launch_gather_rows(st, h->p.na, h->p.C, h->YA, h->p.C, h->idx, h->YAc, h->p.hmax);
  launch_colmean_center(st, h->p.na, h->p.C, h->YAc, h->p.hmax);
  if (h->cfg.measure == MCGRA_MEASURE_CKA) {
    // hsic(H_A, H_A), hsic(Y_A, Y_A) of linear_CKA's denominator (utils.py:1093): |Xc^T Xc|_F^2, constants
    const int hm = h->p.hmax;
    MCGRA_HIP(hipMemsetAsync(h->Q, 0, sizeof(float) * (size_t)hm * hm, st));
    CHK(eg(h, st, true, false, h->p.wdt[le], h->p.wdt[le], h->p.na, 1.f, h->HAc, hm, h->HAc, hm, 0.f, h->Q, hm));
    launch_sumsq(st, (size_t)h->p.wdt[le] * hm, h->Q, h->cst + 1);
    MCGRA_HIP(hipMemsetAsync(h->Q, 0, sizeof(float) * (size_t)hm * hm, st));
    CHK(eg(h, st, true, false, h->p.C, h->p.C, h->p.na, 1.f, h->YAc, hm, h->YAc, hm, 0.f, h->Q, hm));
    launch_sumsq(st, (size_t)h->p.C * hm, h->Q, h->cst + 2);
  }
  if ((h->cfg.measure == MCGRA_MEASURE_HSIC || h->cfg.measure == MCGRA_MEASURE_CKA) && h->cfg.w[0] != 0.f) {
    // centred Gram of feature_adj: constant left factor of c1 (utils.py:1086,1089), from centred columns
    launch_rowsum(st, n, ld, h->FADJ, h->rowsx);
    launch_center_cols(st, n, ld, h->FADJ, h->rowsx, h->cmean, h->XC);
    CHK(eg(h, st, false, true, n, n, n, 1.f, h->XC, ld, h->XC, ld, 0.f, h->KFC, ld));
    if (h->p.split_mode == 2) {
      if (h->p.split_planes == 2) {
        MCGRA_HIP(hipMemsetAsync(h->amax, 0, sizeof(float), st));
        split_absmax(st, n, ld, h->KFC, nullptr, true, h->amax);
      }
      split3_pack(st, n, ld, h->KFC, nullptr, true, h->Apack, h->p.split_planes, h->amax);
    }
    if (gram_split(h)) {      // max |H Kf H|: part of the scale bound of the combined Gram (split_symm_bf16.hip: k_gram_scales)
      MCGRA_HIP(hipMemsetAsync(h->amax + 5, 0, sizeof(float), st));
      split_absmax(st, n, ld, h->KFC, nullptr, false, h->amax + 5);
    }
    launch_rowsumsq(st, n, ld, h->KFC, h->rowsx);
    launch_reduce_rows(st, h->rowsx, n, 1, h->cst + 0);      // hsic(feature_adj, feature_adj)
  }
  if (h->cfg.measure == MCGRA_MEASURE_KL && h->cfg.w[0] != 0.f)
    launch_row_softmax(st, n, ld, h->FADJ, h->XC);      // F.softmax(feature_adj) of calc_kl (:484), constant
  if (h->cfg.measure == MCGRA_MEASURE_KDE) {           // largest magnitude of the caller's feature_adj: how many columns its bins reach (below)
    MCGRA_HIP(hipMemsetAsync(h->coef, 0, sizeof(float), st));
    split_absmax(st, n, ld, h->FADJ, nullptr, false, h->coef);
  }
  // (small_term's HSIC branch relies on zero pad columns in Q / Q2: see there)
  MCGRA_HIP(hipMemsetAsync(h->Q, 0, sizeof(float) * (size_t)h->p.hmax * h->p.hmax, st));
  MCGRA_HIP(hipMemsetAsync(h->Q2, 0, sizeof(float) * (size_t)h->p.hmax * h->p.hmax, st));
  h->step.t3_zero = false;
  MCGRA_KERNEL_CHECK();
  // feature_adj.max() != feature_adj.min() (topology_attack.py:212) is evaluated by the host layer
  MCGRA_HIP(hipStreamSynchronize(st));
  if (h->cfg.measure == MCGRA_MEASURE_KDE) {
    // utils.MutualInformation on an N x N operand: entry (i, j) meets bin j only (utils.py:995), b_j >= j, and the float32 kernel
    // value is exactly 0 once b_j - v > 4.6 (kde_kernels.hip).  adj_norm and modified_adj1 live in [0, 1] ([0, 2] with ori_adj) by
    // construction -- 8 columns; feature_adj is the caller's: its largest magnitude decides how far the bins reach.
    float fmax_ = 0.f;
    MCGRA_HIP(hipMemcpy(&fmax_, h->coef, sizeof(float), hipMemcpyDeviceToHost));
    if (!(fmax_ < 1e30f)) { set_error("measure KDE: feature_adj holds a non-finite value"); return MCGRA_EINVAL; }
    int cols = (int)floorf(fmax_ + 4.7f) + 1;
    if (cols < KDE_NXN_COLS) cols = KDE_NXN_COLS;
    if (cols > n) cols = n;
    if (cols > KDE_MAXC) {
      set_error("measure KDE: max |feature_adj| = %g puts %d bins of utils.MutualInformation within reach of its values; the N x N terms "
                "are evaluated on at most %d columns (values <= %.1f)", (double)fmax_, cols, KDE_MAXC, (double)KDE_MAXC - 4.7);
      return MCGRA_ENOSUP;
    }
    h->kde_cols = cols;
  }
  h->graph_set = true;
  return 0;
}

int mcgra_attack_set_adj_changes(mcgra_attack_t* h, void* stream, const float* packed) {
  if (h) carry_forget(h);      // Rule: drop + forget.  A pack or product of the old M may still be reading it on the side stream.
  if (!h || !packed) { set_error("null argument"); return MCGRA_EINVAL; }
  CHK(carry_drop(h, (hipStream_t)stream));
  launch_unpack_sym((hipStream_t)stream, h->p.n, h->p.ld, packed, nullptr, 0, h->M);
  MCGRA_KERNEL_CHECK();
  h->m_is_full = true;
  return 0;
}
int mcgra_attack_get_adj_changes(mcgra_attack_t* h, void* stream, float* packed) {      // Rule: none.  It reads M, which whatever is in flight also only reads.
  if (!h || !packed) { set_error("null argument"); return MCGRA_EINVAL; }
  if (h->p.sharded && !h->m_is_full) { set_error("row-block rank: only rows [row_begin, row_end) are kept between a step and mcgra_attack_finalize (mcgra_attack_get_rows)"); return MCGRA_EINVAL; }
  launch_pack_tril((hipStream_t)stream, h->p.n, h->p.ld, h->M, packed, false);
  MCGRA_KERNEL_CHECK();
  return 0;
}

// calc(X[idx], Y[idx]) on small operands: gradient w.r.t. Y scattered into G (zero-filled by caller).
// Xg raw gathered constant, Xc its column-centred copy.  Value lands in scal[slot].
int small_term(mcgra_attack* h, hipStream_t st, int width, const float* Ysrc, int ldy, const float* Xg,
                      const float* Xc, double k_signed, float* G, int ldg, int slot, bool want_value) {
  const int na = h->p.na, hm = h->p.hmax;
  // (own split-K workspace: the fused step runs this chain on a side stream, beside products that use h->ws)
  auto eg = [](mcgra_attack* h, hipStream_t st, bool ta, bool tb, int M, int N, int K, float alpha, const float* A, int lda,
               const float* B, int ldb, float beta, float* C, int ldc) -> int {
    MCGRA_HIP(sgemm(st, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, h->ws_small, h->ws_small_bytes));
    return 0;
  };
  if (h->cfg.measure == MCGRA_MEASURE_MSE) {      // gather, value partials, gradient and scatter in one launch (+ the value's sum)
    launch_mse_small_fused(st, na, width, Xg, hm, Ysrc, ldy, h->idx, (float)k_signed, G, ldg, h->scal + slot, h->cm_part, want_value);
    MCGRA_KERNEL_CHECK();
    return 0;
  }
  const bool y8 = h->cfg.measure == MCGRA_MEASURE_HSIC && Ysrc == h->sm2;      // c10: centred from the logits in float64, below
  if (!y8) launch_gather_rows(st, na, width, Ysrc, ldy, h->idx, h->Yg, hm);
  if (h->cfg.measure == MCGRA_MEASURE_CKA) {
    // linear_CKA(X, Y) (utils.py:1091-1096): value hxy / (sqrt(hxx) sqrt(hyy)); Q = Xc^T Yc, R = Yc^T Yc,
    // d/dY = (2/den) Xc Q - (2 hxy / (den hyy)) Yc R.  hxx is the constant in cst[cst_slot].
    launch_colmean_center(st, na, width, h->Yg, hm, h->cm_part);
    MCGRA_HIP(hipMemsetAsync(h->Q, 0, sizeof(float) * (size_t)hm * hm, st));
    MCGRA_HIP(hipMemsetAsync(h->Q2, 0, sizeof(float) * (size_t)hm * hm, st));
    CHK(eg(h, st, true, false, width, width, na, 1.f, Xc, hm, h->Yg, hm, 0.f, h->Q, hm));
    CHK(eg(h, st, true, false, width, width, na, 1.f, h->Yg, hm, h->Yg, hm, 0.f, h->Q2, hm));
    launch_sumsq(st, (size_t)width * hm, h->Q, h->scal + S_TMP);
    launch_sumsq(st, (size_t)width * hm, h->Q2, h->scal + S_TMP2);
    float* ab = h->coef + (slot == S_C9 ? 8 : 12);
    launch_cka_small_coef(st, h->cst + (slot == S_C9 ? 1 : 2), h->scal + S_TMP, h->scal + S_TMP2, (float)k_signed, ab,
                          h->scal + slot);
    CHK(eg(h, st, false, false, na, width, width, 1.f, Xc, hm, h->Q, hm, 0.f, h->Gg, hm));
    CHK(eg(h, st, false, false, na, width, width, 1.f, h->Yg, hm, h->Q2, hm, 0.f, h->Gg2, hm));
    launch_scatter_add2_rows(st, na, width, h->Gg, h->Gg2, hm, h->idx, ab, G, ldg);
  } else if (h->cfg.measure == MCGRA_MEASURE_DP) {   // |Y^T X|_F (:480-481): P = Yg^T Xg, d/dY = X P^T / |P|
    MCGRA_HIP(hipMemsetAsync(h->Q, 0, sizeof(float) * (size_t)hm * hm, st));
    CHK(eg(h, st, true, false, width, width, na, 1.f, h->Yg, hm, Xg, hm, 0.f, h->Q, hm));
    launch_sumsq(st, (size_t)width * hm, h->Q, h->scal + slot);
    CHK(eg(h, st, false, true, na, width, width, 1.f, Xg, hm, h->Q, hm, 0.f, h->Gg, hm));
    launch_scatter_add_rows_invnorm(st, na, width, h->Gg, hm, h->idx, h->scal + slot, (float)k_signed, G, ldg);
  } else if (h->cfg.measure == MCGRA_MEASURE_KDE) {
    // MutualInformation(num_bins = width)(X[idx], Y[idx])[0] (:244-249, :261-265): k_signed d / dY, rows scattered back
    launch_kde_term(st, na, width, width, Xg, hm, h->Yg, hm, k_signed, nullptr, 0, false, h->Gg, hm, false, h->scal + slot, h->kde);
    launch_scatter_add_rows(st, na, width, h->Gg, hm, h->idx, 1.f, G, ldg);
  } else if (h->cfg.measure == MCGRA_MEASURE_KL) {   // calc_kl(X[idx], Y[idx]) (:483-487), X constant
    launch_kl_small(st, na, width, Xg, h->Yg, hm, h->Gg, h->rowvals + 7 * (size_t)h->p.ld);
    launch_reduce_rows(st, h->rowvals + 7 * (size_t)h->p.ld, na, 1, h->scal + slot);
    launch_scatter_add_rows(st, na, width, h->Gg, hm, h->idx, (float)k_signed, G, ldg);
  } else {  // HSIC: value |Xc^T Yc|_F^2, gradient 2 Xc (Xc^T Yc)   (utils.py:1085-1089)
    // Y is centred explicitly: Xc^T Y == Xc^T Yc only in exact arithmetic, and with identical rows of Y
    // (adj_changes == 0) the fp32 residue of Xc's column sums would otherwise be the whole "gradient"
    // (c10: Y = softmax(output2) is nearly the same row on every node, so the STORED float32 softmax has lost most of what the
    //  centring keeps -- 4.8e-5 of the term's gradient on a 3-layer victim at n = 80, against 8e-6 with the rows recomputed from
    //  the logits in float64 and rounded after the centring: node_kernels.hip, k_softmax8_gather)
    if (y8) launch_softmax8_centered(st, na, width, h->Z2, h->p.C, h->idx, h->cfg.head_act, h->Yg8, h->Yg, hm, h->cm_part);
    else launch_colmean_center(st, na, width, h->Yg, hm, h->cm_part);
    // one Q per term (c9: Q, c10: Q2): each is only ever written on its term's width x width block, so its pad columns
    // keep the zeros of the allocation and no fill is needed per step
    float* Qb = slot == S_C10 ? h->Q2 : h->Q;
    CHK(eg(h, st, true, false, width, width, na, 1.f, Xc, hm, h->Yg, hm, 0.f, Qb, hm));
    if (want_value) launch_sumsq(st, (size_t)width * hm, Qb, h->scal + slot);              // pad columns of Q are zero
    CHK(eg(h, st, false, false, na, width, width, 1.f, Xc, hm, Qb, hm, 0.f, h->Gg, hm));
    launch_scatter_add_rows(st, na, width, h->Gg, hm, h->idx, (float)(2.0 * k_signed), G, ldg);
  }
  MCGRA_KERNEL_CHECK();
  return 0;
}

// noise == NULL: modified_adj == M (monitoring forward :290-293 and eps == 0); otherwise adding_noise (:165)
int forward_common(mcgra_attack* h, hipStream_t st, float* adjn_out, const float* noise,
                          double* adjn_rowsum = nullptr) {
  const int n = h->p.n, ld = h->p.ld;
  const bool general = noise != nullptr || h->has_ori;      // (ori != 0: clamp(M + ori) even without noise, :474-478)
  if (!general && h->carry.prep_valid) {
    // d, r and the norm / sparsity sums from the row sums the Adam pass left behind: no pass over M
    const size_t cnt = (size_t)n * rankk_apply_adam_tiles(n);
    prep_from_partials(st, n, h->G_A, adam_row_sums(h, cnt), h->d, h->r, h->rowsq, h->rowsum);
  } else
  launch_prep(st, general, n, ld, h->M, h->has_ori ? h->ORI : nullptr, noise, h->cfg.eps, h->Abuf, h->gate, h->d, h->r, h->rowsq, h->rowsum);
  launch_reduce_rows(st, h->rowsq, n, 1, h->scal + S_SQ);
  launch_reduce_rows(st, h->rowsum, n, 1, h->scal + S_SUM);
  launch_adjn(st, n, ld, general ? h->Abuf : h->M, h->r, adjn_out, adjn_rowsum);
  MCGRA_KERNEL_CHECK();
  return 0;
}

// ori != 0, places that use get_modified_adj(ori_adj) WITHOUT adding_noise's clamp: the monitoring forward (:290-293) and
// the adj_norm of an attack without steps (:142).  adj_norm((1 - I) o M + ori) -> adjn_out; d, r, S_SUM as forward_common.
static int forward_ori_unclamped(mcgra_attack* h, hipStream_t st, float* adjn_out) {
  const int n = h->p.n, ld = h->p.ld;
  launch_axpby2d(st, n, h->M, ld, 1.f, h->ORI, ld, 1.f, h->Bbuf, ld);
  launch_prep(st, false, n, ld, h->Bbuf, nullptr, nullptr, 0.f, nullptr, nullptr, h->d, h->r, h->rowsq, h->rowsum);
  launch_reduce_rows(st, h->rowsum, n, 1, h->scal + S_SUM);
  launch_adjn(st, n, ld, h->Bbuf, h->r, adjn_out, nullptr);
  MCGRA_KERNEL_CHECK();
  return 0;
}

__global__ void k_cn(const double* __restrict__ scal, float coef, float* __restrict__ out) {
  // d/da (coef * |a|_2) = coef * a / |a|, 0 at the origin (torch.norm backward); |a|^2 = sum_{i!=j} M^2 / 2
  const double sq = scal[S_SQ] * 0.5;
  out[0] = sq > 0.0 ? (float)(coef / sqrt(sq)) : 0.f;
}

// {sequence number, code} of the decode into mapped host memory (the host polls the sequence number).  code: 0 = no
// relu-masked pair; 1 = masked pairs, every embedding row alive: the fused low-rank step stands (with a
// ReLU embedding a masked pair has S_ij == 0 exactly, the forward is unchanged, and what relu'(0) = 0 removes from the decode
// backward lies on coordinates the embedding's own ReLU masks anyway); 2 = a dead embedding row (count[1]): the step is
// redone by the Gram evaluation.
__global__ void k_post_mask(unsigned int* __restrict__ count_u32, const double* __restrict__ count_f64,
                            unsigned int* __restrict__ seq_dev, unsigned int* __restrict__ host_slot) {
  unsigned int masked;
  if (count_u32) {
    masked = count_u32[1] != 0u ? 2u : (count_u32[0] != 0u ? 1u : 0u);
    count_u32[0] = 0u; count_u32[1] = 0u;          // re-armed for the next decode
  } else {
    masked = count_f64[1] != 0.0 ? 2u : (count_f64[0] != 0.0 ? 1u : 0u);      // (row-block rank: sums over the ranks)
  }
  const unsigned int seq = ++*seq_dev;
  __hip_atomic_store(host_slot + 1, masked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();
  __hip_atomic_store(host_slot + 0, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// func(x) = clamp(adj_changes - x, 0, 1).sum() (topology_attack.py:398-399), over the strict lower triangle
static int clamp_sum(mcgra_attack* h, hipStream_t st, float x, bool minmax, double* out, float* mn, float* mx) {
  launch_clamp_rowsum(st, h->p.n, h->p.ld, h->M, x, h->rowsx, minmax ? h->rowmin : nullptr, minmax ? h->rowmax : nullptr);
  launch_reduce_rows(st, h->rowsx, h->p.n, 1, h->scal + S_CLAMPSUM);
  if (minmax) launch_minmax(st, h->p.n, h->rowmin, h->rowmax, h->mm);
  MCGRA_KERNEL_CHECK();
  double s;
  float m2[2] = {0, 0};
  MCGRA_HIP(hipMemcpyAsync(&s, h->scal + S_CLAMPSUM, sizeof(double), hipMemcpyDeviceToHost, st));
  if (minmax) MCGRA_HIP(hipMemcpyAsync(m2, h->mm, 2 * sizeof(float), hipMemcpyDeviceToHost, st));
  MCGRA_HIP(hipStreamSynchronize(st));
  *out = 0.5 * s;   // the symmetric matrix counts every pair twice
  if (minmax) { *mn = m2[0]; *mx = m2[1]; }
  return 0;
}

// PGDAttack.projection + bisection (topology_attack.py:338-347, 397-412).  Host-driven:
// only reachable when num_edges < n(n-1)/2, never with main.py's default density.
int project(mcgra_attack* h, hipStream_t st) {
  const double ne = h->cfg.num_edges;
  double s0; float mn, mx;
  CHK(clamp_sum(h, st, 0.f, true, &s0, &mn, &mx));
  float miu = 0.f;
  if ((float)s0 > ne) {
    float a = mn - 1.f, b = mx;     // left = (adj_changes - 1).min(); right = adj_changes.max()
    double fa_s; float fa;
    CHK(clamp_sum(h, st, a, false, &fa_s, nullptr, nullptr));
    fa = (float)fa_s - (float)ne;
    miu = a;
    while ((b - a) >= 1e-5f) {
      miu = (a + b) / 2.f;
      double fm_s;
      CHK(clamp_sum(h, st, miu, false, &fm_s, nullptr, nullptr));
      const float fm = (float)fm_s - (float)ne;
      if (fm == 0.0f) break;
      if (fm * fa < 0.f) b = miu;
      else { a = miu; fa = fm; }
    }
  }
  launch_shift_clamp(st, h->p.n, h->p.ld, h->M, miu);   // clamp(adj_changes - miu, 0, 1); miu = 0 is the plain clamp
  MCGRA_KERNEL_CHECK();
  return 0;
}

// loss terms of the step just taken, from the device scalar slots (one readback + sync): layout of mcgra_attack_step's
// scalars_out
int collect_scalars(mcgra_attack* h, hipStream_t st, double* scalars_out, bool have_clampsum) {
  const mcgra_attack_config_t& c = h->cfg;
  const int n = h->p.n, ld = h->p.ld, C = h->p.C;
  const int he = h->p.wdt[h->p.Le - 1];
  const double sg = sign_of(h);
  const double w1 = c.w[0], w2 = c.w[1], w6 = c.w[5], w7 = c.w[6], w9 = c.w[8], w10 = c.w[9];
  const double k1 = w1 * 1000 * AP_C1, k2 = w2 * 100 * AP_C2, k6 = w6 * 100 * AP_C6, k7 = w7 * AP_C7;
  const double k9 = w9 * AP_C9, k10 = w10 * AP_C10;
  const double n2 = (double)n * n;
  const bool cka = c.measure == MCGRA_MEASURE_CKA;
  const bool hsic = c.measure == MCGRA_MEASURE_HSIC || cka;
  const bool use1 = (w1 != 0), use2 = (w2 != 0);
    if (!have_clampsum) {
      launch_clamp_rowsum(st, n, ld, h->M, 0.f, h->rowsx, nullptr, nullptr);
      launch_reduce_rows(st, h->rowsx, n, 1, h->scal + S_CLAMPSUM);
    }
    double s[S_COUNT];
    MCGRA_HIP(hipMemcpyAsync(s, h->scal, sizeof(s), hipMemcpyDeviceToHost, st));
    MCGRA_HIP(hipStreamSynchronize(st));
    const double nll = s[S_NLL] / h->p.na;
    const double norm_a = sqrt(0.5 * s[S_SQ]);
    const double origin = nll + norm_a * 0.001;
    double c1v = 0, c2v = 0;
    const bool kl = c.measure == MCGRA_MEASURE_KL || c.measure == MCGRA_MEASURE_KDE, dp = c.measure == MCGRA_MEASURE_DP;      // (KDE: the slot holds the value, as for KL)
    if (cka) {
      double cst[8];
      MCGRA_HIP(hipMemcpy(cst, h->cst, sizeof(cst), hipMemcpyDeviceToHost));
      const double d1 = sqrt(cst[0]) * sqrt(s[S_CK1]), d2 = sqrt(s[S_CK1]) * sqrt(s[S_CK3]);
      c1v = d1 > 0 ? k1 * s[S_CK0] / d1 : 0;
      c2v = d2 > 0 ? k2 * s[S_CK2] / d2 : 0;
    }
    else if (dp) { c1v = k1 * sqrt(s[S_H1]); c2v = k2 * sqrt(s[S_H2]); }
    else if (hsic || kl) { c1v = k1 * s[S_H1]; c2v = k2 * s[S_H2]; }
    else { c1v = k1 * s[S_V1] / n2; c2v = k2 * s[S_V2] / n2; }
    if (!use1) c1v = 0;
    if (!use2) c2v = 0;
    const double c6v = k6 * (-s[S_V6] / n2), c7v = k7 * (-s[S_V7] / n2);
    double c9v = 0, c10v = 0;
    if (w9 != 0) c9v = dp ? k9 * sqrt(s[S_C9]) : (hsic || kl) ? k9 * s[S_C9] : k9 * s[S_C9] / ((double)h->p.na * he);
    if (w10 != 0) c10v = dp ? k10 * sqrt(s[S_C10]) : (hsic || kl) ? k10 * s[S_C10] : k10 * s[S_C10] / ((double)h->p.na * C);
    scalars_out[0] = c.weight_sup * origin + sg * (c1v + c2v + c9v + c10v) + c6v + c7v;
    scalars_out[1] = origin; scalars_out[2] = c1v; scalars_out[3] = c2v; scalars_out[4] = c6v; scalars_out[5] = c7v;
    scalars_out[6] = c9v; scalars_out[7] = c10v; scalars_out[8] = 0.5 * s[S_CLAMPSUM]; scalars_out[9] = nll;
    (void)ld;
  return 0;
}

// ---- the general step: every configuration the fused steps do not cover.  Its stages, in program order on the caller's stream:
//   step_forward   forward and decode; Xc = H adj_norm with the start of Kx (Gram evaluation) or the fork of P1 (low-rank step)
//   *_terms        the N x N loss terms of the measure; HSIC decides between the low-rank forms and the Grams
//   gram_eval      the Grams and their gradient products on the split kernel, on the Gram stream beside the rest of the step
//   gram_fp32      ... or on the fp32 SYRK / SYMM
//   step_backward  small-operand terms, victim chain, decode and modified_adj chain backward
//   step_tail      normalisation backward, Adam, projection, scalars
struct GeneralStep {
  mcgra_attack* h;
  hipStream_t st, gst;             // the caller's stream; the Gram evaluation's (st2 beside the rest of the step: gram_ovl)
  const float *noise, *A, *em;     // A: modified_adj (M itself when ori == 0, eps == 0); em: the embedding the decode reads
  const unsigned char* gate;
  int he;                          // width of em
  double sg, k1, k2, k6, k7, k9, k10, n2;
  bool cka, hsic, use1, use2, use9, use10;
  bool gen;                        // modified_adj = clamp(M + ori + eps noise) with its gate
  bool want_xc;                    // HSIC / CKA with c1 or c2: centred operands and Grams (or their low-rank forms)
  bool gs_path;                    // ... the Grams on the split kernel, unless the low-rank form takes the step
  bool gs_only;                    // ... with no low-rank form at all: the step IS a Gram evaluation
  bool adopt;                      // forward of this iteration already done by the last monitor call
  bool kx_adopt;                   // ... and Kx of its adj_norm forked by it (gram_pack_fork_kx)
  bool p1_deferred;                // P1's fork waits for this step's masked-pair count
  bool ky_early;                   // Ky started in front of the entropy pass
  bool small_side;                 // small-operand terms on the third stream (ev_fork3 recorded behind the forward chains)
  bool gram_eval;                  // known after the loss terms: this step evaluates the Grams on the split kernel
};

// One N x N x N product of the Gram evaluation on the split kernel (2-plane fp16 operands, MCGRA_SPLIT_BF16=1: single-plane), timed
// when profiling, on the Gram stream gst: it picks up behind everything enqueued on the caller's stream st so far, and records
// `done` (if any) behind the product.  Split-K slabs in the small graph's slab when there is one, else in `slab`, an N x N buffer
// idle meanwhile.
// (the (A, B) operand magnitudes of a product are read where they are: split3_symm takes B's through its own pointer.  Rounds
//  2 - 5 paired them up in amax[8 ..] with two 4-byte device-to-device copies per product -- eight launches of ~5 us per step on
//  the caller's queue.  No slot is rewritten between a product's fork and its join: amax[1] / [2] come out of the centring
//  passes of this step, [3] / [4] out of hsic_gram_scales / the CKA combine, all in front of the products that read them.)
static int gram_product(mcgra_attack* h, hipStream_t st, hipStream_t gst, const void* Ap, const void* Bp, float* C, float* slab,
                        const float* amax_a, const float* amax_b, int flags, hipEvent_t done) {
  const int n = h->p.n, ld = h->p.ld;
  if (gst != st) { MCGRA_HIP(hipEventRecord(h->ev_fork, st)); MCGRA_HIP(hipStreamWaitEvent(gst, h->ev_fork, 0)); }
  CHK(timer_begin(h, gst, h->profile));
  MCGRA_HIP(split3_symm(gst, n, Ap, Bp, C, ld, 0, -1, h->small_slab ? h->small_slab : slab,
                        h->small_slab ? h->small_slab_bytes : sizeof(float) * (size_t)n * ld, 2, amax_a, 0, -1,
                        flags | (h->p.split_single ? SPLIT_SINGLE : 0), 0, nullptr, 0, nullptr, amax_b));
  CHK(timer_end(h, gst, h->profile, 2.0 * (double)n * n * n));
  if (gst != st && done) MCGRA_HIP(hipEventRecord(done, gst));
  return 0;
}
// Kx = Xc Xc^T from the planes of Xc's rows in Gp0, forked onto the Gram stream: lower tiles, mirrored by the epilogue (full,
// bitwise symmetric matrix); split-K slabs in G_A, idle until the tail
static int fork_kx(mcgra_attack* h, hipStream_t st) {
  hipStream_t gst = (h->p.gram_ovl && h->st2) ? h->st2 : st;
  return gram_product(h, st, gst, h->Gp0, h->Gp0, h->KX, h->G_A, h->amax + 1, h->amax + 1, SPLIT_TRI, nullptr);
}
// Gram-evaluation configurations without a low-rank form (GAT / GraphSAGE victims, CKA, widths > 32, MCGRA_NO_LOWRANK): both packed
// orientations of Xc = H adj_norm in one pass over `adjn` (rows of Xc: both operands of Kx = Xc Xc^T; rows of Xc^T: the B operand of
// G_adjn += LY Xc), diag(Kx) from the same pass, and Kx on the side stream.  Called by the step -- or, one forward earlier, by the
// monitor call whose adj_norm the step adopts (kx_early): the same launches on the same data, the same bits.  rowsx holds the column
// sums of adjn.
static int gram_pack_fork_kx(mcgra_attack* h, hipStream_t st, const float* adjn) {
  const int n = h->p.n, ld = h->p.ld;
  launch_colmean_f32(st, n, ld, h->rowsx, h->cmean);
  pack_center_both(st, n, ld, adjn, h->cmean, h->r, 0.f, h->Gp0, h->Bpack, h->amax + 1, h->gram_diag, reinterpret_cast<double*>(h->XC));
  return fork_kx(h, st);
}
// Ky = Yc Yc^T behind Kx on the Gram stream (ev_first: Kx done, ev_join: Ky done), from the planes the centring pass of
// modified_adj1 just packed
static int launch_ky(GeneralStep& s) {
  mcgra_attack* h = s.h;
  if (s.gst != s.st) MCGRA_HIP(hipEventRecord(h->ev_first, s.gst));    // Kx done
  if (s.use2) CHK(gram_product(h, s.st, s.gst, h->Gp1, h->Gp1, h->KY, h->G_A, h->amax + 2, h->amax + 2, SPLIT_TRI, h->ev_join));
  return 0;
}

// P1 = (H Kf H) Xc: value and gradient of c1 in the low-rank path; the only N x N x N product of such a step.  Forked onto st2 (it
// needs nothing else of the step), joined in front of its only consumer in the tail.
static int fork_p1(GeneralStep& s) {
  mcgra_attack* h = s.h; const int n = h->p.n, ld = h->p.ld;
  hipStream_t sp = h->p.overlap ? h->st2 : s.st;
  if (h->p.overlap) { MCGRA_HIP(hipEventRecord(h->ev_fork, s.st)); MCGRA_HIP(hipStreamWaitEvent(h->st2, h->ev_fork, 0)); }
  if (h->p.split_on && !s.gen) {
    // planes of Xc^T from the rows of the (symmetric) adj_norm (packed by center_xc), then the plane-reusing kernel
    // (split_symm_bf16.hip); split-K slabs of the ragged last round go to KY, idle on a low-rank step
    CHK(timer_begin(h, sp, h->profile));
    MCGRA_HIP(split3_symm(sp, n, h->Apack, h->Bpack, h->KX, ld, 0, -1, h->small_slab ? h->small_slab : h->KY,
                          h->small_slab ? h->small_slab_bytes : sizeof(float) * (size_t)n * ld, h->p.split_planes, h->amax, 0, -1,
                          h->p.split_single ? SPLIT_SINGLE : 0));
    CHK(timer_end(h, sp, h->profile, 2.0 * (double)n * n * n));
    ++h->split_steps;
  } else
  CHK(eg_symm(h, sp, n, n, h->KFC, ld, h->XC, ld, 0.f, h->KX, ld));
  if (h->p.overlap) MCGRA_HIP(hipEventRecord(h->ev_join, h->st2));
  h->step.p1_inflight = true;
  return 0;
}

// Xc = H adj_norm (and, for the low-rank path, |xc_i|^2 = diag(Kx) from the same pass): the packed operands and the start of Kx
// of a Gram evaluation, or the operands and the fork of P1 of a low-rank step
static int center_xc(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld;
  if (s.gen) {                               // possibly asymmetric: true column sums
    if (!h->colpart_d) CHK(dalloc(h, &h->colpart_d, (size_t)h->nstrips * ld));
    launch_colsum(st, n, ld, h->ADJN, h->colpart_d, h->nstrips, h->rowsx);
  }
  if (s.gs_only) {
    // This step IS a Gram evaluation: the fp32 Xc is never stored, Kx starts now, beside the forward chains and the decode.
    // (kx_adopt: the monitor call of the previous iteration did exactly this on the adj_norm this step adopted)
    if (!s.kx_adopt) CHK(gram_pack_fork_kx(h, st, h->ADJN));
  } else {
    // (gram_diag: |xc_i|^2 = diag(Kx) for the scale bound of the combined Grams -- only when the low-rank path does not want it)
    const bool want_lrrs = lr_ok(h) && !s.cka && s.use2;
    launch_center_cols(st, n, ld, h->ADJN, h->rowsx, h->cmean, h->XC, want_lrrs ? h->lrRs : (s.gs_path ? h->gram_diag : nullptr),
                       ((h->p.split_mode == 2 && h->p.split_planes == 2) || gram_split(h)) ? h->amax + 1 : nullptr);
    // Gram evaluation through the split kernel: planes of Xc^T now (cmean is reused by Yc's centring), unless the
    // low-rank product below packs them anyway
    if (gram_split(h) && !s.gen && !(lr_ok(h) && !s.cka && s.use1 && h->p.split_on))
      split3_pack(st, n, ld, h->ADJN, h->cmean, false, h->Bpack, 2, h->amax + 1);
  }
  if (lr_ok(h) && !s.cka && s.use1) {
    // bf16 planes of Xc^T (opt-in split path) on the caller's stream, ahead of the fork: cmean is reused later
    if (h->p.split_on && !s.gen)
      split3_pack(st, n, ld, h->ADJN, h->cmean, false, h->Bpack, h->p.split_planes, h->amax ? h->amax + 1 : nullptr);
    // (in a run whose decode keeps masking pairs the product would be thrown away: it then waits for this step's own
    // masked-pair count, hsic_terms)
    if (!(h->carry.skip_fused && s.use2)) CHK(fork_p1(s));
    else s.p1_deferred = true;
  }
  return 0;
}

// ---- forward: adjacency, normalisation (:164-166), victim and embedding chains (:167-185), dot_product_decode +
// get_modified_adj_after (:187-188)
static int step_forward(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld, hs = h->p.hsum, L = h->p.L, Le = h->p.Le, C = h->p.C, he = s.he;
  // (S_SQ, S_SUM are the first two slots: written by forward_common, kept when its results are adopted)
  MCGRA_HIP(hipMemsetAsync(h->scal + (s.adopt ? 2 : 0), 0, sizeof(double) * (S_COUNT - (s.adopt ? 2 : 0)), st));
  const float* noise_ld = nullptr;
  if (s.noise) {  // caller layout is [n][n]; the kernels use leading dimension ld.  G_A is free at this point.
    MCGRA_HIP(hipMemcpy2DAsync(h->G_A, (size_t)ld * 4, s.noise, (size_t)n * 4, (size_t)n * 4, n, hipMemcpyDeviceToDevice, st));
    noise_ld = h->G_A;
  }
  // adj_norm is symmetric when eps == 0 (ori == 0): its column means are its row sums / n, which k_adjn emits
  if (s.adopt) { float* t = h->ADJN; h->ADJN = h->ADJN_next; h->ADJN_next = t; }
  else CHK(forward_common(h, st, h->ADJN, noise_ld, (s.want_xc && !s.gen) ? h->rowsx : nullptr));
  h->step.p1_inflight = false;
  if (s.want_xc) CHK(center_xc(s));
  // ---- victim(features, adj_norm) (:167) and the CE loss (:172)
  if (!s.adopt) {
    CHK(chain_forward(h, st, h->ADJN, ld, L, h->Tv, h->Pv, h->Hv, h->Sv));
    CHK(head_forward(h, st, h->Hv, h->Z, h->logp, h->sm));
  }
  launch_nll_grad(st, n, C, h->logp, h->sm, C, h->labels, h->cnt, (float)(h->cfg.weight_sup / h->p.na), h->GZ, h->rowvals + 6 * (size_t)ld);
  launch_reduce_rows(st, h->rowvals + 6 * (size_t)ld, n, 1, h->scal + S_NLL);
  // ---- embedding(features, modified_adj - ori_adj) (:185) == first Le layers of victim(features, modified_adj) (:259)
  CHK(chain_forward(h, st, s.A, ld, L, h->Tu, h->Pu, h->Hu, h->Su));
  CHK(head_forward(h, st, h->Hu, h->Z2, nullptr, h->sm2));
  if (h->has_ori) {      // embedding(features, modified_adj - ori_adj) (:185) no longer shares the chain of output2 (:259)
    launch_axpby2d(st, n, s.A, ld, 1.f, h->ORI, ld, -1.f, h->Bbuf, ld);
    CHK(chain_forward(h, st, h->Bbuf, ld, Le, h->Te, h->Pe, h->He, h->Se));
  }
  if (h->p.small_side_on && h->st3 && h->st3 != st && (s.use9 || s.use10)) {
    MCGRA_HIP(hipEventRecord(h->ev_fork3, st));      // (em and softmax(output2) stand: what the small-operand terms need)
    s.small_side = true;
  }
  // ---- dot_product_decode + get_modified_adj_after (:187-188)
  launch_row_normalize(st, n, he, s.em, hs, h->Zn, h->p.hmax, h->nrm, 2.f);
  CHK(eg(h, st, false, true, n, n, he, 1.f, h->Zn, h->p.hmax, h->Zn, h->p.hmax, 0.f, h->A1, ld));
  // (the count of relu-masked pairs is read by the low-rank decision only: HSIC with c2 on a configuration that has the
  // low-rank forms -- every other step skips the counting)
  const bool count_masked = h->cfg.measure == MCGRA_MEASURE_HSIC && lr_ok(h) && h->cfg.w[1] != 0;
  if (count_masked) MCGRA_HIP(hipMemsetAsync(h->nmask, 0, sizeof(unsigned int), st));
  h->step.nmask_zero = false;
  launch_decode_post(st, n, ld, h->A1, h->has_ori ? h->ORI : nullptr, count_masked ? h->nmask : nullptr);
  h->step.lr_step = false;
  return 0;
}

// ---- N x N loss terms (:212-236), one function per measure family
// the elementwise pass: entropy terms c6, c7 (and MSELoss' c1, c2: kmse1, kmse2); y_side = false leaves modified_adj1's to the
// low-rank decode backward
static void elem_terms(GeneralStep& s, float kmse1, float kmse2, bool y_side = true) {
  mcgra_attack* h = s.h;
  launch_loss_elem(s.st, h->p.n, h->p.ld, h->ADJN, y_side ? h->A1 : nullptr, h->FADJ, kmse1, kmse2, (float)(s.k6 / s.n2),
                   (float)(s.k7 / s.n2), h->G_ADJN, y_side ? h->G_A1 : nullptr, h->rowvals);
  launch_reduce_rows(s.st, h->rowvals, h->p.n, 4, h->scal + S_V1);
}
// dot_product(X, Y) = |Y^T X|_F (:480-481); d/dY = X P^T / |P|, d/dX = Y P / |P| with P = Y^T X
static int dp_terms(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld;
  elem_terms(s, 0.f, 0.f);
  if (s.use1) {   // c1 = k1 dot_product(feature_adj, adj_norm): P = adj_norm^T Fadj
    CHK(eg(h, st, true, false, n, n, n, 1.f, h->ADJN, ld, h->FADJ, ld, 0.f, h->KX, ld));
    launch_rowsumsq(st, n, ld, h->KX, h->rowsx);
    launch_reduce_rows(st, h->rowsx, n, 1, h->scal + S_H1);
    CHK(eg(h, st, false, true, n, n, n, 1.f, h->FADJ, ld, h->KX, ld, 0.f, h->XC, ld));
    launch_axpy_invnorm(st, n, ld, h->XC, h->scal + S_H1, (float)s.k1, h->G_ADJN);
  }
  if (s.use2) {   // c2 = k2 dot_product(adj_norm, A1): P = A1^T adj_norm
    CHK(eg(h, st, true, false, n, n, n, 1.f, h->A1, ld, h->ADJN, ld, 0.f, h->KY, ld));
    launch_rowsumsq(st, n, ld, h->KY, h->rowsy);
    launch_reduce_rows(st, h->rowsy, n, 1, h->scal + S_H2);
    CHK(eg(h, st, false, false, n, n, n, 1.f, h->A1, ld, h->KY, ld, 0.f, h->XC, ld));          // d/dX = Y P
    launch_axpy_invnorm(st, n, ld, h->XC, h->scal + S_H2, (float)s.k2, h->G_ADJN);
    CHK(eg(h, st, false, true, n, n, n, 1.f, h->ADJN, ld, h->KY, ld, 0.f, h->XC, ld));         // d/dY = X P^T
    launch_axpy_invnorm(st, n, ld, h->XC, h->scal + S_H2, (float)s.k2, h->G_A1);
  }
  return 0;
}
// calc = MutualInformation(sigma=0.4, num_bins=N) (:199-201): c1 = k1 calc(feature_adj, adj_norm)[0] (:213-216),
// c2 = k2 calc(adj_norm, modified_adj1)[0] (:222-225).  Entry (i, j) of an operand meets bin j only and bins j >= 7 are
// out of reach of values <= 2 in float32 (kde_kernels.hip): the terms live on the first KDE_NXN_COLS columns.
static int kde_terms(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld;
  elem_terms(s, 0.f, 0.f);      // only the entropy slots are non-zero
  const int kc = n < h->kde_cols ? n : h->kde_cols;      // (set_graph: 8, or as far as feature_adj's values reach)
  if (s.use1) launch_kde_term(st, n, kc, n, h->FADJ, ld, h->ADJN, ld, s.k1, nullptr, 0, false, h->G_ADJN, ld, true, h->scal + S_H1, h->kde);
  if (s.use2) launch_kde_term(st, n, kc, n, h->ADJN, ld, h->A1, ld, s.k2, h->G_ADJN, ld, true, h->G_A1, ld, true, h->scal + S_H2, h->kde);
  return 0;
}
// calc_kl (:483-487) against softmax(feature_adj) (XC, set_graph)
static int kl_terms(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld;
  elem_terms(s, 0.f, 0.f);      // only the entropy slots are non-zero
  if (s.use1 || s.use2) {
    launch_kl_rows(st, n, ld, h->ADJN, h->A1, h->XC, s.use1 ? (float)s.k1 : 0.f, s.use2 ? (float)s.k2 : 0.f, h->G_ADJN,
                   h->G_A1, h->rowvals + 4 * (size_t)ld);
    launch_reduce_rows(st, h->rowvals + 4 * (size_t)ld, n, 2, h->scal + S_H1);
  }
  return 0;
}
// MSELoss: elementwise, values and gradients of c1, c2 and the entropy terms in one pass
static int mse_terms(GeneralStep& s) {
  elem_terms(s, (float)(s.k1 * 2.0 / s.n2), (float)(s.k2 * 2.0 / s.n2));
  return 0;
}

// Yc = H modified_adj1 for the Grams (and, on the split kernel, its planes and diag(Ky))
static void center_yc(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld;
  launch_rowsum(st, n, ld, h->A1, h->rowsy);
  const bool gs = gram_split(h) && !s.gen;
  if (gs && !lr_ok(h)) {
    // rows of Yc (both operands of Ky = Yc Yc^T) and of Yc^T (B operand of G_A1 += LX Yc) in one pass over the symmetric
    // modified_adj1 (entries in [0, 1]), diag(Ky) from the same pass
    launch_colmean_f32(st, n, ld, h->rowsy, h->cmean);
    pack_center_both(st, n, ld, h->A1, h->cmean, nullptr, 1.0002f, h->Gp1, h->Gp2, h->amax + 2, h->gram_diag + ld,
                     reinterpret_cast<double*>(h->YC));
  } else {
    launch_center_cols(st, n, ld, h->A1, h->rowsy, h->cmean, h->YC, gs ? h->gram_diag + ld : nullptr, gs ? h->amax + 2 : nullptr);
    if (gs) {
      split3_pack(st, n, ld, h->A1, h->cmean, false, h->Gp2, 2, h->amax + 2);      // Yc^T (A1 is symmetric)
      split3_pack(st, n, ld, h->YC, nullptr, false, h->Gp1, 2, h->amax + 2);       // Yc: both operands of Ky = Yc Yc^T
    }
  }
}

// linear_HSIC / linear_CKA (utils.py:1085-1096): the entropy terms, the low-rank decision, and the operands of whichever
// evaluation the step takes -- the factors of the low-rank forms, or Yc centred (and packed) for the Grams
static int hsic_terms(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld, he = s.he;
  if (s.want_xc && lr_ok(h) && !s.cka) {
    // Low-rank path for c2 needs every off-diagonal pair active in the decode's relu (relu'(0) = 0 would
    // mask a pair in the backward); that is data dependent, so the count is read back once per step.
    unsigned int masked = 0;
    if (s.use2) {
      MCGRA_HIP(hipMemcpyAsync(&masked, h->nmask, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
      MCGRA_HIP(hipStreamSynchronize(st));
    }
    h->step.lr_step = (masked == 0);
    if (s.use2) h->carry.skip_fused = masked != 0;
    if (h->step.lr_step && s.p1_deferred) CHK(fork_p1(s));
  }
  // on a low-rank step with c2 the modified_adj1 side (c7 value and gradient) is folded into k_lr_decode_bwd
  const bool y_fused = h->step.lr_step && s.use2 && lr_decode_supported(he);
  // A step that IS a Gram evaluation centres and packs modified_adj1 and starts Ky FIRST: the side stream is idle from the end of
  // Kx until this point, and the N x N entropy pass and its reduction (40 us at n = 3312) need none of it
  s.ky_early = s.gs_only && s.use2 && !h->step.lr_step && s.gst != st;
  if (s.ky_early) { center_yc(s); CHK(launch_ky(s)); }
  elem_terms(s, 0.f, 0.f, !y_fused);
  if (!s.want_xc) return 0;
  if (h->step.lr_step) {
    ++h->lr_steps;
    if (s.use2) {
      launch_lr_colstats(st, n, he, h->Zn, h->p.hmax, h->lrStats);
      launch_lr_prep(st, n, he, h->Zn, h->p.hmax, h->lrStats, h->lrL, h->lrV, h->p.lr_ldv, h->lrDelta);
      // T = Xc^T [U | D Z | delta^2]: W, W2 and t3 from one pass over Xc
      CHK(eg(h, st, true, false, n, h->p.lr_ldv, n, 1.f, h->XC, ld, h->lrV, h->p.lr_ldv, 0.f, h->lrT, h->p.lr_ldv));
      h->step.t3_zero = false;
      launch_lr_post(st, n, he, h->lrT, h->p.lr_ldv, h->lrStats, h->lrR, h->lrC, h->rowvals + 7 * (size_t)ld);
    }
    return 0;
  }
  ++h->general_steps;
  if (s.use2 && !s.ky_early) center_yc(s);
  return 0;
}

// The part of the backward that needs the forward only: small-operand terms c9 (:237-258) and c10 (:259-272), and the
// victim(adj_norm) chain's backward down to G_P of every layer.  (A Gram-evaluation step runs it beside its Grams.)
// (the small-operand terms need em and softmax(output2) only and feed the backward of the modified_adj chain, the last part of the
//  step: ~20 launches of a few microseconds each -- a sixth of a Citeseer-sized step's critical path -- that run on the third stream
//  beside the decode, the N x N loss passes and the Grams; their products use their own split-K workspace: small_term)
// The fork EVENT is recorded right behind the forward chains; the launches themselves are enqueued later in program order
// (early_bwd: beside the Grams, or at the top of the backward) -- the host needs ~5 us per launch, and enqueued in front of the
// decode they left the caller's queue empty for that long (213 us idle under the profiler, a third of the gain).
static int small_terms(GeneralStep& s, hipStream_t q) {
  mcgra_attack* h = s.h;
  MCGRA_HIP(hipMemsetAsync(h->Gem, 0, sizeof(float) * (size_t)h->p.n * h->p.hmax, q));
  if (s.use9) CHK(small_term(h, q, s.he, s.em, h->p.hsum, h->HAg, h->HAc, s.sg * s.k9, h->Gem, h->p.hmax, S_C9));
  if (s.use10) {
    MCGRA_HIP(hipMemsetAsync(h->Gsm, 0, sizeof(float) * (size_t)h->p.n * h->p.C, q));
    CHK(small_term(h, q, h->p.C, h->sm2, h->p.C, h->YAg, h->YAc, s.sg * s.k10, h->Gsm, h->p.C, S_C10));
    launch_softmax_bwd(q, h->p.n, h->p.C, h->sm2, h->Gsm, h->p.C, h->GZ2);
  }
  return 0;
}
static int early_bwd(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, L = h->p.L, C = h->p.C, hs = h->p.hsum;
  if (!s.small_side) CHK(small_terms(s, st));
  // ---- backward: victim(adj_norm) chain -> G_adjn
  if (h->cfg.head_act) launch_elu_grad_mul(st, n, C, h->Z, h->GZ);     // through elu(out_att(x)) (gat.py:206)
  launch_rowmat_mask(st, n, C, h->p.wdt[L - 1], h->GZ, C, h->Wlin, h->p.wdt[L - 1], 1, nullptr, 0, 0, nullptr, 0, 0,
                     h->Pv + h->p.off[L - 1], hs, h->cfg.act, nullptr, 0, h->GPv + h->p.off[L - 1], hs);
  CHK(chain_backward(h, st, h->ADJN, h->p.ld, L - 1, h->Pv, h->GPv, -1, nullptr, 0));
  if (s.small_side) {      // (behind the victim chain's launches in program order: the caller's queue is fed first)
    MCGRA_HIP(hipStreamWaitEvent(h->st3, h->ev_fork3, 0));
    CHK(small_terms(s, h->st3));
    MCGRA_HIP(hipEventRecord(h->ev_join3, h->st3));
  }
  return 0;
}

// G_adjn += sum_l G_P_l T_l^T (+ the low-rank 2 s2 (U M1^T - D Z W^T) of a low-rank step, in the same pass)
static int victim_rankk(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld, hs = h->p.hsum, he = s.he;
  const bool lr2 = s.hsic && h->step.lr_step && s.use2;
  if (lr2 && rankk_nt_supported(n, n, hs, 2 * he)) {
    MCGRA_HIP(rankk_nt(st, n, n, hs, 1.f, h->GPv, hs, h->Tv, hs, 2 * he, 2.f * (float)(s.sg * s.k2), h->lrL, 2 * he, h->lrR,
                       2 * he, 1.f, h->G_ADJN, ld));
    return 0;
  }
  if (lr2) CHK(eg(h, st, false, true, n, n, 2 * he, 2.f * (float)(s.sg * s.k2), h->lrL, 2 * he, h->lrR, 2 * he, 1.f, h->G_ADJN, ld));
  return eg(h, st, false, true, n, n, hs, 1.f, h->GPv, hs, h->Tv, hs, 1.f, h->G_ADJN, ld);   // sum_l G_P_l T_l^T
}

// linear_CKA's value sums and the left factors of its gradient products (L1 -> KY, L2 -> KX) from the Grams (lower: in lower
// tile storage); amax_l2 / amax_l1: their magnitudes, for the split kernel's packs
static void cka_factors(GeneralStep& s, bool lower, float* amax_l2 = nullptr, float* amax_l1 = nullptr) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld;
  launch_cka_sums(st, n, ld, h->KX, h->KY, h->KFC, s.use1, s.use2, h->rowvals + 4 * (size_t)ld, lower);
  launch_reduce_rows(st, h->rowvals + 4 * (size_t)ld, n, 4, h->scal + S_CK0);
  launch_cka_coef(st, h->scal + S_CK0, h->cst + 0, s.use1 ? (float)s.k1 : 0.f, s.use2 ? (float)s.k2 : 0.f, h->coef);
  launch_cka_lincomb(st, n, ld, h->KX, h->KY, h->KFC, h->coef, s.use1, s.use2, lower, amax_l2, amax_l1);
}

// ---- Gram evaluation on the split kernel (steps the low-rank forms do not cover): four N x N x N products.  They run on
// the Gram stream (gram_ovl) beside the HBM-bound rest of the step:
//   Kx = Xc Xc^T   beside the forward chains, the decode, the entropy pass and Yc's centring / packs
//   Ky = Yc Yc^T   beside the small-operand terms and the victim chain's backward
//   G_A1 += LX Yc  beside the victim chain's rank-k update of G_adjn
//   G_adjn += LY Xc  beside the decode backward and the modified_adj chain's backward
// Full Kx and Ky from the fp16 planes of Xc and Yc (split_symm_bf16.hip): tiles on or below the diagonal, mirrored by the
// epilogue; split-K slabs in G_A, idle until the tail.  G_A1 += LX Yc needs Kx only (LX = 2 s2 Kxc is packed beside Ky),
// G_adjn += LY Xc (LY = 2 (s1 Kfc + s2 Kyc) is combined and packed beside the third), its slabs in KX (dead: combined and
// packed).  linear_CKA's factors need both Grams: it combines first.
static int gram_eval(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st, gst = s.gst; const int n = h->p.n, ld = h->p.ld;
  const float s1 = (float)(s.sg * s.k1), s2 = (float)(s.sg * s.k2);
  if (!s.gs_only) {      // (a low-rank configuration whose decode found a dead row: Xc was centred, not packed)
    split3_pack(st, n, ld, h->XC, nullptr, false, h->Gp0, 2, h->amax + 1);
    CHK(fork_kx(h, st));
  }
  if (!s.ky_early) CHK(launch_ky(s));      // (hsic_terms started it in front of the entropy pass when it could)
  ++h->gram_split_steps;
  const void* LY = h->Gp1;
  if (!s.cka) {
    // operand scales of LY / LX from the diagonals of the centred Grams (known since the centring passes)
    hsic_gram_scales(st, n, (lr_ok(h) && s.use2) ? h->lrRs : h->gram_diag, h->gram_diag + ld, s.use1 ? s1 : 0.f, s.use2 ? s2 : 0.f,
                     h->amax);
    if (gst != st) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_first, 0));
    if (s.use2) {
      // LX = 2 s2 Kxc into the planes Xc's rows held (Kx is done with them); G_A1 += LX Yc right behind Ky (ev_second: complete)
      split3_pack(st, n, ld, h->KX, nullptr, false, h->Gp0, 2, h->amax + 4, 2.f * s2);
      CHK(gram_product(h, st, gst, h->Gp0, h->Gp2, h->G_A1, h->G_A, h->amax + 4, h->amax + 2, SPLIT_BETA, h->ev_second));
    }
    // beside the Grams: everything of the backward that needs the forward only -- enqueued BEHIND the fork of G_A1 += LX Yc, whose
    // operand pack needs Kx and the diagonals only: the ~20 small-operand launches cost the host ~70 us, and in front of the
    // pack they held the third product back by that long (r06 timeline: 27 us between Ky's reduction and the product)
    CHK(early_bwd(s));
    if (s.use2 && gst != st) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_join, 0));      // the combine reads Ky
    // LY straight into its packed planes (the planes Yc's rows held: Ky is done with them), the two value sums from the same
    // pass (partials in YC, dead once packed) -- beside G_A1 += LX Yc
    hsic_combine_pack(st, n, ld, h->KX, h->KY, h->KFC, s.use1 ? s1 : 0.f, s.use2 ? s2 : 0.f, h->amax, h->Gp1, nullptr,
                      reinterpret_cast<double*>(h->YC), h->rowvals + 4 * (size_t)ld);
    launch_reduce_rows(st, h->rowvals + 4 * (size_t)ld, n, 2, h->scal + S_H1);
  } else {
    CHK(early_bwd(s));
    if (gst != st) MCGRA_HIP(hipStreamWaitEvent(st, s.use2 ? h->ev_join : h->ev_first, 0));
    // linear_CKA (:486): the same two gradient products with left factors L1 -> KY, L2 -> KX
    MCGRA_HIP(hipMemsetAsync(h->amax + 3, 0, 2 * sizeof(float), st));
    cka_factors(s, false, h->amax + 4, h->amax + 3);
    split3_pack(st, n, ld, h->KY, nullptr, false, h->Gp0, 2, h->amax + 3);
    LY = h->Gp0;
    if (s.use2) {
      split3_pack(st, n, ld, h->KX, nullptr, false, h->Gp1, 2, h->amax + 4);
      CHK(gram_product(h, st, gst, h->Gp1, h->Gp2, h->G_A1, h->G_A, h->amax + 4, h->amax + 2, SPLIT_BETA, h->ev_second));
    }
  }
  // G_adjn += LY Xc behind the victim chain's rank-k update of G_adjn
  CHK(victim_rankk(s));
  CHK(gram_product(h, st, gst, LY, h->Bpack, h->G_ADJN, h->KX, h->amax + 3, h->amax + 1, SPLIT_BETA, h->ev_join));
  MCGRA_KERNEL_CHECK();
  return 0;
}

// ---- the same on the fp32 MFMA GEMM: Grams are symmetric, only the 128x128 tiles on or below the diagonal are computed (lower
// tile storage), and the gradient products read the mirrored half transposed (SYMM): 3 n^3 MACs per step instead of 4
static int gram_fp32(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld;
  CHK(eg_syrk(h, st, n, n, h->XC, ld, h->KX, ld, s.use2 ? h->YC : nullptr, s.use2 ? h->KY : nullptr));   // H Kx H (and H Ky H)
  if (s.cka) cka_factors(s, true);
  else {
    const float s1 = (float)(s.sg * s.k1), s2 = (float)(s.sg * s.k2);
    launch_hsic_combine(st, n, ld, h->KX, h->KY, h->KFC, s.use1 ? s1 : 0.f, s.use2 ? s2 : 0.f, h->rowvals + 4 * (size_t)ld, true);
    launch_reduce_rows(st, h->rowvals + 4 * (size_t)ld, n, 2, h->scal + S_H1);
  }
  // G_adjn += 2 (s1 Kfc + s2 Kyc) @ Xc ;  G_A1 += 2 s2 Kxc @ Yc   (K 1 = 0, so Xc may replace X)
  if (s.use2) CHK(eg_symm(h, st, n, n, h->KY, ld, h->XC, ld, 1.f, h->G_ADJN, ld, h->KX, h->YC, h->G_A1));
  else CHK(eg_symm(h, st, n, n, h->KY, ld, h->XC, ld, 1.f, h->G_ADJN, ld));
  MCGRA_KERNEL_CHECK();
  return 0;
}

// ---- backward: the low-rank step's decode factors, the forward-only part (unless the Gram evaluation ran it beside its
// products), the decode, and the modified_adj chain (embedding + output2) down to G_P
static int step_backward(GeneralStep& s) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const int n = h->p.n, ld = h->p.ld, hs = h->p.hsum, L = h->p.L, Le = h->p.Le, C = h->p.C, he = s.he;
  const bool lr2 = s.hsic && h->step.lr_step && s.use2;
  if (lr2) {
    CHK(eg(h, st, false, false, n, 2 * he, n, 1.f, h->XC, ld, h->lrT, h->p.lr_ldv, 0.f, h->lrQ, 2 * he));         // [Q | Q2] = Xc [W | W2]
    if (!lr_decode_supported(he))     // widths without a fused decode backward: d c2 / d A1 += 2 s2 Q Z^T, materialised
      CHK(eg(h, st, false, true, n, n, he, 2.f * (float)(s.sg * s.k2), h->lrQ, 2 * he, h->Zn, h->p.hmax, 1.f, h->G_A1, ld));
    MCGRA_KERNEL_CHECK();
  }
  if (!s.gram_eval) { CHK(early_bwd(s)); CHK(victim_rankk(s)); }      // (a Gram-evaluation step ran both beside its products)
  // the decode backward reads G_A1: behind G_A1 += LX Yc on the Gram stream
  if (s.gram_eval && s.use2 && s.gst != st) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_second, 0));

  // ---- backward: decode (S = Zn Zn^T, A1 = offdiag relu(S))
  if (lr2 && lr_decode_supported(he)) {
    // ((G + G^T) o [S > 0]) Zn for G = ie'(A1) + 2 s2 Q Z^T, without materialising G (c7 value from the same pass)
    const int np = launch_lr_decode_bwd(st, n, ld, he, h->A1, h->Zn, h->p.hmax, h->lrQ, (float)(s.k7 / s.n2), h->ws,
                                        h->rowvals + 6 * (size_t)ld, h->GZn, h->p.hmax, h->lrQtZ);
    if (np > 0) launch_reduce_rows(st, h->rowvals + 6 * (size_t)ld, np, 1, h->scal + S_V7);
  } else {
    launch_sym_mask(st, n, ld, h->G_A1, h->A1, h->has_ori ? h->ORI : nullptr, h->G_A);    // G_A used as scratch for (G + G^T) * [S > 0]
    CHK(eg(h, st, false, false, n, he, n, 1.f, h->G_A, ld, h->Zn, h->p.hmax, 0.f, h->GZn, h->p.hmax));
  }
  if (lr2) {   // the -2 s2 KX D part of d c2 / d A1, applied to Zn directly
    const bool fused = lr_decode_supported(he);
    launch_lr_part2(st, n, he, h->lrQ, h->Zn, h->p.hmax, h->lrDelta, h->lrRs, -2.f * (float)(s.sg * s.k2), h->GZn, h->p.hmax,
                    h->rowvals + 7 * (size_t)ld, h->rowvals + 5 * (size_t)ld, fused ? h->lrStats + 2 * he : nullptr,
                    fused ? h->lrQtZ : nullptr, 2.f * (float)(s.sg * s.k2));
    launch_reduce_rows(st, h->rowvals + 5 * (size_t)ld, n, 1, h->scal + S_H2);
  }
  if (s.small_side) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_join3, 0));      // c9 / c10: Gem, GZ2 and their scalars
  launch_row_normalize_bwd(st, n, he, h->GZn, h->Zn, h->p.hmax, h->nrm, h->Gem, h->p.hmax);

  // ---- backward: modified_adj chain (embedding + output2) -> G_A
  if (h->has_ori) {
    // two chains: output2 on modified_adj (only c10 reaches it) and the embedding on modified_adj - ori (em)
    MCGRA_HIP(hipMemsetAsync(h->GPu, 0, sizeof(float) * (size_t)n * hs, st));
    MCGRA_HIP(hipMemsetAsync(h->GPe, 0, sizeof(float) * (size_t)n * hs, st));
    if (s.use10) {
      if (h->cfg.head_act) launch_elu_grad_mul(st, n, C, h->Z2, h->GZ2);
      launch_rowmat_mask(st, n, C, h->p.wdt[L - 1], h->GZ2, C, h->Wlin, h->p.wdt[L - 1], 1, nullptr, 0, 0, nullptr, 0, 0,
                         h->Pu + h->p.off[L - 1], hs, h->cfg.act, nullptr, 0, h->GPu + h->p.off[L - 1], hs);
      CHK(chain_backward(h, st, s.A, ld, L - 1, h->Pu, h->GPu, -1, nullptr, 0));
    }
    launch_rowmat_mask(st, n, 0, he, h->Gem, h->p.hmax, h->Wlin, 0, 0, nullptr, 0, 0, nullptr, 0, 0,
                       h->Pe + h->p.off[Le - 1], hs, h->cfg.act, h->Gem, h->p.hmax, h->GPe + h->p.off[Le - 1], hs);
    CHK(chain_backward(h, st, h->Bbuf, ld, Le - 1, h->Pe, h->GPe, -1, nullptr, 0));
    return 0;
  }
  int ltop;
  if (s.use10) {
    ltop = L - 1;
    if (h->cfg.head_act) launch_elu_grad_mul(st, n, C, h->Z2, h->GZ2);
    launch_rowmat_mask(st, n, C, h->p.wdt[L - 1], h->GZ2, C, h->Wlin, h->p.wdt[L - 1], 1, nullptr, 0, 0, nullptr, 0, 0,
                       h->Pu + h->p.off[L - 1], hs, h->cfg.act, (L - 1 == Le - 1) ? h->Gem : nullptr, h->p.hmax,
                       h->GPu + h->p.off[L - 1], hs);
  } else {
    ltop = Le - 1;
    if (L > Le) MCGRA_HIP(hipMemsetAsync(h->GPu, 0, sizeof(float) * (size_t)n * hs, st));
    launch_rowmat_mask(st, n, 0, he, h->Gem, h->p.hmax, h->Wlin, 0, 0, nullptr, 0, 0, nullptr, 0, 0,
                       h->Pu + h->p.off[Le - 1], hs, h->cfg.act, h->Gem, h->p.hmax, h->GPu + h->p.off[Le - 1], hs);
  }
  CHK(chain_backward(h, st, s.A, ld, ltop, h->Pu, h->GPu, Le - 1, h->Gem, h->p.hmax));
  return 0;
}

// ---- tail: the low-rank step's last contribution to G_adjn, normalisation backward, packed-gradient mirror + Adam + projection
// + clamp (:274-283), scalars
static int step_tail(GeneralStep& s, double* scalars_out) {
  mcgra_attack* h = s.h; hipStream_t st = s.st; const mcgra_attack_config_t& c = h->cfg;
  const int n = h->p.n, ld = h->p.ld, hs = h->p.hsum;
  // the normalisation backward reads G_adjn: behind G_adjn += LY Xc on the Gram stream
  if (s.gram_eval && s.gst != st) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
  bool normbwd_parts = false;
  float* nb_colpart = h->colpart;       // column partials of the normalisation backward: [nb_strips][n]
  int nb_strips = h->nstrips;
  if (s.hsic && h->step.lr_step && (s.use1 || s.use2)) {
    // Last contribution to G_adjn, and the only consumer of P1: everything above ran beside the forked product.
    // G_adjn += 2 s1 P1 + 2 s2 (D^2 Xc + 1 c^T);  v1 = sum P1 o Xc
    if (h->step.p1_inflight) {
      if (h->p.overlap) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
      h->step.p1_inflight = false;
    }
    // ... fused with the two N x N reductions of the normalisation backward that follows (one pass instead of three);
    // its partial sums live in KY, idle on a low-rank step (the product that used it as split-K slab has been joined)
    if (lr_elem_normbwd_scratch_floats(n) <= (size_t)n * ld) {
      double* v1part = nullptr;
      int v1count = 0;
      launch_lr_elem_normbwd(st, n, ld, h->XC, s.use1 ? h->KX : nullptr, s.use2 ? h->lrDelta : nullptr, s.use2 ? h->lrC : nullptr,
                             2.f * (float)(s.sg * s.k1), 2.f * (float)(s.sg * s.k2), h->G_ADJN, s.A, h->r, h->KY, h->rowpart,
                             &nb_colpart, &nb_strips, &v1part, &v1count);
      launch_reduce_rows(st, v1part, v1count, 1, h->scal + S_H1);
      normbwd_parts = true;
    } else {
      launch_lr_elem(st, n, ld, h->XC, s.use1 ? h->KX : nullptr, s.use2 ? h->lrDelta : nullptr, s.use2 ? h->lrC : nullptr,
                     2.f * (float)(s.sg * s.k1), 2.f * (float)(s.sg * s.k2), h->G_ADJN, h->rowvals + 4 * (size_t)ld);
      launch_reduce_rows(st, h->rowvals + 4 * (size_t)ld, n, 1, h->scal + S_H1);
    }
  }
  // Adam's scalars first: the fused tail below consumes them
  h->t += 1;
  hipLaunchKernelGGL(k_cn, dim3(1), dim3(1), 0, st, h->scal, (float)(c.weight_sup * 0.001), h->mm + 2);
  bool adam_done = false;
  // normalisation backward writes G_A (beta = 0), then the chain's outer products accumulate
  if (h->p.fuse_tail && rankk_apply_adam_supported(n, ld, hs) && !h->has_ori) {
    // one pass over the lower tile pairs: apply step + rank-k update + gradient mirror + Adam, no G_A in between
    launch_normbwd(st, n, ld, h->G_ADJN, s.A, h->r, h->d, h->rowpart, nb_colpart, nb_strips, h->gd, nullptr, normbwd_parts);
    // (its row sums of the new M go to G_A, which this path leaves unused; not with a projection still to come)
    const size_t cnt = (size_t)n * rankk_apply_adam_tiles(n);
    const bool emit = !s.gen && adam_emits_partials(h, cnt);
    MCGRA_HIP(rankk_apply_adam(st, n, ld, hs, h->GPu, hs, h->Tu, hs, h->G_ADJN, h->r, h->gd, s.gate, adam_update(h, h->t, emit ? cnt : 0)));
    h->carry.prep_valid = emit;
    adam_done = true;
  } else if (rankk_nt_supported(n, n, hs, 0) && !h->has_ori) {
    // one pass: G_A = GPu Tu^T + (G_adjn_ij r_i r_j + gd_i), the apply step of the normalisation backward as the
    // epilogue of the rank-k update
    launch_normbwd(st, n, ld, h->G_ADJN, s.A, h->r, h->d, h->rowpart, nb_colpart, nb_strips, h->gd, nullptr, normbwd_parts);
    MCGRA_HIP(rankk_nt(st, n, n, hs, 1.f, h->GPu, hs, h->Tu, hs, 0, 0.f, nullptr, 0, nullptr, 0, 0.f, h->G_A, ld, h->G_ADJN, ld,
                       h->r, h->gd));
  } else {
    launch_normbwd(st, n, ld, h->G_ADJN, s.A, h->r, h->d, h->rowpart, nb_colpart, nb_strips, h->gd, h->G_A, normbwd_parts);
    CHK(eg(h, st, false, true, n, n, hs, 1.f, h->GPu, hs, h->Tu, hs, 1.f, h->G_A, ld));
    if (h->has_ori) CHK(eg(h, st, false, true, n, n, hs, 1.f, h->GPe, hs, h->Te, hs, 1.f, h->G_A, ld));   // d / d (modified_adj - ori)
  }

  // ---- packed-gradient mirror + Adam + projection + clamp (:274-283)
  if (!adam_done) {
    h->carry.prep_valid = false;
    launch_adam_sym(st, n, ld, h->G_A, s.gate, adam_update(h, h->t));
  }
  MCGRA_KERNEL_CHECK();
  h->have_step = true;
  if (may_project(h)) { CHK(project(h, st)); h->carry.prep_valid = false; }

  if (scalars_out) CHK(collect_scalars(h, st, scalars_out));
  return 0;
}

int step_general(mcgra_attack_t* h, void* stream, const float* noise, double* scalars_out) {
  if (!h) { set_error("null handle"); return MCGRA_EINVAL; }
  if (!h->graph_set) { set_error("mcgra_attack_set_graph must be called first"); return MCGRA_EINVAL; }
  if ((h->cfg.eps != 0.f) != (noise != nullptr)) {
    set_error("noise must be given exactly when eps != 0 (it stands for torch.randn_like at topology_attack.py:475)");
    return MCGRA_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  if (h->p.sharded && !h->fs_active) {
    set_error("this engine is a row-block rank: drive it with mcgra_attack_shard_begin / mcgra_attack_shard_next");
    return MCGRA_EINVAL;
  }
  // Rule: the fused step goes first and takes what it adopts (fs_begin, fs_pack_fork); the general step takes Kx and drops the rest, below.
  // (after a step whose decode masked a pair the general path goes first: it reads the masked-pair count itself, and
  // only once that is zero again is the fused step worth enqueueing -- a masked run otherwise pays for both every step)
  if (!noise && !h->p.sharded && fused_step_possible(h) && !h->carry.skip_fused) {
    const int rc = fused_step(h, st, scalars_out);      // 1: a relu-masked pair in the decode, the general path redoes the step
    if (rc <= 0) return rc;
  }
  // Rule: take, then drop.  Kx of this step's adj_norm, forked by the monitor call whose forward the step adopts, is taken over;
  // anything else in flight is dropped (the general step packs its own operands), and so is a forward the fused step would have adopted.
  const bool kx_adopt = h->carry.kx_early && h->carry.fwd_cached && !noise && !h->has_ori;
  if (kx_adopt) h->carry.kx_early = false;
  CHK(carry_drop(h, st));
  h->carry.fused_last = h->carry.fused_fwd_valid = false;

  const mcgra_attack_config_t& c = h->cfg;
  GeneralStep s{};
  s.h = h; s.st = st; s.noise = noise; s.he = h->p.wdt[h->p.Le - 1]; s.sg = sign_of(h); s.n2 = (double)h->p.n * h->p.n;
  const double w1 = c.w[0], w2 = c.w[1], w6 = c.w[5], w7 = c.w[6], w9 = c.w[8], w10 = c.w[9];
  s.k1 = w1 * 1000 * AP_C1; s.k2 = w2 * 100 * AP_C2; s.k6 = w6 * 100 * AP_C6; s.k7 = w7 * AP_C7; s.k9 = w9 * AP_C9; s.k10 = w10 * AP_C10;
  s.use1 = w1 != 0; s.use2 = w2 != 0; s.use9 = w9 != 0; s.use10 = w10 != 0;
  s.cka = c.measure == MCGRA_MEASURE_CKA;
  s.hsic = c.measure == MCGRA_MEASURE_HSIC || s.cka;      // both run the centred-Gram path
  s.gen = noise != nullptr || h->has_ori;
  s.A = s.gen ? h->Abuf : h->M; s.gate = s.gen ? h->gate : nullptr; s.em = (h->has_ori ? h->He : h->Hu) + h->p.off[h->p.Le - 1];
  s.want_xc = s.hsic && (s.use1 || s.use2);
  s.gs_path = gram_split(h) && !s.gen && s.want_xc;
  s.gs_only = s.gs_path && !lr_ok(h);
  s.gst = (s.gs_path && h->p.gram_ovl && h->st2) ? h->st2 : st;
  s.adopt = h->carry.fwd_cached && !s.gen; s.kx_adopt = kx_adopt;      // (kx_adopt implies adopt)
  h->carry.fwd_cached = false;

  CHK(step_forward(s));
  const int m = c.measure;
  CHK(m == MCGRA_MEASURE_DP ? dp_terms(s) : m == MCGRA_MEASURE_KDE ? kde_terms(s) : m == MCGRA_MEASURE_KL ? kl_terms(s)
      : s.hsic ? hsic_terms(s) : mse_terms(s));
  MCGRA_KERNEL_CHECK();
  s.gram_eval = s.gs_path && !h->step.lr_step;
  if (s.want_xc) {
    // Join the forked P1 product before the Grams may overwrite KX; a low-rank step joins it as late as possible, in front of
    // its only consumer (step_tail)
    if (h->step.p1_inflight && !h->step.lr_step) {
      if (h->p.overlap) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
      h->step.p1_inflight = false;
    }
    if (s.gram_eval) CHK(gram_eval(s));
    else if (!h->step.lr_step) CHK(gram_fp32(s));
  }
  CHK(step_backward(s));
  return step_tail(s, scalars_out);
}

int mcgra_attack_step(mcgra_attack_t* h, void* stream, const float* noise, double* scalars_out) {
  return step_general(h, stream, noise, scalars_out);
}

long long mcgra_attack_masked_fused_steps(mcgra_attack_t* h) { return h ? (long long)h->masked_fused_steps : 0; }
long long mcgra_attack_cut_product_steps(mcgra_attack_t* h) { return h ? (long long)h->cut_product_steps : 0; }
int mcgra_attack_product_mode(mcgra_attack_t* h) {
  if (!h) return 0;
  return plan_product_mode(h->p.split_single, gram_split(h), h->p.split_mode, h->p.split_planes);
}

int mcgra_attack_path_stats(mcgra_attack_t* h, long long* lowrank_steps, long long* general_steps) {
  if (!h) { set_error("null handle"); return MCGRA_EINVAL; }
  if (lowrank_steps) *lowrank_steps = h->lr_steps;
  if (general_steps) *general_steps = h->general_steps;
  return 0;
}

long long mcgra_attack_fused_steps(mcgra_attack_t* h) { return h ? (long long)h->fused_steps : 0; }
long long mcgra_attack_gram_split_steps(mcgra_attack_t* h) { return h ? (long long)h->gram_split_steps : 0; }

int mcgra_attack_monitor(mcgra_attack_t* h, void* stream, float* out_logp, double* sparsity) {
  if (!h || !h->graph_set) { set_error("engine not set up"); return MCGRA_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  if (h->p.sharded) { set_error("row-block rank: use mcgra_attack_shard_begin(MCGRA_SHARD_MONITOR)"); return MCGRA_EINVAL; }
  // Rule: none.  A monitor call adds to what is in flight; forking an item again replaces it (the pack on its own side stream:
  // fw_prep; Kx behind a drop, below).  It leaves ONE forward: the fused one or the general one.
  if (fused_step_possible(h) && h->carry.fused_last && h->cfg.eps == 0.f) {
    // the monitoring forward IS the next iteration's forward (eps == 0): both chains from M, adopted by fused_step
    CHK(fused_forward(h, st));
    h->carry.fused_fwd_valid = true;
    h->carry.fwd_cached = false;
    if (out_logp)
      MCGRA_HIP(hipMemcpyAsync(out_logp, h->logp, sizeof(float) * (size_t)h->p.n * h->p.C, hipMemcpyDeviceToDevice, st));
    if (sparsity) {
      double s;
      if (h->carry.early_pack) MCGRA_HIP(hipStreamWaitEvent(st, h->ev_pack, 0));      // (the sum rides on the pack's stream)
      MCGRA_HIP(hipMemcpyAsync(&s, h->scal + S_SUM, sizeof(double), hipMemcpyDeviceToHost, st));
      MCGRA_HIP(hipStreamSynchronize(st));
      *sparsity = s / ((double)h->p.n * h->p.n);
    }
    return 0;
  }
  h->carry.fused_fwd_valid = false;
  // adj_norm2 must not overwrite ADJN, which has to survive for the post-loop decode (:300): it goes to ADJN_next
  // (adopted by the next step, see fwd_cached) or, without reuse, to the A1 buffer.
  const bool want_xc = (h->cfg.measure == MCGRA_MEASURE_HSIC || h->cfg.measure == MCGRA_MEASURE_CKA) &&
                       (h->cfg.w[0] != 0 || h->cfg.w[1] != 0);
  float* dst = fwd_reuse(h) ? h->ADJN_next : h->A1;
  if (h->has_ori) CHK(forward_ori_unclamped(h, st, dst));
  else
  CHK(forward_common(h, st, dst, nullptr, (fwd_reuse(h) && want_xc) ? h->rowsx : nullptr));
  if (h->p.kx_early_on && want_xc && gram_split(h) && !lr_ok(h) && !h->has_ori && h->cfg.eps == 0.f && h->have_step) {
    // the next step of this configuration is a Gram evaluation whose first product needs this adj_norm only: packed and forked now,
    // it runs beside the chains below and beside the next step's own forward part instead of behind them (the row partials in G_A
    // that forward_common just consumed make room for the product's split-K slabs)
    CHK(carry_drop(h, st));      // (two monitor calls in a row: the first one's Kx)
    CHK(gram_pack_fork_kx(h, st, dst));
    if (h->p.gram_ovl && h->st2) MCGRA_HIP(hipEventRecord(h->ev_first, h->st2));
    h->carry.kx_early = true;
    if (!h->small_slab) h->carry.prep_valid = false;      // (the product's split-K slabs went into G_A, over the row partials forward_common just consumed)
  }
  CHK(chain_forward(h, st, dst, h->p.ld, h->p.L, h->Tv, h->Pv, h->Hv, h->Sv));
  CHK(head_forward(h, st, h->Hv, h->Z, h->logp, fwd_reuse(h) ? h->sm : nullptr));
  h->carry.fwd_cached = fwd_reuse(h);
  if (out_logp)
    MCGRA_HIP(hipMemcpyAsync(out_logp, h->logp, sizeof(float) * (size_t)h->p.n * h->p.C, hipMemcpyDeviceToDevice, st));
  if (sparsity) {
    double s;
    MCGRA_HIP(hipMemcpyAsync(&s, h->scal + S_SUM, sizeof(double), hipMemcpyDeviceToHost, st));
    MCGRA_HIP(hipStreamSynchronize(st));
    *sparsity = s / ((double)h->p.n * h->p.n);
  }
  return 0;
}

// out += dot_product_decode2(Z) (topology_attack.py:421-467); Z is [n x w] with leading dim ldz
static int dd2(mcgra_attack* h, hipStream_t st, int mode, const float* Z, int w, int ldz, float* out) {
  const int n = h->p.n, ld = h->p.ld;
  const float* src = Z;
  int lsrc = ldz;
  if (mode == 1 || mode >= 4) {
    const float p = mode == 5 ? 3.f : (mode == 6 ? 5.f : 2.f);
    launch_row_normalize(st, n, w, Z, ldz, h->GZn, h->p.hmax, nullptr, p);
    src = h->GZn; lsrc = h->p.hmax;
  }
  CHK(eg(h, st, false, true, n, n, w, 1.f, src, lsrc, src, lsrc, 0.f, h->KX, ld));
  const int emode = (mode == 0 || mode == 1) ? 0 : (mode == 3 ? 3 : 2);
  launch_dd2_accum(st, n, ld, h->KX, emode, h->rowpart, out, n);
  MCGRA_KERNEL_CHECK();
  return 0;
}

// The post-loop ensemble (:300-324), behind both entries.  comps == NULL (mcgra_attack_finalize): every summand is added to out
// as it is made.  comps != NULL (mcgra_attack_finalize_components): summand k goes to its own matrix comps + k n n -- a matrix is
// copied, a decode accumulates into a zeroed one, so that it is the bits the first form adds -- and then, when out_mask holds it,
// into out by the same add.  The arguments were checked.
static int finalize_run(mcgra_attack* h, hipStream_t st, int decode_mode, const float* H_A, const float* Y_A,
                        const float* label_adj, unsigned out_mask, float* out, float* comps) {
  const int n = h->p.n, ld = h->p.ld, hs = h->p.hsum, Le = h->p.Le, L = h->p.L;
  // Rule: drop + forget.  What a monitor call forked for a step that never came reads M, which is overwritten below (:301), and writes
  // scratch; the forward it left and the row sums the Adam pass left describe the old M.  (skip_fused is kept: a step may follow.)
  CHK(carry_drop(h, st));
  carry_forget(h, true);
  if (!h->have_step) {               // epochs == 0: adj_norm of :142
    if (h->has_ori) CHK(forward_ori_unclamped(h, st, h->ADJN));
    else CHK(forward_common(h, st, h->ADJN, nullptr));
  }
  // em = embedding(features, adj_norm) ; adj_changes <- dot_product_decode(em) (:300-301)
  if (h->carry.fused_last && h->have_step) {
    // the fused step never stores adj_norm; embedding(features, adj_norm) of the last iteration is its victim-chain
    // activation of layer emb_nlayer (shared weights), saved by fused_step
    launch_row_normalize(st, n, h->p.wdt[Le - 1], h->em_last, h->p.hmax, h->Zn, h->p.hmax, h->nrm, 2.f);
  } else {
    CHK(chain_forward(h, st, h->ADJN, ld, Le, h->Tu, h->Pu, h->Hu, h->Su));
    launch_row_normalize(st, n, h->p.wdt[Le - 1], h->Hu + h->p.off[Le - 1], hs, h->Zn, h->p.hmax, h->nrm, 2.f);
  }
  CHK(eg(h, st, false, true, n, n, h->p.wdt[Le - 1], 1.f, h->Zn, h->p.hmax, h->Zn, h->p.hmax, 0.f, h->M, ld));
  launch_decode_post(st, n, ld, h->M, nullptr);            // adj_changes <- the decode (:301); M stays the state
  h->m_is_full = true;                                     // (every rank of a row-block attack now holds the same, whole M)
  const float* mod = h->M;                                 // modified_adj = get_modified_adj(ori_adj) (:302)
  if (h->has_ori) {
    launch_axpby2d(st, n, h->M, ld, 1.f, h->ORI, ld, 1.f, h->Bbuf, ld);
    mod = h->Bbuf;
  }
  const size_t nn = (size_t)n * n;
  bool started = false;                                    // out holds a summand
  // out = X, then out = out + X: s = c_first; s = s + c_next; ...
  auto add = [&](const float* X, int ldx) {
    if (started) launch_axpby2d(st, n, out, n, 1.f, X, ldx, 1.f, out, n);
    else launch_axpby2d(st, n, X, ldx, 1.f, nullptr, 0, 1.f, out, n);
    started = true;
  };
  // summand k, an n x n matrix X
  auto matrix = [&](int k, const float* X, int ldx) {
    if (!comps) { add(X, ldx); return; }
    launch_axpby2d(st, n, X, ldx, 1.f, nullptr, 0, 1.f, comps + k * nn, n);
    if (out && (out_mask >> k & 1u)) add(comps + k * nn, n);
  };
  // summand k, dot_product_decode2 of Z
  auto decode = [&](int k, const float* Z, int w, int ldz) -> int {
    if (!comps) return dd2(h, st, decode_mode, Z, w, ldz, out);      // (learned and feature came first: out is started)
    MCGRA_HIP(hipMemsetAsync(comps + k * nn, 0, sizeof(float) * nn, st));
    CHK(dd2(h, st, decode_mode, Z, w, ldz, comps + k * nn));
    if (out && (out_mask >> k & 1u)) add(comps + k * nn, n);
    return 0;
  };
  // out = modified_adj + feature_adj (:314)
  matrix(0, mod, ld);
  matrix(1, h->FADJ, ld);
  // H_A1, H_A2 = embedding(features, modified_adj) with 1 / 2 layers; Y_A2 = victim (:304-308)
  CHK(chain_forward(h, st, mod, ld, L, h->Tu, h->Pu, h->Hu, h->Su));
  CHK(head_forward(h, st, h->Hu, h->Z2, h->logp, nullptr));
  CHK(decode(2, h->Hu + h->p.off[h->p.fin0 - 1], h->p.wdt[h->p.fin0 - 1], hs));   // H_A1 (:304-305)
  CHK(decode(3, h->Hu + h->p.off[h->p.fin1 - 1], h->p.wdt[h->p.fin1 - 1], hs));   // H_A2 (:306-307)
  CHK(decode(4, h->logp, h->p.C, h->p.C));
  if (H_A) CHK(decode(5, H_A, h->p.wdt[Le - 1], h->p.wdt[Le - 1]));   // (:315-316)
  if (Y_A) CHK(decode(6, Y_A, h->p.C, h->p.C));                        // (:317-318)
  if (label_adj) matrix(7, label_adj, n);                             // (:319-320)
  MCGRA_KERNEL_CHECK();
  return 0;
}

int mcgra_attack_finalize(mcgra_attack_t* h, void* stream, int decode_mode, const float* H_A, const float* Y_A,
                          const float* label_adj, float* out) {
  if (!h || !out || !h->graph_set) { set_error("engine not set up / null out"); return MCGRA_EINVAL; }
  if (decode_mode < 0 || decode_mode > 6) { set_error("decode_mode %d", decode_mode); return MCGRA_EINVAL; }
  return finalize_run(h, (hipStream_t)stream, decode_mode, H_A, Y_A, label_adj, 0u, out, nullptr);
}

int mcgra_attack_finalize_components(mcgra_attack_t* h, void* stream, int decode_mode, const float* H_A, const float* Y_A,
                                     const float* label_adj, unsigned out_mask, float* out, float* comps, unsigned* present) {
  if (!h || !h->graph_set) { set_error("engine not set up"); return MCGRA_EINVAL; }
  if (decode_mode < 0 || decode_mode > 6) { set_error("decode_mode %d", decode_mode); return MCGRA_EINVAL; }
  const unsigned have = 0x1fu | (H_A ? 1u << 5 : 0u) | (Y_A ? 1u << 6 : 0u) | (label_adj ? 1u << 7 : 0u);
  if (!comps) { set_error("finalize_components: null comps"); return MCGRA_EINVAL; }
  if (out_mask & ~have) {
    set_error("finalize_components: out_mask 0x%x names a component that is not given (present 0x%x)", out_mask, have);
    return MCGRA_EINVAL;
  }
  if (out && !out_mask) { set_error("finalize_components: out_mask 0 with an out to write"); return MCGRA_EINVAL; }
  CHK(finalize_run(h, (hipStream_t)stream, decode_mode, H_A, Y_A, label_adj, out_mask, out, comps));
  if (present) *present = have;
  return 0;
}

int mcgra_attack_buffer(mcgra_attack_t* h, const char* name, float** ptr, int* rows, int* cols, int* ldp) {
  if (!h || !name || !ptr) { set_error("null argument"); return MCGRA_EINVAL; }
  const int n = h->p.n, ld = h->p.ld;
  struct E { const char* nm; float* p; int r, c, l; };
  const int le = h->p.Le - 1;
  const E tab[] = {
      {"M", h->M, n, n, ld}, {"adj_norm", h->ADJN, n, n, ld}, {"A1", h->A1, n, n, ld},
      {"G_adjn", h->G_ADJN, n, n, ld}, {"G_A1", h->G_A1, n, n, ld}, {"G_A", h->G_A, n, n, ld},
      {"G_sym", h->GSYM, n, n, ld}, {"adam_m", h->am, n, n, ld}, {"adam_v", h->av, n, n, ld},
      {"d", h->d, 1, n, ld}, {"r", h->r, 1, n, ld}, {"logp", h->logp, n, h->p.C, h->p.C}, {"sm2", h->sm2, n, h->p.C, h->p.C},
      {"em", (h->has_ori ? h->He : h->Hu) + h->p.off[le], n, h->p.wdt[le], h->p.hsum}, {"G_em", h->Gem, n, h->p.wdt[le], h->p.hmax},
      {"HA", h->HA, n, h->p.wdt[le], h->p.hmax}, {"YA", h->YA, n, h->p.C, h->p.C}, {"T0", h->Tv, n, h->p.wdt[0], h->p.hsum},
      {"KFC", h->KFC, n, n, ld},
      {"GPu", h->GPu, n, h->p.hsum, h->p.hsum}, {"GPv", h->GPv, n, h->p.hsum, h->p.hsum}, {"GZn", h->GZn, n, h->p.wdt[le], h->p.hmax},
      {"Zn", h->Zn, n, h->p.wdt[le], h->p.hmax}, {"gd", h->gd, 1, n, ld},
  };
  for (const E& e : tab)
    if (strcmp(e.nm, name) == 0) {
      if (!e.p) {
        set_error("buffer '%s' is not kept by this engine (G_sym needs MCGRA_KEEP_GSYM=1 at create)", name);
        return MCGRA_EINVAL;
      }
      *ptr = e.p;
      if (rows) *rows = e.r;
      if (cols) *cols = e.c;
      if (ldp) *ldp = e.l;
      return 0;
    }
  set_error("unknown buffer '%s'", name);
  return MCGRA_EINVAL;
}

int mcgra_attack_copy_buffer(mcgra_attack_t* h, void* stream, const char* name, float* dst, int dst_ld) {
  float* p = nullptr;
  int r = 0, c = 0, l = 0;
  CHK(mcgra_attack_buffer(h, name, &p, &r, &c, &l));
  if (!dst || dst_ld < c) { set_error("bad destination"); return MCGRA_EINVAL; }
  CHK(carry_wait(h, (hipStream_t)stream));      // Rule: wait.  Scratch buffers under a forked pack, product or Kx.
  MCGRA_HIP(hipMemcpy2DAsync(dst, (size_t)dst_ld * 4, p, (size_t)l * 4, (size_t)c * 4, r, hipMemcpyDeviceToDevice,
                             (hipStream_t)stream));
  return 0;
}

int mcgra_attack_profile(mcgra_attack_t* h, int enable) {
  if (!h) return MCGRA_EINVAL;
  h->profile = enable != 0;
  return 0;
}

int mcgra_attack_gemm_stats(mcgra_attack_t* h, int reset, int64_t* launches, double* ms, double* flops) {
  if (!h) return MCGRA_EINVAL;
  GemmTimer& T = h->timer;
  double tot = 0;
  if (T.used) {
    MCGRA_HIP(hipEventSynchronize(T.ev[T.used - 1]));
    for (size_t i = 0; i + 1 < T.used; i += 2) {
      float e = 0.f;
      MCGRA_HIP(hipEventElapsedTime(&e, T.ev[i], T.ev[i + 1]));
      tot += e;
    }
  }
  if (launches) *launches = T.launches;
  if (ms) *ms = tot;
  if (flops) *flops = T.flops;
  if (reset) { T.used = 0; T.launches = 0; T.flops = 0; }
  return 0;
}

}  // extern "C"
