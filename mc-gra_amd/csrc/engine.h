// The attack engine's state (one mcgra_attack_t) and the helpers its step implementations share.  The handle is the constant plan
// of create (attack_plan.h) and the configuration it was made from, one bit of per-graph state (has_ori), what a call leaves for
// the next (Carry) and a step's scratch flags (StepScratch), buffers, streams and events, and counters.
// attack.hip: create / set_* / the general step (every measure, eps != 0, Gram evaluation of linear_HSIC);
// attack_fused.hip: the low-rank HSIC step evaluated from the learnable adjacency M directly.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/mcgra.h"
#include "attack_plan.h"
#include "common.h"
#include "kernels.h"

// utils.Align_Parameter_Cora (utils.py:1100-1111)
static const double AP_C1 = 100, AP_C2 = 1000, AP_C6 = 10, AP_C7 = 10, AP_C9 = 1, AP_C10 = 1;

enum Scal {  // device scalar slots (double)
  S_SQ = 0, S_SUM, S_NLL, S_V1, S_V2, S_V6, S_V7, S_H1, S_H2, S_C9, S_C10, S_TOTX, S_TOTY, S_CLAMPSUM,
  S_TMP, S_TMP2, S_CK0, S_CK1, S_CK2, S_CK3, S_COUNT = 32
};

struct GemmTimer {
  std::vector<hipEvent_t> ev;  // pairs
  size_t used = 0;
  int64_t launches = 0;
  double flops = 0;
};

// ---- What a call leaves for the next (the same table and invariants)
// (I1) An in-flight flag is true exactly from the launch that forks the work until a wait on its event has been enqueued on the
//      caller's stream by whoever adopts or drops it.
// (I2) An adoptable result is true only while M, the model and the graph are the ones it was computed from.
// (I3) No entry reads a StepScratch field before writing it in the same step or forward (a row-block rank's step or forward spans
//      mcgra_attack_shard_begin to its last shard_next).  The exceptions are written out at StepScratch.
// Three transitions change a Carry field from outside the code that forks or adopts it (attack_fused.hip):
//   carry_wait     the caller's stream waits for the event of every in-flight item; no flag changes
//   carry_drop     carry_wait, then the in-flight items and their bookkeeping are cleared (their results are scratch nobody reads)
//   carry_forget   M, the model or the graph changed: the adoptable results are cleared (fused_last describes the last STEP, not
//                  M: only a fused commit and the general step write it)
// Besides them a Carry field is written where the work is forked or its result stands (fw_prep, fork_p1 / fork_p1_early, the
// monitor call, the Adam passes, hsic_terms' masked-pair count, shard_next), and where a step adopts it (fs_begin, fs_pack_fork,
// step_general).  Every extern "C" entry that takes (h, stream) opens with its rule; a new entry point is a new row:
//
//   entry                          rule            what and why
//   set_model                      forget          nothing in flight reads the model (the pack reads M and r, the products read planes)
//   set_graph                      drop + forget   skip_fused is kept (see there: a hint about the order of the paths, never about a result)
//   set_adj_changes                drop + forget   M is overwritten: a pack may still be reading it
//   get_adj_changes, get_rows      none            they read M, which whatever is in flight also only reads
//   step (step_general)            take, drop      the fused step goes first (below); the general step adopts the cached forward and the Kx
//                                                  forked with it, and drops the rest: it packs its own operands
//     ... fused (fs_begin,         take            the forward a monitor call left, its pack (joined at ev_pack) and a row-block rank's
//         fs_pack_fork)                            product (handed to step.p1_inflight, joined by join_p1); an abandoned step: fused_resync
//   monitor                        none            it adds to what is in flight.  Forking an item again replaces it: the pack on its own side
//                                                  stream (fw_prep), Kx and a rank's product behind a drop (two monitor calls in a row)
//   finalize                       drop + forget   M is overwritten by the decode; skip_fused is kept (a step may follow: the parity tests do)
//   copy_buffer, product_replay    wait            scratch under a forked pack / product / Kx is read (or timed over) on the caller's stream
//   shard_begin                    none            no stream work; an abandoned monitoring forward takes the last one's result with it
//   shard_next                     as step / monitor
//   shard_scalars                  none            it reads scalar slots that the caller's stream wrote
//   buffer (no stream)             --              raw pointers: read them through copy_buffer, or behind the wait it performs
struct Carry {
  // -- adoptable results (I2)
  bool fwd_cached = false;         // adj_norm (ADJN_next), d, r, the victim chain and log-probs of the CURRENT M (general monitor call; fwd_reuse)
  bool fused_fwd_valid = false;    // both chains, heads, d / r / mean of the CURRENT M are in place (left by the fused monitor call)
  bool prep_valid = false;         // G_A holds the per-tile row sums of the current M (left by the Adam pass of the tail kernels)
  bool skip_fused = false;         // the last step's decode masked a pair: the general path goes first (it re-checks).  A hint: stale, it costs
                                   //   one step by the slower path, so set_graph, finalize and fused_resync keep it (carry_forget's argument)
  bool fused_last = false;         // the last step ran fused: adj_norm of that iteration was never stored (see em_last)
  // -- in flight on the side stream when the call returns (I1), each with the event that ends it
  bool early_pack = false;         // ev_pack: Bpack / the pack's row partials of the CURRENT M (packed beside the forward of this M)
  bool kx_early = false;           // ev_first (gram_ovl; else it ran on the caller's stream): Kx of the current M, forked by the last monitor call
  bool p1_early = false;           // ev_join: a row-block rank's pack + product, forked by the forward of the CURRENT M.  Its bookkeeping:
  bool p1_first = false;           //   the forked product was cut (the all-to-all waits for ev_first only; also set by a step's own fork)
  int p1_early_cut = 0, p1_early_split = 0;      //   what that launch adds to cut_product_steps / split_steps once a step takes it
};
// Scratch flags of one step or forward: on the handle only because the stages need them.  Exceptions to (I3):
//  - p1_inflight stays set, together with carry.p1_early, across the return of a row-block rank's forward (fs_pack_fork takes both);
//  - nmask_zero and t3_zero remember that a zero fill is still in place from the step before.  false is always right (the fill is
//    redone), so whoever may have written the words -- the general step, set_graph, an abandoned step -- just clears them.
struct StepScratch {
  bool lr_step = false;            // general step: it takes the low-rank form (no relu-masked pair in the decode)
  bool p1_inflight = false;        // the product P1 is forked and not yet joined
  int tail_rows = 0, tail_rows2 = 0;   // rows behind the first / second cut of this step's product (0: no early tail pass)
  bool planes_valid = false;       // uncentred planes of the CURRENT M are in Bpack (between the pack of a step and its Adam pass: planes_mm)
  bool nmask_zero = false;         // the decode's masked-pair counter holds 0 (left so by k_post_mask)
  bool t3_zero = false;            // column 2 he of lrT (t3 of the low-rank factors) holds zeros (fused step; the general path writes it)
  // the fused step's stages (attack_fused.hip)
  bool fs_adopted = false;         // fs_begin: the step took the forward a monitor call left (fs_forward then passes)
  int fs_l = 0;                    // fw_layer_product / fw_layer_post: the forward's layer; fs_decode_bwd, fs_bwd_product / fs_bwd_post:
  int fs_l2 = 0;                   //   the backward levels still to do, victim chain | modified_adj chain; fs_gather_*: the gather (fs_l)
  int fs_np = 0;                   // fs_decode: row partials of the decode's entropy term
  int fs_nblk = 0;                 // fs_tail_reduce: blocks of the tail's first pass (partials of the loss terms' values)
  bool fs_dec_forked = false;      // fs_decode: the decode runs on the fourth stream; its first reader joins it (fs_small_terms, fs_decode_bwd)
};

struct mcgra_attack {
  mcgra_attack(const mcgra_attack_config_t& c, const mcgra::AttackPlan& plan) : cfg(c), p(plan) {}
  const mcgra_attack_config_t cfg;
  const mcgra::AttackPlan p;       // what create decided (attack_plan.h: every switch is described there): the only copy, constant
  // The one bit of per-graph state (set_graph).  A non-zero ori_adj (never produced by main.py, accepted by the class:
  // topology_attack.py:164, :185, :188, :302): the general path only (the predicates below the struct).  modified_adj =
  // clamp(M + ori + eps noise) lives in Abuf (with its clamp gate), the embedding runs on Bbuf = modified_adj - ori in its own
  // chain (Te / Pe / He / GPe) while output2 keeps the chain on modified_adj.
  bool has_ori = false;
  Carry carry;                     // what the last call left for the next (above)
  StepScratch step;                // scratch flags of the step / forward in progress (above)
  int64_t t = 0;                   // Adam step count
  bool have_step = false;
  bool m_is_full = true;           // every row of M is current (a row-block rank after its first step holds its own rows only, until finalize)
  int test_mutate = 0;             // TEST-ONLY (mcgra_attack_test_mutate, see attack_fused.hip): 1 wipes P1, 2 drops the tail's rank-k terms,
                                   // 3 zeroes MSELoss / KL's per-pair multipliers, 4 wipes the KL row statistics
  float* ADJN_next = 0;            // adj_norm of the monitoring forward, adopted by the next step (p.fwd_reuse)
  bool graph_set = false, model_set = false;
  std::vector<void*> allocs;
  // N x N
  float *M = 0, *am = 0, *av = 0, *ADJN = 0, *A1 = 0, *G_ADJN = 0, *G_A1 = 0, *G_A = 0;
  float *KX = 0, *KY = 0, *KFC = 0, *FADJ = 0, *GSYM = 0, *XC = 0, *YC = 0;
  // vectors
  float *cmean = 0;                // fp32 column means for the centring passes
  float *d = 0, *r = 0, *rowpart = 0, *colpart = 0, *gd = 0, *nrm = 0, *cnt = 0, *rowmin = 0, *rowmax = 0, *mm = 0;
  double *rowsq = 0, *rowsum = 0, *rowvals = 0, *rowsx = 0, *rowsy = 0, *scal = 0;
  int *labels = 0, *idx = 0, *correct = 0;
  // weights
  float* W[MCGRA_MAX_LAYERS] = {0};
  float* b[MCGRA_MAX_LAYERS] = {0};
  float *Wlin = 0, *blin = 0;
  float* Ws[MCGRA_MAX_LAYERS] = {0};   // GraphSAGE self weights (has_self), [dims[l] x dims[l+1]]
  float *S0 = 0, *Sv = 0, *Su = 0;    // self terms X Ws_0 (constant) and H_{l-1} Ws_l of both chains
  // node-level
  float *Tv = 0, *Pv = 0, *Hv = 0, *GPv = 0;   // victim(adj_norm) chain, [n x hsum]
  float *Tu = 0, *Pu = 0, *Hu = 0, *GPu = 0;   // victim/embedding(modified_adj) chain
  float *Y = 0, *GT = 0, *Z = 0, *logp = 0, *sm = 0, *Z2 = 0, *sm2 = 0, *GZ = 0, *GZ2 = 0, *Gsm = 0;
  float *Zn = 0, *GZn = 0, *Gem = 0;
  float *HA = 0, *YA = 0, *HAg = 0, *HAc = 0, *YAg = 0, *YAc = 0, *Yg = 0, *Gg = 0, *Q = 0;
  float *Q2 = 0, *Gg2 = 0, *coef = 0;
  // has_ori (above): allocated by the first set_graph that brings one
  float *ORI = 0, *Bbuf = 0, *Te = 0, *Pe = 0, *He = 0, *GPe = 0, *Se = 0;
  float* Abuf = 0;                 // modified_adj after adding_noise (only when eps != 0 or ori != 0; otherwise it is M itself)
  unsigned char* gate = 0;         // clamp pass-through mask of adding_noise's torch.clamp
  double* colpart_d = 0;
  double* cm_part = 0;             // scratch of launch_colmean_center
  double* Yg8 = 0;                 // softmax(output2)[idx] in float64 (linear_HSIC's c10: launch_softmax8_centered)
  double* kde = 0;                 // measure KDE: tables + per-block partials of one term (kde_kernels.hip: kde_scratch_doubles)
  int kde_cols = mcgra::KDE_NXN_COLS;   // ... columns of the N x N operands whose kernel values can be non-zero in float32 (set_graph: from max |feature_adj|)
  double* cst = 0;                 // constants of the CKA terms: [0] hsic(Fadj,Fadj), [1] hsic(HA,HA), [2] hsic(YA,YA)
  float* ws = 0;
  size_t ws_bytes = 0;
  int nstrips = 32;
  bool profile = false;
  // low-rank linear_HSIC(adj_norm, modified_adj1) (lowrank_kernels.hip; p.lr_ok)
  float *lrL = 0, *lrV = 0, *lrT = 0, *lrR = 0, *lrQ = 0, *lrDelta = 0, *lrC = 0;
  double *lrStats = 0, *lrRs = 0, *lrQtZ = 0;
  unsigned int* nmask = 0;
  int64_t lr_steps = 0, general_steps = 0;
  // second stream: the one N x N x N product of the low-rank path depends only on adj_norm, so it is forked
  // right after the normalisation and runs (MFMA-bound) under the HBM-bound rest of the step
  hipStream_t st2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // row-block ranks: ev_first is recorded behind the first part of a cut product (p.a2a_overlap; monolithic: p.early_tail_on)
  hipEvent_t ev_first = nullptr, ev_second = nullptr;
  // early pack (p.early_pack_on): ev_r: r ready; ev_pack: planes and row partials ready
  hipEvent_t ev_r = nullptr, ev_pack = nullptr;
  float* small_slab = nullptr;     // split-K slabs of a small graph's N x N x N products (more than an N x N buffer holds: split3_small_slab_bytes)
  size_t small_slab_bytes = 0;
  bool fs_last = false;            // the monitor call in progress was begun as MCGRA_SHARD_MONITOR_LAST
  // third stream of the fused step: the small-operand terms c9 / c10 (a chain of ~16 tiny launches that needs only the
  // forward) run beside the low-rank factor chain; its products use their own split-K workspace
  hipStream_t st3 = nullptr;
  hipEvent_t ev_fork3 = nullptr, ev_join3 = nullptr;
  float* ws_small = nullptr;
  size_t ws_small_bytes = 0;
  // fourth stream of the (monolithic) fused step: the decode recomputed per pair (the longest node-level kernel, needs
  // only Zn) beside the low-rank factor chain, with its own slab buffer
  hipStream_t st4 = nullptr;
  hipEvent_t ev_fork4 = nullptr, ev_join4 = nullptr;
  float* ws_dec = nullptr;
  // The decode's masked-pair count of the fused step is posted to mapped host memory by k_post_mask together with a
  // launch sequence number ({seq, masked}); the host polls it in front of the Adam pass (no stream sync).
  volatile unsigned int* mask_host = nullptr;    // [0] sequence number of the post, [1] masked != 0
  unsigned int* mask_host_dev = nullptr;         // the same words through the device's address space
  unsigned int* mask_seq_dev = nullptr;          // device-side counter of the posts
  unsigned int mask_seq = 0;                     // posts enqueued so far (moves where k_post_mask is launched)
  unsigned int mask_want = 0;                    // sequence number of the post the step in flight will poll for
  int64_t cut_product_steps = 0;   // row-block steps whose product was cut for the all-to-all (a2a_overlap)
  int64_t masked_fused_steps = 0;  // fused steps whose decode relu-masked pairs of live rows (they stand: DESIGN.md section 1b)
  unsigned char *Apack = 0, *Bpack = 0;      // packed planes of the split product's operands (p.split_on)
  float *amax = 0;                 // [0] max |H Kf H| (per graph), [1] max |Xc| (per step, from the centring pass)
  int64_t split_steps = 0;
  // Gram evaluation through the split kernel (p.gram_split)
  double* gram_diag = 0;           // [2][ld]: |xc_i|^2, |yc_i|^2 (diagonals of the centred Grams: scale bound of the combined Grams)
  unsigned char *Gp0 = 0, *Gp1 = 0, *Gp2 = 0;
  int64_t gram_split_steps = 0;
  GemmTimer timer;
  // fused step (attack_fused.hip; p.fused)
  float *klA = 0, *kl1 = 0, *klv = 0;      // fused KL step: logsumexp of adj_norm's rows, of modified_adj1's rows, v_i = the row's share of c2
  double *klpart = 0, *klvsum = 0;         // ... per-(column slice, row) partials of the two passes [64][n][2]; v_i in fp64 [ld]
  float *FV = 0, *FY = 0;          // right-hand sides / results of the skinny products on M  [n x p.fcols]
  mcgra::YView fy{nullptr, 0, 1, 0};      // the last such product as its consumers read it (FY, or the split-K slabs in ws)
  char* rkbuf = 0;                 // packed fp16 planes of the tail's rank-k panels (fl_tail_pack_bytes)
  float *em_last = 0;              // embedding(features, adj_norm) of the last iteration (:300), = its victim-chain activations
  double *fstat = 0;               // small fp64 vectors: colsum(V) [64] | colsum(W) [64] | mean^T W [64] | sum(mean) [2]
  char* pm_scratch = nullptr;      // scratch of planes_mm.hip (p.planes_mm_on)
  char* sx_scratch = nullptr;      // packed right-hand side of skinny_x3 (p.fwd_x3)
  float* Zpair = nullptr;          // pair-interleaved copy of Zn for the decode's scalar loads (fused_lowrank.hip: k_decode_fly_s)
  int64_t fused_steps = 0;
  // row-block sharding (mcgra_attack_shard_*; p.sharded, p.world ... p.fyw)
  char* arena = nullptr;           // caller-owned exchange arena (mcgra_attack_bind_exchange)
  int64_t arena_bytes = 0;
  int64_t off_fy = 0, off_sg = 0, off_sc = 0, off_a2s = 0, off_a2r = 0, off_nxn = 0;
  float *SG = 0, *A2S = 0, *A2R = 0, *NXS = 0;   // views into the arena: n-vector stage [p.npad][p.sgw], all-to-all send / recv, N x N stage
  double* SC = 0;                  // 16 scalars summed over the ranks (from the stages' scalar lanes)
  // The fused step as a table of stages (attack_fused.hip: FS_STAGES, and FW_STAGES for its forward): a row-block rank runs it
  // to the next exchange point and returns.  The step's constants are rebuilt on every entry (FusedStep); only these cross an
  // exchange:
  int fs_state = 0, fw_state = 0;  // index of the next stage of the step / of the forward (0: from the top)
  int fs_what = 0, fs_want = 0;    // what mcgra_attack_shard_begin asked for: MCGRA_SHARD_*; scalars (2: already collected)
  bool fs_active = false;          // between shard_begin and the last shard_next
  bool fs_open = false;            // a fused step was started and has not reached a regular exit (see fused_resync)
  // ... and the stages' own counters and flags (step.fs_*)
  double fs_scalars[10] = {0};
};

// ---- the planned paths as the graph in place allows them
// A non-zero ori_adj takes the general path only: the fused / low-rank forms assume modified_adj == M and modified_adj1 ==
// offdiag relu(Zn Zn^T), and the monitoring forward (:290-293) runs on the UNclamped M + ori, so there is nothing for the next
// step to adopt; a later graph without one has the planned paths again.  (create allocates from the raw plan: the buffers must be
// there for that later graph.)
static inline bool lr_ok(const mcgra_attack* h) { return h->p.lr_ok && !h->has_ori; }
static inline bool fused_ok(const mcgra_attack* h) { return h->p.fused != mcgra::FUSED_NONE && !h->has_ori; }
static inline bool gram_split(const mcgra_attack* h) { return h->p.gram_split && !h->has_ori; }
static inline bool late_mean(const mcgra_attack* h) { return h->p.late_mean && !h->has_ori; }
static inline bool planes_mm_on(const mcgra_attack* h) { return h->p.planes_mm_on && !h->has_ori; }
static inline bool fwd_reuse(const mcgra_attack* h) { return h->p.fwd_reuse && !h->has_ori; }

// ---- scratch layouts the fused and the general step share
// The operand pack's per-block row partials in A1: sums of squares [n][np], and behind them (16-byte aligned) the row sums [n][np]
static inline float* pack_row_sums(const mcgra_attack* h, int np) { return h->A1 + (((size_t)h->p.n * np + 3) & ~(size_t)3); }
// The row partials of the new M an Adam pass leaves in G_A for the next forward (prep_from_partials): cnt = n * tiles floats,
// and behind them (8-byte aligned) as many fp64 row sums ...
static inline double* adam_row_sums(const mcgra_attack* h, size_t cnt) { return reinterpret_cast<double*>(h->G_A + ((cnt + 1) & ~(size_t)1)); }
// The edge-budget projection (:339) can follow the Adam pass: clamp(a, 0, 1).sum() <= n (n - 1) / 2, so a larger budget never
// triggers the bisection.
static inline bool may_project(const mcgra_attack* h) { return h->cfg.num_edges < 0.5 * (double)h->p.n * (double)h->p.n; }
// ... which it emits when no projection follows and they fit into G_A.  prep_valid says the same: ONE predicate for both.
static inline bool adam_emits_partials(const mcgra_attack* h, size_t cnt) {
  return !may_project(h) && 3 * cnt + 4 <= (size_t)h->p.n * h->p.ld;
}
// Adam step t (1-based) on M / am / av, for whichever of the three Adam kernels runs it: the only copy of the hyper-parameters
// (torch.optim.Adam's defaults).  emit_cnt: 0, or the pass leaves its cnt row partials of the new M in G_A (adam_row_sums).
static inline mcgra::AdamUpdate adam_update(const mcgra_attack* h, int64_t t, size_t emit_cnt = 0) {
  const double b1 = 0.9, b2 = 0.999;
  const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
  mcgra::AdamUpdate u{};
  u.M = h->M; u.am = h->am; u.av = h->av;
  u.omb1 = (float)(1.0 - b1); u.b2 = (float)b2; u.omb2 = (float)(1.0 - b2);
  u.step_size = (float)(h->cfg.lr / bc1); u.sqrt_bc2 = (float)sqrt(bc2); u.eps = 1e-8f;
  u.cn = h->mm + 2;
  u.gsym_dbg = h->p.keep_gsym ? h->GSYM : nullptr;
  u.do_clamp = may_project(h) ? 0 : 1;
  if (emit_cnt) { u.ps_out = h->G_A; u.pq_out = adam_row_sums(h, emit_cnt); }
  return u;
}

// attack_fused.hip
bool fused_step_possible(const mcgra_attack* h);
int carry_wait(mcgra_attack* h, hipStream_t st);         // the transitions of Carry (above)
int carry_drop(mcgra_attack* h, hipStream_t st);
void carry_forget(mcgra_attack* h, bool keep_skip_fused = false);
int fused_forward(mcgra_attack* h, hipStream_t st);
// returns 1 when the step must be redone by the general path (a relu-masked pair in the decode), 0 when done
int fused_step(mcgra_attack* h, hipStream_t st, double* scalars_out);
int64_t fused_exchange_bytes(const mcgra_attack* h);
extern "C" int step_general(mcgra_attack_t* h, void* stream, const float* noise, double* scalars_out);     // attack.hip: every row, replicated

#define CHK(expr)            \
  do {                       \
    int rc__ = (expr);       \
    if (rc__ != 0) return rc__; \
  } while (0)


// ---- shared helpers (attack.hip)
int timer_begin(mcgra_attack* h, hipStream_t st, bool big);
int timer_end(mcgra_attack* h, hipStream_t st, bool big, double flops);
int eg(mcgra_attack* h, hipStream_t st, bool ta, bool tb, int M, int N, int K, float alpha, const float* A, int lda,
       const float* B, int ldb, float beta, float* C, int ldc, mcgra::YView* keep = nullptr);      // keep: a split-K product stays in its slabs (h->ws) for the next kernel
int head_forward(mcgra_attack* h, hipStream_t st, const float* H, float* Z, float* logp, float* sm);
double sign_of(const mcgra_attack* h);
extern "C" {      // (defined inside attack.hip's extern "C" block)
int small_term(mcgra_attack* h, hipStream_t st, int width, const float* Ysrc, int ldy, const float* Xg, const float* Xc,
               double k_signed, float* G, int ldg, int slot, bool want_value = true);   // want_value: also the term's value (HSIC: not needed for the gradient)
int project(mcgra_attack* h, hipStream_t st);
int collect_scalars(mcgra_attack* h, hipStream_t st, double* scalars_out, bool have_clampsum = false);
__global__ void k_cn(const double* __restrict__ scal, float coef, float* __restrict__ out);
__global__ void k_post_mask(unsigned int* __restrict__ count_u32, const double* __restrict__ count_f64,
                            unsigned int* __restrict__ seq_dev, unsigned int* __restrict__ host_slot);

}
