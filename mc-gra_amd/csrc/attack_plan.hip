// The attack engine's create-time decisions as one pure function of (configuration, environment): attack_plan.h.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/mcgra.h"
#include "common.h"
#include "kernels.h"
#include "attack_plan.h"

namespace mcgra {

static int first_char(const char* v) { return v ? (unsigned char)v[0] : -1; }

// The A/B switches of the parity suite and of the measurements under profiles/  are honoured only when
// MCGRA_AB=1 is set beside them: a variable left in the environment of a real run changes nothing -- and says so once.
static int ab_env(const char* name) {
  const char* v = getenv(name);
  if (!v) return -1;
  const char* on = getenv("MCGRA_AB");
  if (on && on[0] == '1') return first_char(v);
  // (said once per variable and process, not once per engine)
  static std::mutex mu;
  static std::vector<std::string> said;
  std::lock_guard<std::mutex> lock(mu);
  for (const std::string& s : said) if (s == name) return -1;
  said.emplace_back(name);
  fprintf(stderr, "[mcgra] %s=%s is ignored: A/B switches are honoured only under MCGRA_AB=1\n", name, v);
  return -1;
}

PlanEnv read_plan_env() {
  PlanEnv e;
  e.split_bf16 = first_char(getenv("MCGRA_SPLIT_BF16"));
  e.testing = first_char(getenv("MCGRA_TESTING"));
  e.keep_gsym = ab_env("MCGRA_KEEP_GSYM");
  e.no_fwd_reuse = ab_env("MCGRA_NO_FWD_REUSE");
  e.no_fused_tail = ab_env("MCGRA_NO_FUSED_TAIL");
  e.no_lowrank = ab_env("MCGRA_NO_LOWRANK");
  e.gram_split = ab_env("MCGRA_GRAM_SPLIT");
  e.overlap = ab_env("MCGRA_OVERLAP");
  e.gram_overlap = ab_env("MCGRA_GRAM_OVERLAP");
  e.gram_kx_early = ab_env("MCGRA_GRAM_KX_EARLY");
  e.small_side = ab_env("MCGRA_SMALL_SIDE");
  e.no_fused_lr = ab_env("MCGRA_NO_FUSED_LR");
  e.no_fused_post = ab_env("MCGRA_NO_FUSED_POST");
  e.early_pack = ab_env("MCGRA_EARLY_PACK");
  e.early_p1 = ab_env("MCGRA_EARLY_P1");
  e.early_tail = ab_env("MCGRA_EARLY_TAIL");
  e.mse_decode_side = ab_env("MCGRA_MSE_DECODE_SIDE");
  e.mse_small_inline = ab_env("MCGRA_MSE_SMALL_INLINE");
  e.planes_mm = ab_env("MCGRA_PLANES_MM");
  e.fwd_x3 = ab_env("MCGRA_FWD_X3");
  e.p1_behind_pack = ab_env("MCGRA_P1_BEHIND_PACK");
  e.a2a_overlap = ab_env("MCGRA_A2A_OVERLAP");
  return e;
}

// a 0 / 1 switch that overrides a default when it is set to something
static bool forced_or(int sw, bool dflt) { return sw > 0 ? sw == '1' : dflt; }

static const char* const MEASURE_NAME[] = {"HSIC", "MSELoss", "KL", "CKA", "DP", "KDE"};

int plan_attack(const mcgra_attack_config_t& cfg, const PlanEnv& env, AttackPlan* p) {
  *p = AttackPlan();
  if (cfg.n < 2 || cfg.nlayer < 2 || cfg.nlayer > MCGRA_MAX_LAYERS || cfg.emb_nlayer < 1 || cfg.emb_nlayer > cfg.nlayer ||
      cfg.nclass < 1 || cfg.n_attack < 1) {
    set_error("bad config: n=%d nlayer=%d emb_nlayer=%d nclass=%d n_attack=%d", cfg.n, cfg.nlayer, cfg.emb_nlayer, cfg.nclass,
              cfg.n_attack);
    return MCGRA_EINVAL;
  }
  if (cfg.measure < MCGRA_MEASURE_HSIC || cfg.measure > MCGRA_MEASURE_KDE) {
    set_error("measure %d: HSIC, MSELoss, KL, CKA, DP, KDE (topology_attack.py:194-208)", cfg.measure);
    return MCGRA_ENOSUP;
  }
  if (cfg.measure == MCGRA_MEASURE_KDE && (cfg.dims[cfg.emb_nlayer] > KDE_MAXC || cfg.nclass > KDE_MAXC)) {
    set_error("measure KDE: embedding width %d / %d classes; the c x c joint of utils.MutualInformation is built for widths <= %d",
              cfg.dims[cfg.emb_nlayer], cfg.nclass, KDE_MAXC);
    return MCGRA_ENOSUP;
  }
  if (cfg.shard_world < 0 || (cfg.shard_world == 0 && (cfg.row_begin != 0 || (cfg.row_end != 0 && cfg.row_end < cfg.n)))) {
    set_error("row block [%d, %d) without shard_world", cfg.row_begin, cfg.row_end);
    return MCGRA_EINVAL;
  }
  if (cfg.shard_world > 0) {
    const int rpr = cfg.shard_rows;
    if (rpr < 256 || rpr % 256 != 0 || (long long)rpr * cfg.shard_world < cfg.n || cfg.row_begin % rpr != 0 ||
        cfg.row_begin / rpr >= cfg.shard_world ||
        cfg.row_end != (cfg.row_begin + rpr < cfg.n ? cfg.row_begin + rpr : (cfg.row_begin < cfg.n ? cfg.n : cfg.row_begin))) {
      set_error("row block [%d, %d) is not rank %d's block of %d x %d rows (shard_rows: a multiple of 256 with shard_rows * "
                "shard_world >= n)", cfg.row_begin, cfg.row_end, rpr > 0 ? cfg.row_begin / rpr : -1, cfg.shard_world, rpr);
      return MCGRA_EINVAL;
    }
  }
  p->fin0 = cfg.fin_layers[0] > 0 ? cfg.fin_layers[0] : 1;
  p->fin1 = cfg.fin_layers[1] > 0 ? cfg.fin_layers[1] : 2;
  if (p->fin0 > cfg.nlayer || p->fin1 > cfg.nlayer || cfg.act < 0 || cfg.act > 1) {
    set_error("bad act / fin_layers");
    return MCGRA_EINVAL;
  }
  const int n = p->n = cfg.n;
  // rows of the N x N buffers start on 128-byte lines (ld a multiple of 32 floats; round 3: of 4): the 64- and 128-column
  // tile rows of the tail, the pack and the skinny products are then whole lines (+1 ... 2 % steps/s at N = 10 000, where
  // ld = 10 016; profiles/r04_ab_edge_tiles_ld_align.txt).
  const int ld = p->ld = (n + 31) & ~31;
  const int L = p->L = cfg.nlayer;
  p->Le = cfg.emb_nlayer;
  p->C = cfg.nclass;
  p->na = cfg.n_attack;
  int o = 0, hm = cfg.nclass;
  for (int l = 0; l < L; ++l) {
    p->off[l] = o;
    p->wdt[l] = cfg.dims[l + 1];
    if (p->wdt[l] < 1) { set_error("bad dims[%d]", l + 1); return MCGRA_EINVAL; }
    o += (p->wdt[l] + 3) & ~3;
    if (p->wdt[l] > hm) hm = p->wdt[l];
  }
  p->hsum = o;
  p->hmax = (hm + 3) & ~3;
  const int he = p->wdt[p->Le - 1];
  const bool relu_gcn = !cfg.has_self && cfg.act == 0 && cfg.head_act == 0;
  const bool hsic = cfg.measure == MCGRA_MEASURE_HSIC;
  const bool elementwise = cfg.measure == MCGRA_MEASURE_MSE || cfg.measure == MCGRA_MEASURE_KL;

  p->keep_gsym = env.keep_gsym == '1';
  p->testing = env.testing == '1';
  p->fwd_reuse = cfg.eps == 0.f && env.no_fwd_reuse != '1';
  p->fuse_tail = env.no_fused_tail != '1';
  p->lr_ok = hsic && cfg.act == 0 && he <= 32 && env.no_lowrank != '1';
  if (p->lr_ok) p->lr_ldv = (2 * he + 1 + 3) & ~3;

  // The one N x N x N product of a low-rank step.  Default for n >= 1024: the 2-plane fp16 split on the 16-bit matrix
  // cores (split_symm_bf16.hip: fp32-level error, three plane products).  MCGRA_SPLIT_BF16=0: fp32 MFMA SYMM;
  // =2: the 3-plane bf16 split kernel (six products, fp32 exponent range) at any size; =3: the 2-plane fp16
  // kernel at any size.
  // =1: the fp16 x 2 operands, ONE plane product (fp16 accuracy: 2^-11 per operand; a third of the matrix-core work) -- what "bf16 MFMA"
  // in BASELINE.json's configs[2] / [4] means taken literally.  Never a default: the reference's CPU path is fp32.
  const bool split_asked = env.split_bf16 > 0;      // (the first character decides)
  const int sm = split_asked ? env.split_bf16 : (n >= 1024 ? '3' : '0');
  p->split_single = sm == '1';      // (by name only: also the Gram evaluation's four products, below)
  if (p->lr_ok && cfg.eps == 0.f && (sm == '1' || sm == '2' || sm == '3')) {
    p->split_on = true;
    p->split_planes = sm == '2' ? 3 : 2;
    p->split_mode = 2;
  }
  // The Gram evaluation of HSIC (steps the low-rank forms do not cover: a masked decode, GAT / SAGE chains,
  // MCGRA_NO_LOWRANK) through the 2-plane fp16 kernel as well: Kx = Xc Xc^T and Ky = Yc Yc^T as full matrices, then
  // G_adjn += Ky' Xc and G_A1 += Kx' Yc -- four products of 2 n^3 instead of 3 n^3 MACs of fp32 SYMM at a third of
  // their rate.  MCGRA_GRAM_SPLIT=0: fp32 path.  (The Gram evaluation's products stay 3-product splits under =1.)
  if ((hsic || cfg.measure == MCGRA_MEASURE_CKA) && cfg.eps == 0.f && (sm == '3' || sm == '1') && env.gram_split != '0') {
    p->gram_split = true;
    p->split_planes = 2;      // (what a split product of these modes has as well)
  }
  // The product on the engine's own stream, beside the HBM-bound kernels of the step that do not need it.  On by
  // default with the 2-plane fp16 kernel (64 KB of LDS and 212 VGPRs per CU leave room for them: 9.1 vs 9.4 ms per
  // step at N = 10 000 although the product itself slows from 4.8 to 5.6 ms); the fp32 SYMM and the 3-plane kernel
  // hold every CU's LDS and registers, so what runs beside them crawls and slows them by about as much as it hides
  // (measured: 21.2-21.5 ms with the side stream, 21.6 without).  MCGRA_OVERLAP=0 / 1 overrides.
  p->overlap = forced_or(env.overlap, p->split_mode == 2 && p->split_planes == 2);
  // (the fused MSELoss and KL steps -- attack_fused.hip -- use the side streams of the small-operand terms and of the decode too)
  p->side_streams = p->lr_ok || p->gram_split || (elementwise && cfg.eps == 0.f && relu_gcn);
  if (p->side_streams) {
    // Gram evaluation: its four products on the side stream, beside the HBM-bound rest of the step (gram_eval).
    // MCGRA_GRAM_OVERLAP=0: everything on the caller's stream, same launches in the same order (bit-identical: A/B test)
    p->gram_ovl = p->gram_split && env.gram_overlap != '0';
    // ... and the first of them forked by the monitoring forward (configurations without a low-rank form; MCGRA_GRAM_KX_EARLY=0: by the step)
    p->kx_early_on = p->gram_ovl && !p->lr_ok && p->fwd_reuse && env.gram_kx_early != '0';
    // (KDE: its small-operand terms share one scratch table with the N x N terms -- they stay on the caller's stream)
    p->small_side_on = cfg.measure != MCGRA_MEASURE_KDE && env.small_side != '0';
  }

  // The fused steps (attack_fused.hip).  HSIC: the low-rank step with every N x N quantity from M and n-vectors, on the split
  // product.  MSELoss (round 5): calc = MSELoss is elementwise in (M, feature_adj, r, Zn), so the same two tail passes over tile
  // pairs serve it with no N x N x N product and no N x N intermediate (adj_norm, modified_adj1, the gradients w.r.t. them are
  // never stored) -- and a row-block rank needs no N x N exchange at all.  KL (round 6): calc = calc_kl (:197-198, :483-487) is
  // elementwise in the same quantities plus per-row softmax statistics of adj_norm and modified_adj1 -- the MSELoss step's data
  // flow with one more per-pair pass for the statistics; softmax(feature_adj) (XC, constant per graph) takes feature_adj's place
  // in the tail.  MCGRA_NO_FUSED_LR=1: general path only.
  // widest skinny product on M: [r o Tv | Tu] + the means column, or the low-rank factors beside the last layer's; the
  // elementwise measures have no means column and no low-rank factors
  int fc = elementwise ? 0 : 2 * he + 1 + p->wdt[L - 1];
  for (int l = 0; l < L; ++l) {
    const int w = 2 * p->wdt[l] + (elementwise ? 0 : 1);
    if (w > fc) fc = w;
  }
  fc = (fc + 3) & ~3;
  const int kmax = p->hsum > 2 * he ? p->hsum : 2 * he;      // rank-k depth of the tail's panels
  char* why = p->why_not_fused;
  const size_t wn = sizeof(p->why_not_fused);
  // the rule, in the order its refusals are reported: what the three steps share ...
  if (!hsic && !elementwise)
    snprintf(why, wn, "measure %s has no fused step (HSIC, MSELoss and KL have one)", MEASURE_NAME[cfg.measure]);
  else if (env.no_fused_lr == '1')
    snprintf(why, wn, "MCGRA_NO_FUSED_LR=1");
  else if (cfg.eps != 0.f)
    snprintf(why, wn, "eps != 0 (adding_noise makes modified_adj asymmetric: general step)");
  else if (!relu_gcn)
    snprintf(why, wn, "a GAT / GraphSAGE victim (the fused steps cover the ReLU GCN chain without self weights)");
  else if (!lr_decode_supported(he))
    snprintf(why, wn, "embedding width %d (the per-pair decode is built for widths 8, 16 and 32)", he);
  else if (!fl_tail_supported(n, ld, kmax) && n < 256)
    snprintf(why, wn, "n = %d < 256", n);
  else if (!fl_tail_supported(n, ld, kmax))
    snprintf(why, wn, "summed layer widths %d / twice the embedding width %d > 64 (rank-k depth of the tail's panels: e.g. more "
             "than four 16-wide layers)", p->hsum, 2 * he);
  else if (fc > 64)
    snprintf(why, wn, "skinny products of %d columns > 64", fc);
  // ... and what HSIC adds: the low-rank form, the split product, an N x N term
  else if (hsic && !p->lr_ok)
    snprintf(why, wn, "MCGRA_NO_LOWRANK=1");
  else if (hsic && !p->split_on && split_asked)
    snprintf(why, wn, "MCGRA_SPLIT_BF16=%c (the product runs on the fp32 kernel; 1, 2 and 3 are the split modes)", (char)sm);
  else if (hsic && !p->split_on)
    snprintf(why, wn, "n = %d < 1024 without MCGRA_SPLIT_BF16=1/2/3 (the product runs on the fp32 kernel)", n);
  else if (hsic && cfg.w[0] == 0.f && cfg.w[1] == 0.f)
    snprintf(why, wn, "w1 == w2 == 0 (no N x N HSIC term)");
  else
    p->fused = hsic ? FUSED_HSIC : (cfg.measure == MCGRA_MEASURE_MSE ? FUSED_MSE : FUSED_KL);
  if (p->fused) p->fcols = fc;

  p->fused_post = env.no_fused_post != '1';
  p->early_pack_on = env.early_pack != '0';
  p->early_p1_on = cfg.shard_world > 0 && env.early_p1 != '0';
  p->early_tail_on = env.early_tail != '0';
  p->mse_decode_side = env.mse_decode_side == '1';
  p->mse_small_inline = env.mse_small_inline != '0';
  p->late_mean = p->fused == FUSED_HSIC && cfg.shard_world == 0;
  // default from n = 8192: on smaller graphs the step is bound by its chain of launches, and the two extra launches per
  // product (magnitude + pack of the right-hand side) cost more than the matrix-pipe time they free (Cora-shape step
  // 0.51 -> 0.56 ms, N = 4096 0.86 -> 0.92 ms with it); MCGRA_PLANES_MM=1 forces it on (tests), =0 off
  p->planes_mm_on = p->late_mean && p->split_planes == 2 && planes_mm_supported(n, 32) && forced_or(env.planes_mm, n >= 8192);
  {
    // The forward of a step whose planes the early pack makes on the product's stream (attack_fused.hip) needs nothing the
    // product reads or writes, so the product is forked behind the pack and the forward runs beside it -- on skinny_x3.hip,
    // whose blocks fit beside a product block, not on gemm_f32, whose blocks do not.  Default from n = 8192, where the
    // product is long enough to hide the forward; MCGRA_FWD_X3 / MCGRA_P1_BEHIND_PACK = 0 / 1 force each part (A/B).
    const bool can = p->late_mean && p->overlap && p->early_pack_on && p->split_planes == 2;
    int wf = 0;      // (the forward's widest product: [r o Tv_l | Tu_l])
    for (int l = 0; l < L; ++l) wf = 2 * p->wdt[l] > wf ? 2 * p->wdt[l] : wf;
    p->fwd_x3 = can && forced_or(env.fwd_x3, n >= 8192) && skinny_x3_supported(n, wf, ld);
    p->p1_behind_pack_on = can && forced_or(env.p1_behind_pack, p->fwd_x3);
  }

  // row-block ranks: only the fused steps are sharded, and the host-driven bisection of the projection is not
  p->row0 = 0; p->row1 = n;
  if (!p->fused)
    snprintf(p->why_not_sharded, sizeof(p->why_not_sharded), "%s", p->why_not_fused);
  else if (cfg.num_edges < 0.5 * (double)n * (double)n)
    snprintf(p->why_not_sharded, sizeof(p->why_not_sharded), "a projection budget that can bind (host-driven bisection)");
  else
    p->shardable = true;
  if (cfg.shard_world > 0 && !p->shardable) {
    set_error("shard_world > 0 needs a configuration a fused step covers and a projection budget that cannot bind: %s",
              p->why_not_sharded);
    return MCGRA_ENOSUP;
  }
  if (cfg.shard_world > 0) {
    p->sharded = true;
    p->world = cfg.shard_world; p->rpr = cfg.shard_rows; p->rank = cfg.row_begin / cfg.shard_rows;
    p->npad = p->rpr * p->world;
    p->row0 = cfg.row_begin; p->row1 = cfg.row_end;
    // exchanged node arrays (attack_fused.hip: wide_stage / narrow_stage): n-vector columns (decode backward | |xc_i|^2 as
    // two words) + a two-column scalar lane; the wide one carries a product's fcols columns in front of them
    p->sgw = ((he + 2 + 3) & ~3) + 2;
    p->fyw = fc + p->sgw;
    // the all-to-all of P1 beside the own row panels of the product (attack_fused.hip): free when a whole round of the chip
    // ends behind the peers' tiles, worth a second ragged round while world <= 4 (world 8 at N = 10 000: 200 tiles on 256
    // CUs, nothing to run beside)
    p->a2a_overlap = env.a2a_overlap >= 0 ? (env.a2a_overlap == '1' ? 2 : 0) : (p->world >= 2 ? 1 : 0);
  }
  return 0;
}

// every flag of the plan, one "name=value" per line
static void plan_text(const AttackPlan& p, char* out, size_t cap) {
  size_t len = 0;
  out[0] = 0;
  auto put = [&](const char* name, long long v) {
    if (len < cap) len += (size_t)snprintf(out + len, cap - len, "%s=%lld\n", name, v);
  };
  auto put_list = [&](const char* name, const int* v) {
    std::string s;
    for (int l = 0; l < p.L; ++l) s += (l ? "," : "") + std::to_string(v[l]);
    if (len < cap) len += (size_t)snprintf(out + len, cap - len, "%s=%s\n", name, s.c_str());
  };
#define P_(f) put(#f, (long long)p.f)
  P_(n); P_(ld); P_(L); P_(Le); P_(C); P_(na); P_(hsum); P_(hmax); P_(fin0); P_(fin1);
  put_list("off", p.off); put_list("wdt", p.wdt);
  P_(keep_gsym); P_(testing); P_(fwd_reuse); P_(fuse_tail); P_(lr_ok); P_(lr_ldv); P_(split_on); P_(split_planes); P_(split_single);
  P_(split_mode); P_(gram_split); P_(overlap); P_(side_streams); P_(gram_ovl); P_(kx_early_on); P_(small_side_on); P_(fused);
  P_(fcols); P_(fused_post); P_(early_pack_on); P_(early_p1_on); P_(early_tail_on); P_(mse_decode_side); P_(mse_small_inline);
  P_(late_mean); P_(planes_mm_on); P_(fwd_x3); P_(p1_behind_pack_on); P_(a2a_overlap); P_(shardable); P_(sharded); P_(world);
  P_(rank); P_(rpr); P_(npad); P_(row0); P_(row1); P_(sgw); P_(fyw);
#undef P_
}

}  // namespace mcgra

using namespace mcgra;

extern "C" int mcgra_attack_plan(const mcgra_attack_config_t* cfg, mcgra_attack_plan_t* out) {
  if (!cfg || !out) { set_error("null argument"); return MCGRA_EINVAL; }
  memset(out, 0, sizeof(*out));
  AttackPlan p;
  const int rc = plan_attack(*cfg, read_plan_env(), &p);
  const bool row_block_refused = rc == MCGRA_ENOSUP && p.why_not_sharded[0];      // (set behind a complete plan only)
  if (rc && !row_block_refused) return rc;
  out->fused = p.fused;
  out->lowrank = p.lr_ok;
  out->product_mode = plan_product_mode(p.split_single, p.gram_split, p.split_mode, p.split_planes);
  out->shardable = p.shardable;
  snprintf(out->why, sizeof(out->why), "%s", p.why_not_sharded);
  plan_text(p, out->text, sizeof(out->text));
  return 0;
}
