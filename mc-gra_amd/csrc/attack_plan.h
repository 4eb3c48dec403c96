// Which code an attack engine runs, decided from (configuration, environment) alone: plan_attack makes no HIP call and no
// allocation, so the decision can be read and tested without a device (mcgra_attack_plan, include/mcgra.h).
// mcgra_attack_create (attack.hip) plans, then allocates what the plan asks for, then makes its streams.
#pragma once
#include <stdint.h>

#include "../../include/mcgra.h"

namespace mcgra {

// Every environment switch of create, read once.  -1: unset (or an A/B switch without MCGRA_AB=1), else the value's first
// character (0: set but empty).
struct PlanEnv {
  int split_bf16 = -1, testing = -1;      // MCGRA_SPLIT_BF16, MCGRA_TESTING: honoured as they stand
  // the A/B switches of the parity suite and of the measurements under profiles/ (INTEGRATION.md section 5): MCGRA_<NAME>
  int keep_gsym = -1, no_fwd_reuse = -1, no_fused_tail = -1, no_lowrank = -1, gram_split = -1, overlap = -1, gram_overlap = -1,
      gram_kx_early = -1, small_side = -1, no_fused_lr = -1, no_fused_post = -1, early_pack = -1, early_p1 = -1, early_tail = -1,
      mse_decode_side = -1, mse_small_inline = -1, planes_mm = -1, fwd_x3 = -1, p1_behind_pack = -1, a2a_overlap = -1;
};

enum FusedKind { FUSED_NONE = 0, FUSED_HSIC = 1, FUSED_MSE = 2, FUSED_KL = 3 };

// Every create-time constant of an engine.  The engine holds ONE constant copy (engine.h: mcgra_attack::p) and every step reads it
// there; the in-class values below are what plan_attack starts from, never what an engine runs on.  Six of the switches are off
// while the graph in place has a non-zero ori_adj: they are read through the predicates of engine.h (lr_ok(h), ...), marked [ori].
struct AttackPlan {
  int n = 0, ld = 0, L = 0, Le = 0, C = 0, na = 0, hsum = 0, hmax = 0, fin0 = 1, fin1 = 2;      // n = cfg.n; ld: leading dimension of the N x N buffers
  int off[MCGRA_MAX_LAYERS + 1] = {0};   // column offset of layer l inside the concatenated node buffers
  int wdt[MCGRA_MAX_LAYERS + 1] = {0};   // width of layer l output (dims[l+1])
  bool keep_gsym = false;          // MCGRA_KEEP_GSYM=1: keep the mirrored packed gradient of each step readable as "G_sym" (parity tests)
  bool testing = false;            // MCGRA_TESTING=1 at create: mcgra_attack_test_mutate is accepted (refused otherwise)
  // The monitoring forward of :290-296 (victim on the updated adjacency) is exactly the first forward of the next
  // iteration (:164-167) when eps == 0: mcgra_attack_monitor leaves its adj_norm, degree vectors, chain and
  // log-probs in place and the next step adopts them instead of recomputing (bit-identical, one N x N pass and two
  // skinny products less per step).  MCGRA_NO_FWD_REUSE=1 disables.
  bool fwd_reuse = false;          // [ori] (the adoption itself: Carry::fwd_cached)
  bool fuse_tail = true;           // apply + rank-k + mirror + Adam in one kernel (MCGRA_NO_FUSED_TAIL=1: separate kernels)
  // low-rank linear_HSIC(adj_norm, modified_adj1) (lowrank_kernels.hip); MCGRA_NO_LOWRANK=1 disables
  bool lr_ok = false;              // [ori] configuration allows it (HSIC, ReLU embedding, width <= 32)
  int lr_ldv = 0;
  // P1 through the split kernel of split_symm_bf16.hip instead of the fp32 MFMA SYMM
  bool split_on = false;
  bool split_single = false;       // MCGRA_SPLIT_BF16=1 (by name only, never a default): P1 as the single-plane product x0 y0 of the fp16 x 2 operands
  int split_planes = 3;            // 3: bf16 x 3 (six products); 2: fp16 x 2 (three products, operand scales from amax)
  int split_mode = 0;              // 0: fp32 MFMA SYMM; 2: split3_symm_kernel on packed planes
  // Gram evaluation (masked / GAT / MCGRA_NO_LOWRANK steps) through the same kernel: planes of Xc, Yc, the combined
  // Grams and Yc^T; amax[2] = max |Yc|, [3] = max |2 (s1 Kfc + s2 Kyc)|, [4] = max |2 s2 Kxc|, [8..15] = the
  // (A, B) scale pairs of the four products
  bool gram_split = false;         // [ori]
  bool overlap = false;            // MCGRA_OVERLAP=1 forks the N x N x N product onto the engine's own stream
  bool side_streams = false;       // the engine wants the device's shared side streams and its own events
  bool gram_ovl = false;           // the Gram evaluation's four products on the side stream, beside the rest of the step (MCGRA_GRAM_OVERLAP=0: caller's stream)
  // a configuration whose every step is a Gram evaluation (no low-rank form): the first product, Kx = Xc Xc^T, needs adj_norm of the
  // CURRENT M only -- the monitoring forward forks pack + Kx as soon as adj_norm stands, and the next step finds them in flight
  bool kx_early_on = false;        // (MCGRA_GRAM_KX_EARLY=0: the step packs and forks Kx itself, as in round 5)
  bool small_side_on = false;      // general step: the small-operand terms c9 / c10 (~20 tiny launches) on the third stream, beside the decode and the N x N passes (MCGRA_SMALL_SIDE=0: caller's stream)
  // fused low-rank step (attack_fused.hip): everything N x N from M and n-vectors; MCGRA_NO_FUSED_LR=1 disables
  int fused = FUSED_NONE;          // [ori: fused_ok(h)] which fused step the configuration allows: HSIC; MSELoss (calc = MSELoss: no product, no low-rank
                                   //   factors); KL (calc = calc_kl: the MSELoss step's data flow + per-row softmax statistics)
  // an elementwise measure: every branch of the MSELoss step that is not MSELoss' own arithmetic
  bool elementwise() const { return fused == FUSED_MSE || fused == FUSED_KL; }
  bool kl() const { return fused == FUSED_KL; }
  int fcols = 0;                   // leading dimension of FV / FY
  char why_not_fused[256] = "";    // fused == FUSED_NONE: the first term of the rule that fails
  bool fused_post = true;          // forward: post pass + next layer's T / heads in one launch (MCGRA_NO_FUSED_POST=1: separate kernels)
  // early pack (attack_fused.hip): the planes of the product's operand are packed on the product's stream as soon as r is
  // known, beside the forward's two products on the caller's stream (ev_r: r ready; ev_pack: planes and row partials ready)
  bool early_pack_on = true;       // MCGRA_EARLY_PACK=0 disables (A/B)
  bool early_p1_on = false;        // row-block rank: pack (uncentred) + N x N x N product forked by the FORWARD, as soon as r is complete
  // monolithic, n >= 8192: the product is cut behind whole rounds of the chip that cover the first `tail_rows` rows of P1 (both
  // orientations); the tail's first pass over those rows runs beside the product's last rounds (MCGRA_EARLY_TAIL=0 disables)
  bool early_tail_on = true;
  bool mse_decode_side = false;    // fused MSELoss / KL step on a small graph: the decode on the fourth stream as in the HSIC step (MCGRA_MSE_DECODE_SIDE=1; A/B)
  bool mse_small_inline = true;    // fused MSELoss step on a small graph: the two one-launch small-operand terms on the caller's stream (MCGRA_MSE_SMALL_INLINE=0: third stream; A/B)
  // Monolithic fused step: the column means of adj_norm come out of the PACK of the product's operand (row sums of the
  // packed values) instead of out of a 33rd column (M r) of the first forward product; the product's operand is then
  // packed uncentred -- (H Kf H) 1 = 0, so P1 is the same up to 1e-7 -- and the means are only needed behind the pack.
  bool late_mean = false;          // [ori]
  // ... and with uncentred planes of the CURRENT M in Bpack (between the pack of a step and its Adam pass) the skinny
  // products on M that run beside the N x N x N product read those planes (planes_mm.hip).  MCGRA_PLANES_MM=0 disables.
  bool planes_mm_on = false;       // [ori] (the planes' validity: StepScratch::planes_valid)
  // Monolithic fused step with the early pack: the forward's two skinny products on the bf16x3 kernel whose blocks fit beside a
  // product block (skinny_x3.hip; MCGRA_FWD_X3=0 / 1: gemm_f32 / forced on), and the product forked behind the pack on its own
  // stream instead of behind the forward (MCGRA_P1_BEHIND_PACK=0 / 1; A/B).  Both default on from n = 8192.
  bool fwd_x3 = false, p1_behind_pack_on = false;
  // row-block ranks.  shardable / why_not_sharded: whether a row-block rank may run this configuration, whatever cfg.shard_world says
  bool shardable = false, sharded = false;
  char why_not_sharded[256] = "";
  // row-block sharding (mcgra_attack_shard_*): this rank owns rows [row0, row1) of M / am / av
  int world = 1, rank = 0, rpr = 0, npad = 0, row0 = 0, row1 = 0;
  int sgw = 0, fyw = 0;            // row widths (floats, even) of the narrow / wide exchanged node arrays
  // the product computes the row panels of the peers first and the own ones last; ev_first is recorded behind the first part, the
  // P1 all-to-all then runs beside the second (attack_fused.hip; MCGRA_A2A_OVERLAP=0 / 1 forces off / on)
  int a2a_overlap = 0;             // 0: the product in one piece; 1: cut where it is free or cheap (default); 2: always (MCGRA_A2A_OVERLAP=1)
};

PlanEnv read_plan_env();      // getenv only (an A/B switch set without MCGRA_AB=1 is ignored, and said so once per process)

// 0, or MCGRA_EINVAL / MCGRA_ENOSUP with the reason in mcgra_last_error.  A row-block rank (cfg.shard_world > 0) of a
// configuration that is not shardable is refused with MCGRA_ENOSUP behind a COMPLETE plan (p->shardable == false tells it apart).
int plan_attack(const mcgra_attack_config_t& cfg, const PlanEnv& env, AttackPlan* p);

// mcgra_attack_product_mode (include/mcgra.h) of these flags
inline int plan_product_mode(bool split_single, bool gram_split, int split_mode, int split_planes) {
  if (split_single && (gram_split || (split_mode == 2 && split_planes == 2))) return 1;
  return split_mode == 2 && split_planes == 2 ? 3 : split_mode;
}

}  // namespace mcgra
