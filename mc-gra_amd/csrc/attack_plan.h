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

// Every create-time constant of an engine (engine.h describes each where the handle keeps its working copy).
struct AttackPlan {
  int ld = 0, L = 0, Le = 0, C = 0, na = 0, hsum = 0, hmax = 0, fin0 = 1, fin1 = 2;
  int off[MCGRA_MAX_LAYERS + 1] = {0}, wdt[MCGRA_MAX_LAYERS + 1] = {0};
  bool keep_gsym = false, testing = false, fwd_reuse = false, fuse_tail = true;
  bool lr_ok = false;
  int lr_ldv = 0;
  bool split_on = false, split_single = false;
  int split_planes = 3, split_mode = 0;
  bool gram_split = false, overlap = false;
  bool side_streams = false;      // the engine wants the device's shared side streams and its own events
  bool gram_ovl = false, kx_early_on = false, small_side_on = false;
  int fused = FUSED_NONE, fcols = 0;
  char why_not_fused[256] = "";   // fused == FUSED_NONE: the first term of the rule that fails
  bool fused_post = true, early_pack_on = true, early_p1_on = false, early_tail_on = true, mse_decode_side = false,
       mse_small_inline = true;
  bool late_mean = false, planes_mm_on = false, fwd_x3 = false, p1_behind_pack_on = false;
  // row-block ranks.  shardable / why_not_sharded: whether a row-block rank may run this configuration, whatever cfg.shard_world says
  bool shardable = false, sharded = false;
  char why_not_sharded[256] = "";
  int a2a_overlap = 0, world = 1, rank = 0, rpr = 0, npad = 0, row0 = 0, row1 = 0, sgw = 0, fyw = 0;
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
