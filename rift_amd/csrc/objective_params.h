// The defaults and refusals of RiftObjectiveParams (rift_hip.h), decided on the host before any launch.  Header-only and free of HIP
// types, like eval_params.h, so that a stand-alone program can run it under the host sanitizers (tools/checks/objective_params_check.cpp).
#pragma once
#include <math.h>

#include "../../include/rift_hip.h"

// false: `kind` has no run-time settings (*p untouched)
static inline bool rift_objective_params_set_default(int kind, RiftObjectiveParams* p) {
  if (kind != RIFT_LOSS_RIFT && kind != RIFT_LOSS_GRPO) return false;
  p->clip_low = 0.8; p->clip_high = 1.2;                       // rift_trainer.py:165, grpo_trainer.py:178
  p->dual_clip = kind == RIFT_LOSS_RIFT ? 3.0 : 0.0;           // rift_trainer.py:168-170
  p->kl_beta = kind == RIFT_LOSS_GRPO ? 0.2 : 0.0;             // grpo_trainer.py:182
  p->entropy_coef = 0.0;
  return true;
}

// nullptr: the call is accepted; else the reason, a string literal.  has_ref: in->ref_group_logits != NULL
static inline const char* rift_objective_params_refusal(int kind, const RiftObjectiveParams* p, bool has_ref) {
  if (!p) return "params == NULL";
  if (kind != RIFT_LOSS_RIFT && kind != RIFT_LOSS_GRPO) return "kind has no objective settings (RIFT and GRPO only)";
  const double f[5] = {p->clip_low, p->clip_high, p->dual_clip, p->kl_beta, p->entropy_coef};
  for (int i = 0; i < 5; ++i)
    if (!isfinite(f[i])) return "a field is not finite";
  if (p->clip_low <= 0.0 || p->clip_low > 1.0) return "clip_low outside (0, 1]";
  if (p->clip_high < 1.0) return "clip_high < 1";
  if (p->dual_clip != 0.0 && p->dual_clip <= 1.0) return "dual_clip neither 0 nor > 1";
  if (p->kl_beta < 0.0) return "kl_beta < 0";
  if (p->entropy_coef < 0.0) return "entropy_coef < 0";
  if (p->kl_beta > 0.0 && !has_ref) return "kl_beta > 0 without ref_group_logits";
  return nullptr;
}
