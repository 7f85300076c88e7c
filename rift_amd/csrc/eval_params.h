// The refusals of RiftEvalParams (rift_hip.h), decided on the host before any launch.  Header-only and free of HIP types, so that a
// stand-alone program can run it under the host sanitizers (tools/checks/eval_params_check.cpp).
#pragma once
#include <math.h>

#include "../../include/rift_hip.h"

// nullptr: the parameters are accepted; else the reason, a string literal
static inline const char* rift_eval_params_refusal(const RiftEvalParams* p) {
  if (!p) return "params == NULL";
  if (p->reward_model != RIFT_REWARD_DENSE && p->reward_model != RIFT_REWARD_SPARSE) return "reward_model outside {0, 1}";
  const double f[12] = {p->gamma, p->alpha_collision, p->alpha_boundary, p->alpha_comfort, p->alpha_l_align, p->alpha_vel_align,
                        p->alpha_l_center, p->alpha_center_bias, p->alpha_velocity, p->alpha_timestep, p->bbox_inflation_ratio, p->resolution};
  for (int i = 0; i < 12; ++i)
    if (!isfinite(f[i])) return "a field is not finite";
  if (p->gamma < 0.0) return "gamma < 0";
  if (p->bbox_inflation_ratio <= 0.0) return "bbox_inflation_ratio <= 0";
  if (p->resolution <= 0.0) return "resolution <= 0";
  return nullptr;
}

static inline void rift_eval_params_set_default(RiftEvalParams* p) {
  p->reward_model = RIFT_REWARD_DENSE; p->near_lane_change = 1; p->gamma = 0.98;
  p->alpha_collision = 20.0; p->alpha_boundary = 5.0; p->alpha_comfort = 0.8; p->alpha_l_align = 0.5; p->alpha_vel_align = 0.05;
  p->alpha_l_center = 0.6; p->alpha_center_bias = 0.0; p->alpha_velocity = 0.1; p->alpha_timestep = 0.1;
  p->bbox_inflation_ratio = 1.1; p->resolution = 0.5;
}
