// The run-time choice of the executed candidate (include/rift_select.h states the rule): the host half -- defaults and refusals, free of HIP
// types, so that a stand-alone program built by a plain C++ compiler can run it (tests/test_select_abi_host.py).  The stage itself is part
// of control_tick_kernel (control.h).
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/rift_select.h"

static inline void riftcs_params_set_default(RiftSelectParams* p) {
  p->mode = RIFTCS_GREEDY; p->reserved = 0; p->temperature = 1.0;
}

// nullptr: the call is accepted; else the reason, a string literal.  Everything riftcs_control_tick refuses on top of rift_control_tick's own
// refusals, ahead of any launch.
static inline const char* riftcs_refusal(const RiftSelectParams* p, const double* u, int K) {
  if (!p) return "params == NULL";
  if (p->mode < RIFTCS_GREEDY || p->mode > RIFTCS_SAMPLE) return "mode outside {0, 1}";
  if (p->reserved != 0) return "reserved != 0";
  if (!isfinite(p->temperature) || p->temperature <= 0.0) return "temperature not finite or <= 0";
  if (p->mode == RIFTCS_SAMPLE) {
    if (K > 0 && !u) return "u == NULL in SAMPLE";
    for (int k = 0; k < K; ++k)
      if (!(u[k] >= 0.0 && u[k] < 1.0)) return "u[k] NaN or outside [0, 1)";
  }
  return nullptr;
}

// The reciprocal both sides multiply by: formed in fp64, rounded to fp32 once (kept finite: 0 * r is the top candidate's exponent).
static inline float riftcs_inv_temperature(const RiftSelectParams* p) { return (float)fmin(1.0 / p->temperature, 3.4028234663852886e38); }
