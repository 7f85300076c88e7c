// The run-time choice of the collision test (include/rift_footprint.h states the rule): the host half -- defaults and refusals, free of HIP
// types, so that a stand-alone program built by a plain C++ compiler can run it (tests/test_footprint_abi_host.py).  The test itself is
// footprint_collision_body (footprint.h).
#pragma once
#include <stddef.h>

#include "../../include/rift_footprint.h"

static inline void riftfp_params_set_default(RiftCollisionParams* p) {
  p->mode = RIFTFP_ENVELOPE; p->reserved = 0;
}

// nullptr: the call is accepted; else the reason, a string literal.  Everything the riftfp_ entries refuse on top of the wrapped entry's own
// refusals, ahead of any launch.
static inline const char* riftfp_refusal(const RiftCollisionParams* p) {
  if (!p) return "collision params == NULL";
  if (p->mode < RIFTFP_ENVELOPE || p->mode > RIFTFP_FOOTPRINT) return "collision mode outside {0, 1}";
  if (p->reserved != 0) return "collision reserved != 0";
  return nullptr;
}
