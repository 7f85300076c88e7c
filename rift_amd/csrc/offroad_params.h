// The run-time choice of the off-road flag's extent (include/rift_offroad.h states the rule): the host half -- defaults and refusals, free of
// HIP types, so that a stand-alone program built by a plain C++ compiler can run it (tests/test_offroad_abi_host.py).  The lookup itself is
// footprint_off_road_body (offroad_extent.h).
#pragma once
#include <stddef.h>

#include "../../include/rift_offroad.h"

static inline void riftof_params_set_default(RiftOffRoadParams* p) {
  p->extent = RIFTOF_CENTER; p->reserved = 0;
}

// nullptr: the call is accepted; else the reason, a string literal.  Everything the riftof_ entries refuse on top of the wrapped entry's own
// refusals, ahead of any launch.
static inline const char* riftof_refusal(const RiftOffRoadParams* p) {
  if (!p) return "offroad params == NULL";
  if (p->extent < RIFTOF_CENTER || p->extent > RIFTOF_FOOTPRINT) return "off-road extent outside {0, 1}";
  if (p->reserved != 0) return "offroad reserved != 0";
  return nullptr;
}

// riftof_off_road_matrix on top of that: the corners are read under FOOTPRINT, and `which` speaks of them
static inline const char* riftof_matrix_refusal(const RiftOffRoadParams* p, const float* vertices, const uint8_t* which) {
  if (const char* why = riftof_refusal(p)) return why;
  if (!vertices && p->extent == RIFTOF_FOOTPRINT) return "vertices == NULL under FOOTPRINT";
  if (!vertices && which) return "vertices == NULL with which given";
  return nullptr;
}
