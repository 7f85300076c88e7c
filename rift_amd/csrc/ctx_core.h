// The half of an engine context that is no build parameter: what the operand-format-free entries (shared.hip), the launch bookkeeping
// (launch.h) and the routing of the exported trampolines (abi.cpp) need.  Defined ONCE for the library; each engine build (engine.hip, one
// per MFMA operand format) derives its full context from it inside its own namespace (rift_bf::Ctx / rift_hf::Ctx : RiftCtx), so the two
// builds' context types cannot collide.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <set>
#include <string>
#include <vector>

#include "../../include/rift_hip.h"
#include "devmem.h"
#include "drivable_grid.h"

struct RiftCtxCore {
  int opfmt = 0;                         // FIRST member (set by rift_ctx_create of the build): abi.cpp reads it to route a call to the build (bf16 / fp16 operands) that owns the context
  int device = 0;
  std::string err;
  hipStream_t stream = nullptr;
  bool dry = false;
  // optional per-launch HIP-event profiling (bench roofline leg; off on the timed path)
  bool prof_on = false; double prof_flops = 0.0; bool prof_shapes = false;
  std::set<std::string> prof_names;
  std::vector<hipEvent_t> prof_pool; size_t prof_used = 0;
  struct Rec { const char* label; hipEvent_t e0, e1; double flops; };
  std::vector<Rec> prof_recs;
  int poison_lds = -1;                   // RIFT_POISON_LDS diagnostic (see lds_poison_kernel)
  struct { std::string delay_label; long long delay_ticks = 0; } dg;      // RIFT_DELAY diagnostic (see delay_kernel)
  struct PiHead { const float *w0 = nullptr, *b0 = nullptr, *ln_g = nullptr, *ln_b = nullptr, *w3 = nullptr, *b3 = nullptr; } pi;   // planning_decoder.pi_head.mlp.{0,1,3}: the trainable tensors, read LIVE through these pointers (resolved at load)
  bool loaded = false;
  // state of the last forward, consumed by rift_loss_backward
  float* last_qfinal = nullptr; float* last_hpi = nullptr; float* last_prob = nullptr;
  uint8_t* last_rkpm = nullptr; int last_bs = 0, last_R = 0;
  // loss scratch
  DevBuf<double> l_S, l_cnt; DevBuf<float> l_dz, l_partial;
  DevBuf<double> l_T;      // [bs][LOSS_NTERM] per-scene term sums of rift_loss_backward_ex, reserved when its `terms` are asked for
  DevBuf<double> l_sink;   // [2] where loss_reduce_kernel's objective sums go when there is no objective (rift_head_backward)
  DevBuf<double> clip_part;
  DevBuf<float> cr_buf; DevBuf<double> cr_part;   // PPO critic scratch (rows x 1153 floats)
  bool ro8 = true;                  // candidate rollout with eight lanes per candidate (rollout.h; RIFT_RO8=0: one lane, the round-1 form)
  DevBuf<float> ro_raw;             // rift_rollout: the unsmoothed speed history handed from the closed-loop kernel to the kinematics kernel
  DevBuf<char> tick_scratch;        // rift_group_advantage_tick: per-CBV intermediates (reused CBV by CBV in stream order)
  // riftdm_load: the town's drivable polygons and their grid (drivable_grid.h).  `grid` keeps the host-side numbers only (its vectors
  // are emptied after the upload); used_on: the stream of the last launch that read the images -- waited for before they are released
  struct DMap { bool loaded = false; DrivableGrid grid; DrivableImages img; hipStream_t used_on = nullptr; bool used = false; } dmap;
  DevBuf<double> ga_scratch;        // riftga_arena_advantage: per-scene partials and the arena's totals (adv_params.h), handed from launch to launch
};

// The C handle of include/rift_hip.h.  It adds nothing: a build's context derives from it and its entries cast down once at the top.
struct RiftCtx : RiftCtxCore {};
