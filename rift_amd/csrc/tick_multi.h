// The rollout tick's per-CBV kernels with the CBV as a second grid dimension (rift_group_advantage_tick, shared.hip): everything of the
// evaluation chain except the candidate rollout itself is independent between the CBVs of a tick, so one launch per STAGE serves all of
// them -- reference-line deviations and neighbour forecasts ahead of the rollouts, kinematics / collision / off-road flags, returns and
// z-scores behind them.  The rollouts stay one launch per CBV: CBV k + 1 starts from the PID state CBV k leaves (the reference shares one
// never-reset controller).  The bodies are the single-CBV kernels' (adv.h, rollout.h), unchanged: same arithmetic, same results.
#pragma once
#include "adv.h"
#include "drivable_map.h"
#include "footprint.h"
#include "offroad_extent.h"
#include "rollout.h"

namespace rift {

#define RIFT_TICK_CHUNK 8                        // CBVs per launch (the descriptors travel as kernel arguments)

struct TickK {                                   // one CBV: inputs and its own slices of the library's scratch
  const float* traj; int G, Tfull, Pmax, N, H, W;
  const float *ref_pos, *ref_ang; const int* ref_len;
  float *dd, *da; int* ci;                       // (G, 40)
  const double* actors; double* ov;              // [actions | speed | location | yaw | extent]; (N, 40, 4, 2)
  RolloutP ro;                                   // rollout outputs (and the closed-loop kernel's own arguments)
  const uint8_t* mask; double ox, oy, ch, sh;    // raster, origin, cos / sin of its heading
  double off_x, off_y;                           // pixel offset of this CBV's raster (the old entry: 200, 200 whatever the raster)
  uint8_t *col, *offr;                           // (G, 40), (G, 80)
  double *ret, *adv;                             // (G): scratch, or the caller's `returns` rows; (G)
  double* terms;                                 // (G, 8) of the caller's `terms`, or NULL
};
struct TickArr {                                 // the evaluator's settings are those of RiftEvalParams (the old entry: the reference's defaults)
  TickK d[RIFT_TICK_CHUNK]; int K, near_lane_change; double gamma, inflation, res;
  RewardP reward; int reward_default;            // reward_default: the weights are the reference's defaults -> the instance that folds them (adv.h)
  DrivableMapDev map; double map_inv_res;        // LAST (the stages before them keep their argument offsets): read by stage 7 only; a CBV uses the map when mask == NULL and H > 0
};
static_assert(sizeof(TickArr) <= 4096, "TickArr travels as a kernel argument");

template <class RP>
__device__ __forceinline__ void tick_return(const TickK& d, double gamma, const RP& rp) {
  constexpr int Ts = 40, TR = RIFT_RO_LEN;
  if (d.terms) rollout_return_body<true>(d.dd, d.da, d.ro.speed, d.ro.acc, d.ro.ang_vel, d.ro.ang_acc, d.col, Ts, d.offr, TR, d.G, Ts, gamma, rp, d.ret, TR, d.terms);
  else rollout_return_body<false>(d.dd, d.da, d.ro.speed, d.ro.acc, d.ro.ang_vel, d.ro.ang_acc, d.col, Ts, d.offr, TR, d.G, Ts, gamma, rp, d.ret, TR, (double*)nullptr);
}

// STAGE 0: reference-line deviations (block 128)   1: neighbour forecast (block 64)   2: kinematics + corners (block 256)
//       3: collision flags (256)   4: off-road flags (256)   5: returns (256)   6: z-score (256)
//       7: off-road flags of a chunk with CBVs that use the drivable-area map (256): launched IN PLACE of stage 4 (riftdm_group_advantage_tick)
//       8: collision flags from the footprints themselves (256; footprint.h): launched IN PLACE of stage 3 (riftfp_group_advantage_tick, FOOTPRINT)
//       9: off-road flags from the centre and the four corners stage 2 wrote (256; offroad_extent.h), masks, the map and "no flags" in one launch
//          as in stage 7: launched IN PLACE of stage 4 / 7 (riftof_group_advantage_tick, FOOTPRINT) on eight times their blocks -- 8 lanes per step
template <int STAGE>
__global__ void tick_multi_kernel(const TickArr a) {
  if ((int)blockIdx.y >= a.K) return;
  const TickK& d = a.d[blockIdx.y];
  constexpr int Ts = 40, M = 12, TR = RIFT_RO_LEN;
  if (STAGE == 0) ref_line_info_body(d.traj, d.G, d.Tfull, Ts, M, d.ref_pos, d.ref_ang, d.ref_len, d.Pmax, d.dd, d.da, d.ci);
  if (STAGE == 1) { if (d.N > 0) { const double* p = d.actors; const size_t N = (size_t)d.N; other_vehicle_rollout_body(p, p + 3 * N, p + 4 * N, p + 7 * N, p + 8 * N, d.N, Ts, a.near_lane_change, a.inflation, d.ov); } }
  if (STAGE == 2) rollout_kinematics_body(d.ro);
  if (STAGE == 3) collision_matrix_body(d.ro.vertices, d.G, TR, d.ov, d.N, Ts, d.col);          // (no neighbours: the loop over them is empty, every flag 0)
  if (STAGE == 8) footprint_collision_body(d.ro.vertices, d.G, TR, d.ov, d.N, Ts, RIFTFP_FOOTPRINT, d.col, (int32_t*)nullptr);
  if (STAGE == 4) {
    if (d.mask) off_road_body(d.ro.center, d.G * TR, d.mask, d.H, d.W, d.ox, d.oy, d.ch, d.sh, a.res, -a.res, d.off_x, d.off_y, d.offr);
    else { const int i = blockIdx.x * 256 + threadIdx.x; if (i < d.G * TR) d.offr[i] = 0; }
  }
  if (STAGE == 7) {
    if (d.mask) off_road_body(d.ro.center, d.G * TR, d.mask, d.H, d.W, d.ox, d.oy, d.ch, d.sh, a.res, -a.res, d.off_x, d.off_y, d.offr);
    else if (d.H > 0) off_road_map_body(d.ro.center, d.G * TR, a.map, RasterPose{d.ox, d.oy, d.ch, d.sh, a.res, d.off_x, d.off_y, a.map_inv_res}, d.H, d.W, d.offr);
    else { const int i = blockIdx.x * 256 + threadIdx.x; if (i < d.G * TR) d.offr[i] = 0; }
  }
  if (STAGE == 9) footprint_off_road_body(d.ro.center, d.ro.vertices, d.G * TR, d.mask, a.map, RasterPose{d.ox, d.oy, d.ch, d.sh, a.res, d.off_x, d.off_y, a.map_inv_res},
                                          d.H, d.W, RIFTOF_FOOTPRINT, d.offr, (uint8_t*)nullptr);
  if (STAGE == 5) {                                // (wave-uniform branches: nothing of the breakdown runs without `terms`)
    if (a.reward_default) tick_return(d, a.gamma, RewardDefaults());
    else tick_return(d, a.gamma, a.reward);
  }
  if (STAGE == 6) group_zscore_body(d.ret, 1, d.G, d.adv);
}

}  // namespace rift
