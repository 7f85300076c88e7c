// Off-road flags for the whole footprint (include/rift_offroad.h states THE RULE; the host statement is
// rift_amd/planning/fine_tuner/rlft/traj_eval/offroad_extent.py): the centre of a rollout step and its four corners, each decided by the point
// rule of its source -- off_road_pixel + off_road_mask_flag (adv.h) for a raster, off_road_pixel + off_road_map_flag (drivable_map.h) for the
// loaded map; nothing of either is restated here.
// The map's lookup walks a cell's polygons and their vertices and diverges between points, so the five points of a step are not run one
// after the other in one thread: each has a lane of its own.  A step owns one aligned group of 8 lanes -- lane 0 the centre, lanes 1 to 4
// the corners, lanes 5 to 7 idle -- and a block of 256 threads holds 32 steps.  The five flags meet in one wave-wide ballot (no LDS, no
// atomics; lanes that are idle or past the end vote 0), of which lane 0 of the group takes its group's byte and writes `out` and `which`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rift_offroad.h"
#include "adv.h"
#include "drivable_map.h"

namespace rift {

// mask: the raster source; mask == NULL and H > 0: the map m; mask == NULL and H == 0: no flags (zeros).  q: the raster's pose for either
// source (res_x = q.res, res_y = -q.res).  vertices is read under FOOTPRINT only; which: NULL or (n_points).
__device__ __forceinline__ void footprint_off_road_body(const float* __restrict__ center /*(n,2)*/, const float* __restrict__ vertices /*(n,4,2)*/,
                                                        int n_points, const uint8_t* __restrict__ mask, const DrivableMapDev& m, const RasterPose& q,
                                                        int H, int W, int extent, uint8_t* __restrict__ out, uint8_t* __restrict__ which) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) >> 3;      // the step
  const int k = threadIdx.x & 7;                                              // the point of the step
  const bool live = i < n_points && (k == 0 || (k < 5 && extent == RIFTOF_FOOTPRINT)) && (mask != nullptr || H > 0);
  bool off = false;
  if (live) {
    const float* p = k == 0 ? center + 2 * i : vertices + 8 * i + 2 * (k - 1);
    double px, py;
    off_road_pixel((double)p[0], (double)p[1], q.ox, q.oy, q.c, q.s, q.res, -q.res, q.off_x, q.off_y, px, py);
    off = (mask ? off_road_mask_flag(px, py, mask, H, W) : off_road_map_flag(px, py, m, q, H, W)) != 0;      // (wave-uniform per CBV)
  }
  const unsigned long long votes = __ballot(off);                             // every lane of the wave arrives here
  if (k == 0 && i < n_points) {
    const unsigned bits = (unsigned)(votes >> (threadIdx.x & 56)) & 0x1fu;    // the group's five flags: bit k = point k
    out[i] = bits != 0;
    if (which) which[i] = (uint8_t)bits;
  }
}
__global__ __launch_bounds__(256) void footprint_off_road_kernel(const float* __restrict__ center, const float* __restrict__ vertices, int n_points,
                                                                 const uint8_t* __restrict__ mask, const DrivableMapDev m, const RasterPose q, int H, int W,
                                                                 int extent, uint8_t* __restrict__ out, uint8_t* __restrict__ which) {
  footprint_off_road_body(center, vertices, n_points, mask, m, q, H, W, extent, out, which);
}

}  // namespace rift
