/*
 * librift_hip.so -- off-road flags for the whole footprint, chosen at run time: an extension of the C-ABI of include/rift_hip.h with a
 * header and a symbol prefix of its own (`riftof_`), layered as include/rift_footprint.h, include/rift_select.h, include/rift_advantage.h and
 * include/rift_drivable.h are.  The three entries depend on no MFMA operand format, need no trampoline and are defined once per library
 * (csrc/shared.hip; the kernel in csrc/offroad_extent.h, defaults and refusals in csrc/offroad_params.h).  Conventions, error codes, RiftCtx,
 * RiftEvalParams and RiftTickCBV are rift_hip.h's; RiftCollisionParams is rift_footprint.h's.
 */
#ifndef RIFT_OFFROAD_H
#define RIFT_OFFROAD_H

#include "rift_footprint.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RIFTOF_CENTER = 0, RIFTOF_FOOTPRINT = 1 };
typedef struct RiftOffRoadParams {
  int32_t extent, reserved;   /* reserved: 0 */
} RiftOffRoadParams;          /* 8 bytes */

/* CENTER, 0: the flags of rift_off_road_matrix / riftdm_off_road_matrix.  No context, no device. */
int riftof_params_default(RiftOffRoadParams* out);

/* The off-road flag of every rollout step from the step's footprint centre alone (CENTER: the reference's flag) or from the centre and the
 * four corners of the footprint (FOOTPRINT), against a raster (`mask`) or against the loaded drivable-area map (mask == NULL).
 * THE RULE.  The host statement (off_road_extent, rift_amd/planning/fine_tuner/rlft/traj_eval/offroad_extent.py) and the kernel
 * (csrc/offroad_extent.h) implement this text.
 *   For one rollout step the five tested points are, in this order:
 *     point 0: the centre, center[g][t]
 *     points 1 to 4: the vertices vertices[g][t][0..3]
 *   All are fp32 and are widened to fp64.
 *   Each point is decided by the existing point rule of its source, bit for bit:
 *     Raster source: rift_off_road_matrix's arithmetic (off_road_body, adv.h).  The pixel is rint(global_to_pixel(p)).  The point is off road
 *       iff the pixel lies inside (H, W) and mask[py][px] == 1.
 *     Map source: off_road_map_body / pixel_drivable (csrc/drivable_map.h; include/rift_drivable.h states that rule), unchanged.
 *   A point whose pixel falls outside the raster is not off road, as today.
 *     CENTER (0): the flag is point 0's.  These are today's flags.
 *     FOOTPRINT (1): the flag is the OR of the five points' flags.
 *   A FOOTPRINT flag is therefore never below the CENTER flag, by construction and not only up to rounding.
 *   Optional second output which[g][t] (u8): bit k is set iff point k is off road.  Under CENTER only bit 0 can be set.
 * The rule samples five points.  It does not test the footprint's area: a kerb spike narrower than the car between two corners is not seen.
 * It is not the reference's rule either (centre only); FOOTPRINT is therefore opt-in.
 *
 * center: DEVICE (n, 2) f32; vertices: DEVICE (n, 4, 2) f32, or NULL under CENTER without `which`; mask: DEVICE (H, W) u8 with 1 = off road,
 * or NULL: the loaded map (RIFT_ERR_STATE if none is loaded), (H, W) then being the raster the rule speaks of; ox, oy, heading: the pose of the
 * raster's centre; params: its resolution is read (rounded to fp32, as the reference's resolution_hw); the pixel offsets are (H / 2, W / 2),
 * the height going to x, as in riftdm_off_road_matrix; off_road: DEVICE (n) u8; which: DEVICE (n) u8, or NULL.
 * CENTER with which == NULL launches the existing kernel of the source (off_road_kernel / off_road_map_kernel) under its existing label and
 * gives its bits; every other combination launches footprint_off_road_kernel: eight lanes per step, one tested point per lane, three idle.
 * RIFT_ERR_ARG with a message (rift_last_error), decided on the host before any launch and ahead of the wrapped entry's own refusals, which
 * apply unchanged: offroad == NULL; extent outside {CENTER, FOOTPRINT}; reserved != 0; vertices == NULL under FOOTPRINT, or with `which`
 * given. */
int riftof_off_road_matrix(RiftCtx* ctx, const float* center, const float* vertices, int n, const uint8_t* mask, int H, int W, double ox,
                           double oy, double heading, const RiftEvalParams* params, const RiftOffRoadParams* offroad, uint8_t* off_road,
                           uint8_t* which, void* stream);

/* riftfp_group_advantage_tick with the off-road flags under `offroad`.  Every other argument means what it means there, per CBV the source
 * is chosen as it is there -- a CBV with a mask uses the raster, one with mask == NULL and H > 0 the loaded map, one with mask == NULL and
 * H == 0 gets no flags -- and the refusals of that entry apply unchanged, behind those of `offroad` (offroad == NULL; extent outside the
 * enumeration; reserved != 0).  CENTER issues exactly the launches of riftfp_group_advantage_tick and gives its bits.  FOOTPRINT launches
 * stage 9 of the tick (tick_multi_kernel_9: THE RULE above on the corners stage 2 wrote, eight lanes per candidate and step) IN PLACE of
 * stage 4 / 7 and composes freely with both collision modes; everything behind the flags -- returns, terms, z-score -- is untouched. */
int riftof_group_advantage_tick(RiftCtx* ctx, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                const RiftEvalParams* params, const RiftCollisionParams* collision, const RiftOffRoadParams* offroad,
                                double* advantage, double* returns, double* terms, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RIFT_OFFROAD_H */
