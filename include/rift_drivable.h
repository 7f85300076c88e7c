/*
 * librift_hip.so -- the drivable-area map: an extension of the C-ABI of include/rift_hip.h with a header and a symbol prefix of its own
 * (`riftdm_`).  rift_hip.h and its `rift_*` symbols are one closed statement (the generated trampolines, the ctypes mirror and the list of
 * exported symbols are derived from it and checked against it); these six entries depend on no MFMA operand format, need no trampoline
 * and are defined once per library (csrc/shared.hip).  Conventions, error codes, RiftCtx, RiftEvalParams and RiftTickCBV are rift_hip.h's.
 */
#ifndef RIFT_DRIVABLE_H
#define RIFT_DRIVABLE_H

#include "rift_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Off-road flags from a device-resident drivable-area map, without a raster.  The drivable polygons of a town are static: they are loaded
 * ONCE and every rollout point is decided against the few polygons near it, so a tick neither draws nor uploads a mask.
 * THE RULE.  Pixel (px, py) of a CBV's (H, W) raster is drivable iff, for some polygon of the map, the pixel centre lies inside or on the
 * boundary of the polygon whose vertices are int32(rint(global_to_pixel(vertex))), global_to_pixel being the reference's
 * (traj_evaluator.py:324-331: fp64, resolution rounded to fp32 first, + (H / 2, W / 2) with the height going to x, as in
 * rift_group_advantage_tick_ex).  Interior: even-odd, half-open in y; boundary inclusive; exact integer arithmetic on the rounded vertices.
 * A ring may repeat its first vertex as its last; a polygon that rounds to a line clears the pixels of that line.  A rollout point is off
 * road iff its pixel (rift_off_road_matrix's arithmetic, bit for bit) lies inside the raster and is not drivable.
 * This is not cv2.fillPoly pixel for pixel: a scanline rasteriser also sets the outline it draws along each edge, up to half a pixel outside
 * the polygon.  Where the two differ the rasteriser says drivable and this rule says off road.  The map is therefore opt-in.
 *
 * vertices: HOST (poly_start[n_polys], 2) f64, global frame; poly_start: HOST (n_polys + 1) i32.  cell: side of a grid cell in metres (16 is
 * a good default); margin: metres by which a polygon's bounding box is inflated for the grid (1.0).  A call with resolution * sqrt(2) >
 * margin is refused: rounding moves a vertex by up to half a pixel per axis.  A second load replaces the first (the old images are released
 * after the stream that last read them has been waited for); the upload is complete when the call returns.  RIFT_ERR_ARG with a message:
 * a polygon with fewer than 3 vertices, a coordinate that is not finite, poly_start not monotone, cell <= 0, margin < 0. */
int riftdm_load(RiftCtx* ctx, const double* vertices, const int32_t* poly_start, int n_polys, double cell, double margin, void* stream);
int riftdm_clear(RiftCtx* ctx);
typedef struct RiftDrivableInfo {
  int32_t n_polys, n_vertices; /* of the loaded map */
  int32_t nx, ny;              /* grid cells */
  int32_t max_cell_list;       /* the longest polygon list of a cell */
  int32_t reserved;
  double  cell, margin;        /* metres */
  double  x0, y0;              /* the grid's lower corner, global frame */
  int64_t device_bytes;        /* held on the device by the map */
} RiftDrivableInfo;            /* 64 bytes */
/* RIFT_ERR_STATE when no map is loaded (as every entry below). */
int riftdm_info(RiftCtx* ctx, RiftDrivableInfo* out);
/* rift_off_road_matrix from the map: the raster (H, W) at origin (ox, oy) and `heading` exists only as a rule.  Of `params` the resolution
 * is read.  RIFT_ERR_ARG, decided before any launch: the faults of RiftEvalParams, H or W <= 0, resolution * sqrt(2) > margin. */
int riftdm_off_road_matrix(RiftCtx* ctx, const float* rollout_center, int n_points, int H, int W, double ox, double oy, double heading,
                             const RiftEvalParams* params, uint8_t* off_road, void* stream);
/* The mask the reference would hand to the lookup, drawn by the rule: mask (H, W) u8 on the DEVICE, 1 = off road, 0 = drivable.
 * rift_off_road_matrix on this mask gives riftdm_off_road_matrix's flags. */
int riftdm_raster(RiftCtx* ctx, int H, int W, double ox, double oy, double heading, const RiftEvalParams* params, uint8_t* mask,
                         void* stream);
/* rift_group_advantage_tick_ex where a CBV may take its off-road flags from the map.  Per RiftTickCBV: off_road_mask == NULL and H > 0 and
 * W > 0 -- from the map, with the CBV's pose, H, W; a mask given -- the raster path, as ever (a tick may mix the two); off_road_mask == NULL
 * and H == 0 -- no off-road flags.  The launches are those of rift_group_advantage_tick_ex, one off-road launch per chunk.  RIFT_ERR_STATE
 * when a CBV asks for the map and none is loaded; RIFT_ERR_ARG for resolution * sqrt(2) > margin, for H or W < 0 or only one of them 0 with
 * a NULL mask, and for the faults of rift_group_advantage_tick_ex -- all decided before any launch. */
int riftdm_group_advantage_tick(RiftCtx* ctx, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                  float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                  const RiftEvalParams* params, double* advantage, double* returns, double* terms, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RIFT_DRIVABLE_H */
