"""The host statement of the off-road rule of include/rift_offroad.h: THE RULE of that header in numpy.  The kernel
(csrc/offroad_extent.h) is held to this file bit for bit (tests/test_gpu_offroad_extent.py).

    off_road_extent(center (..., 2), vertices (..., 4, 2), point_rule, extent) -> (flags (...) bool, which (...) uint8)

For one rollout step the five tested points are, in this order: point 0, the centre; points 1 to 4, the vertices 0 to 3.  All are fp32 and
are widened to fp64 by the point rule.  `point_rule` decides each point by the existing rule of its source -- points (..., 2) float32 ->
bool (...), 1 = off road; a point whose pixel falls outside the raster is not off road:

    raster_point_rule(mask, pose, res)                  rift_off_road_matrix's arithmetic: the pixel is rint(global_to_pixel(p)), off road iff
                                                        it lies inside (H, W) and mask[py][px] == 1
    the map source                                      the rule of include/rift_drivable.h; its numpy statement is the tests' (tests/drivable_cases.py)

extent "center": the flag is point 0's (today's flags); "footprint": the flag is the OR of the five points' flags, so a footprint flag is
never below the centre flag.  which: bit k is set iff point k is off road; under "center" only bit 0 can be set.
The rule samples five points; it does not test the footprint's area.
"""
import math

import numpy as np

EXTENTS = ("center", "footprint")


def raster_point_rule(mask, pose, res: float = 0.5):
    """The point rule of the raster source: mask (H, W) uint8 with 1 = off road, pose (x, y, heading) of the raster's centre, res metres per
    pixel (rounded to fp32, as the reference's resolution_hw).  The pixel offsets are (H / 2, W / 2) as fp32, the height going to x."""
    mask = np.asarray(mask)
    H, W = mask.shape
    ox, oy, c, s = float(pose[0]), float(pose[1]), math.cos(float(pose[2])), math.sin(float(pose[2]))
    r, off_x, off_y = float(np.float32(res)), float(np.float32(H / 2)), float(np.float32(W / 2))

    def rule(points):
        p = np.asarray(points, dtype=np.float32).astype(np.float64)              # widened: exact
        dx, dy = p[..., 0] - ox, p[..., 1] - oy
        lx, ly = dx * c + dy * s, dx * (-s) + dy * c                             # products and sums rounded one by one (numpy does not contract)
        px, py = np.rint(lx / r + off_x), np.rint(ly / (-r) + off_y)
        inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        out = np.zeros(p.shape[:-1], dtype=np.bool_)
        out[inside] = mask[py[inside].astype(np.int64), px[inside].astype(np.int64)] == 1
        return out

    return rule


def off_road_extent(center, vertices, point_rule, extent: str = "footprint"):
    """center (..., 2) fp32, vertices (..., 4, 2) fp32 (not read under "center": may be None) -> (flags (...) bool, which (...) uint8)."""
    if extent not in EXTENTS:
        raise ValueError(f"off_road: extent = {extent!r}; known: {list(EXTENTS)}")
    center = np.asarray(center, dtype=np.float32)
    which = np.asarray(point_rule(center), dtype=np.bool_).astype(np.uint8)      # bit 0: the centre
    if extent == "footprint":
        vertices = np.asarray(vertices, dtype=np.float32)
        assert vertices.shape == center.shape[:-1] + (4, 2)
        for k in range(4):                                                       # bits 1 to 4: the vertices in their order
            which |= np.asarray(point_rule(vertices[..., k, :]), dtype=np.bool_).astype(np.uint8) << np.uint8(k + 1)
    return which != 0, which
