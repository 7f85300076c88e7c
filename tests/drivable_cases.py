"""The drivable-area rule of include/rift_drivable.h (riftdm_load) restated in numpy, brute force: every polygon is tested against every
pixel of its rounded bounding box, with no grid and no culling -- so the device's grid, margin and box test are checked by it, not shared
with it.  Also: the grid's cell lists restated (for the host test of csrc/drivable_grid.h) and the seeded cases of the tests.

The rule: pixel (px, py) of an (H, W) raster is drivable iff for some polygon the pixel centre lies inside or on the boundary of the polygon
with the vertices int32(rint(global_to_pixel(vertex))); interior even-odd and half-open in y, boundary inclusive, integer arithmetic.
"""
import math

import numpy as np


def global_to_pixel(points, pose, res, H, W):
    """The reference's global_to_pixel (traj_evaluator.py:324-327) in fp64, products and sums as separate roundings: (n, 2) -> (n, 2) pixel
    coordinates (x, y); resolution_hw and the offset (H / 2, W / 2) are float32 arrays there -- the height goes to x."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    c, s = math.cos(float(pose[2])), math.sin(float(pose[2]))
    dx, dy = p[:, 0] - float(pose[0]), p[:, 1] - float(pose[1])
    lx = dx * c + dy * s
    ly = dx * (-s) + dy * c
    r = float(np.float32(res))
    return np.stack([lx / r + float(np.float32(H / 2)), ly / (-r) + float(np.float32(W / 2))], -1)


def rounded_vertices(poly, pose, res, H, W):
    """(n, 2) int64 pixel vertices of one polygon: np.round is half to even, as rint."""
    return np.round(global_to_pixel(poly, pose, res, H, W)).astype(np.int32).astype(np.int64)


def polygon_covers(v, X, Y):
    """Inside-or-on-boundary of the integer polygon v (n, 2) for integer point arrays X, Y (any shape): bool array."""
    inside = np.zeros(X.shape, dtype=np.bool_)
    on = np.zeros(X.shape, dtype=np.bool_)
    ax, ay = int(v[-1, 0]), int(v[-1, 1])
    for bx, by in ((int(q[0]), int(q[1])) for q in v):
        ex, ey = bx - ax, by - ay
        cross = ex * (Y - ay) - ey * (X - ax)
        on |= (cross == 0) & (X >= min(ax, bx)) & (X <= max(ax, bx)) & (Y >= min(ay, by)) & (Y <= max(ay, by))
        if ey != 0:                                   # half-open in y: the edge owns its lower end, not its upper one
            straddle = (ay > Y) != (by > Y)
            inside ^= straddle & ((cross > 0) if ey > 0 else (cross < 0))      # the crossing lies to the right of the centre
        ax, ay = bx, by
    return inside | on


def off_road_mask(polygons, pose, res=0.5, H=400, W=400):
    """(H, W) uint8, 1 = off road, 0 = drivable: the mask riftdm_raster draws."""
    mask = np.ones((H, W), dtype=np.uint8)
    for poly in polygons:
        v = rounded_vertices(poly, pose, res, H, W)
        x0, x1 = max(int(v[:, 0].min()), 0), min(int(v[:, 0].max()), W - 1)
        y0, y1 = max(int(v[:, 1].min()), 0), min(int(v[:, 1].max()), H - 1)
        if x0 > x1 or y0 > y1:
            continue
        X, Y = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.int64), np.arange(y0, y1 + 1, dtype=np.int64))
        mask[y0:y1 + 1, x0:x1 + 1][polygon_covers(v, X, Y)] = 0
    return mask


def point_pixels(points, pose, res, H, W):
    """The lookup's pixel of every rollout point (float32 in, fp64 arithmetic): (n, 2) int64 and the inside-the-raster flags."""
    px = np.round(global_to_pixel(np.asarray(points, dtype=np.float32).astype(np.float64), pose, res, H, W))
    valid = (px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)
    return px.astype(np.int64), valid


def off_road_flags(points, polygons, pose, res=0.5, H=400, W=400, mask=None):
    """get_off_road_matrix on the rule's mask: points (..., 2) float32 -> bool of the leading shape.  Outside the raster: not off road."""
    pts = np.asarray(points, dtype=np.float32)
    mask = off_road_mask(polygons, pose, res, H, W) if mask is None else mask
    px, valid = point_pixels(pts.reshape(-1, 2), pose, res, H, W)
    out = np.zeros(px.shape[0], dtype=np.bool_)
    out[valid] = mask[px[valid, 1], px[valid, 0]] == 1
    return out.reshape(pts.shape[:-1])


def edge_distance(polygons, pose, res, H, W, reach=2):
    """(H, W) float64: distance in pixels of every pixel centre to the nearest rounded edge, exact up to `reach` (beyond it: inf)."""
    dist = np.full((H, W), np.inf)
    for poly in polygons:
        v = rounded_vertices(poly, pose, res, H, W).astype(np.float64)
        a = v[-1]
        for b in v:
            x0, x1 = max(int(min(a[0], b[0])) - reach, 0), min(int(max(a[0], b[0])) + reach, W - 1)
            y0, y1 = max(int(min(a[1], b[1])) - reach, 0), min(int(max(a[1], b[1])) + reach, H - 1)
            if x0 <= x1 and y0 <= y1:
                X, Y = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.float64), np.arange(y0, y1 + 1, dtype=np.float64))
                e = b - a
                L2 = float(e @ e)
                t = np.clip(((X - a[0]) * e[0] + (Y - a[1]) * e[1]) / L2, 0.0, 1.0) if L2 > 0 else np.zeros_like(X)
                d = np.hypot(X - (a[0] + t * e[0]), Y - (a[1] + t * e[1]))
                win = dist[y0:y1 + 1, x0:x1 + 1]
                np.minimum(win, d, out=win)
            a = b
    return dist


# ---- the grid of csrc/drivable_grid.h, restated ------------------------------------------------------------
def grid_lists(polygons, cell=16.0, margin=1.0):
    """{'x0', 'y0', 'nx', 'ny', 'lists': {(ix, iy): [polygon, ...]}}: every polygon in exactly the cells its bounding box, inflated by
    `margin`, touches; the grid starts at the smallest inflated corner and covers the largest."""
    boxes = np.array([[p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()] for p in (np.asarray(q, dtype=np.float64) for q in polygons)])
    x0, y0 = boxes[:, 0].min() - margin, boxes[:, 1].min() - margin
    nx = int(math.floor((boxes[:, 2].max() + margin - x0) / cell)) + 1
    ny = int(math.floor((boxes[:, 3].max() + margin - y0) / cell)) + 1
    lists = {}
    for k, b in enumerate(boxes):
        i0, i1 = int(math.floor((b[0] - margin - x0) / cell)), int(math.floor((b[2] + margin - x0) / cell))
        j0, j1 = int(math.floor((b[1] - margin - y0) / cell)), int(math.floor((b[3] + margin - y0) / cell))
        for j in range(j0, j1 + 1):
            for i in range(i0, i1 + 1):
                lists.setdefault((i, j), []).append(k)
    return {"x0": x0, "y0": y0, "nx": nx, "ny": ny, "lists": lists, "boxes": boxes}


def pixel_world(pose, res, H, W):
    """World position of every pixel centre of the raster: (H, W, 2)."""
    r = float(np.float32(res))
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    lx, ly = (X - H / 2) * r, (Y - W / 2) * -r
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return np.stack([pose[0] + lx * c - ly * s, pose[1] + lx * s + ly * c], -1)


# ---- seeded cases ----------------------------------------------------------------------------------------
def lane_strip(rng, start, heading, length, width=3.5, step=2.0, curvature=0.0, close=False):
    """One lane as a polygon: the left boundary forward, the right boundary back; close=True repeats the first vertex (shapely's ring)."""
    n = max(int(length / step), 1) + 1
    h = heading + curvature * step * np.arange(n)
    pts = np.zeros((n, 2))
    pts[0] = start
    pts[1:] = np.asarray(start) + np.cumsum(np.stack([np.cos(h[:-1]), np.sin(h[:-1])], -1) * step, 0)
    nrm = np.stack([-np.sin(h), np.cos(h)], -1) * (width / 2)
    ring = np.concatenate([pts + nrm, (pts - nrm)[::-1]], 0)
    return np.concatenate([ring, ring[:1]], 0) if close else ring


def lane_map(seed, n_strips=60, span=200.0, centre=(0.0, 0.0)):
    """A seeded town patch: n_strips lanes of 20 - 60 m at random places and headings inside a span x span square, every third one closed
    by a repeated vertex, some curved."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_strips):
        start = np.asarray(centre) + rng.uniform(-span / 2, span / 2, 2)
        out.append(lane_strip(rng, start, rng.uniform(-math.pi, math.pi), rng.uniform(20.0, 60.0), width=rng.choice([3.0, 3.5, 7.0]),
                              curvature=rng.choice([0.0, 0.0, 0.02, -0.03]), close=(k % 3 == 0)))
    return out


PIL_CASES = (  # (seed, H, W, res): the cases of tests/golden/drivable_pil.npz (tests/golden/gen_drivable.py)
    (11, 400, 400, 0.5), (12, 400, 400, 0.5), (13, 200, 300, 0.5))


def pil_case(seed, H, W, res):
    rng = np.random.default_rng(1000 + seed)
    polys = lane_map(seed, 60, span=max(H, W) * res)
    pose = (float(rng.uniform(-20, 20)), float(rng.uniform(-20, 20)), float(rng.uniform(-math.pi, math.pi)))
    return polys, pose


GPU_CELL, GPU_MARGIN = 16.0, 1.0
GPU_ORIGIN = (1500.0, -800.0)            # a town's coordinates are not small numbers


def gpu_map():
    """The 40 polygons of tests/test_gpu_drivable_map.py (cell 16 m, margin 1 m): 36 seeded lane strips in a 96 m square, and by hand a
    triangle (36), a 200-vertex disc (37), a long strip whose box spans five cells in x (38), and a 4 m square that ends 0.5 m short of a
    cell border, so that the next cell lists it through the margin only (39).  tests/test_drivable_host.py finds each of those in the grid."""
    ox, oy = GPU_ORIGIN
    polys = lane_map(5, 36, span=96.0, centre=(ox + 48.0, oy + 48.0))
    polys.append(np.array([[ox + 38.0, oy + 17.0], [ox + 50.0, oy + 19.0], [ox + 41.0, oy + 28.0]]))
    a = np.linspace(0.0, 2 * math.pi, 200, endpoint=False)
    polys.append(np.stack([ox + 60.0 + 9.0 * np.cos(a), oy + 30.0 + 9.0 * np.sin(a)], -1))
    g = grid_lists(polys, GPU_CELL, GPU_MARGIN)           # (the lower corner of the grid is set by the strips: what follows lies above it)
    bx, by = g["x0"] + 11 * GPU_CELL, g["y0"] + 8 * GPU_CELL    # a cell corner
    polys.append(np.array([[bx - 30.0, by - 12.0], [bx + 42.0, by - 12.0], [bx + 42.0, by - 8.0], [bx - 30.0, by - 8.0]]))
    polys.append(np.array([[bx - 4.5, by - 6.0], [bx - 0.5, by - 6.0], [bx - 0.5, by - 2.0], [bx - 4.5, by - 2.0]]))
    return polys


def gpu_poses(polys):
    """name -> (x, y, heading): axis-aligned in the middle of the strips; rotated at the grid's left edge, next to the polygon that sets it
    (part of the raster lies outside the grid); far from the grid origin and rotated, over the margin case and the five-cell strip."""
    g = grid_lists(polys, GPU_CELL, GPU_MARGIN)
    k = int(np.argmin(g["boxes"][:, 0]))
    v = np.asarray(polys[k])[int(np.argmin(np.asarray(polys[k])[:, 0]))]
    bx, by = g["x0"] + 11 * GPU_CELL, g["y0"] + 8 * GPU_CELL
    return {"axis": (GPU_ORIGIN[0] + 52.0, GPU_ORIGIN[1] + 30.0, 0.0), "corner": (float(v[0]) - 3.0, float(v[1]) + 1.0, 0.7),
            "far": (bx + 1.0, by - 5.0, 2.5)}


GPU_RASTERS = (((64, 64), 0.5), ((48, 80), 0.25), ((64, 64), 0.25), ((48, 80), 0.5),
               ((48, 80), 0.4))       # (0.4 is no power of two: the kernels divide by it where they multiply by 1 / 0.5)


def comb(origin, heading, n=20, pitch=2.0, width=1.0, length=30.0):
    """n strips of `width` metres every `pitch` metres ahead of `origin` along `heading`, each `length` metres across: whatever moves more than
    a metre along the heading changes between drivable and off road."""
    c, s = math.cos(heading), math.sin(heading)
    out = []
    for i in range(n):
        d0, d1 = 1.0 + pitch * i, 1.0 + pitch * i + width
        loc = np.array([[d0, -length / 2], [d1, -length / 2], [d1, length / 2], [d0, length / 2]])
        out.append(np.stack([origin[0] + loc[:, 0] * c - loc[:, 1] * s, origin[1] + loc[:, 0] * s + loc[:, 1] * c], -1))
    return out
