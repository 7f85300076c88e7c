"""The host statement of the collision test of include/rift_footprint.h: THE RULE of that header, operation for operation, in numpy fp64
(numpy does not fuse a product into a sum, so every product and every sum below is rounded once, as the kernel's __dmul_rn / __dadd_rn are).
The kernel (csrc/footprint.h) is held to this file bit for bit (tests/test_gpu_footprint.py).

    collision_matrix(center_vertices (G, Tc, 4, 2), other_vertices (N, >= Ts, 4, 2), Ts, mode) -> (flags (G, Ts) bool, first_actor (G, Ts) int32)

mode "envelope" is the test of rift_collision_matrix (the reference's STRtree query without a predicate: axis-aligned envelopes, closed
intervals); mode "footprint" tests the oriented quadrilaterals themselves behind the envelope test.
"""
import numpy as np

MODES = ("envelope", "footprint")


def _envelopes_meet(P, Q):
    """P (..., 4, 2), Q (..., 4, 2) broadcastable -> bool: the closed envelopes share a point (apart iff one lies strictly beyond the other)."""
    px0, px1, py0, py1 = P[..., 0].min(-1), P[..., 0].max(-1), P[..., 1].min(-1), P[..., 1].max(-1)
    qx0, qx1, qy0, qy1 = Q[..., 0].min(-1), Q[..., 0].max(-1), Q[..., 1].min(-1), Q[..., 1].max(-1)
    return ~((qx0 > px1) | (qx1 < px0) | (qy0 > py1) | (qy1 < py0))


def _no_axis_separates(P, Q):
    """The separating-axis part for P, Q (..., 4, 2) fp64 of one common shape: relative to vertex 0 of P, the eight edge normals (P's four
    edges, then Q's), strict comparison."""
    origin = P[..., :1, :]
    p, q = P - origin, Q - origin                                      # one rounded subtraction per coordinate
    apart = np.zeros(P.shape[:-2], dtype=np.bool_)
    for quad in (p, q):
        for k in range(4):
            a, b = quad[..., k, :], quad[..., (k + 1) & 3, :]
            nx, ny = (b[..., 1] - a[..., 1])[..., None], (a[..., 0] - b[..., 0])[..., None]
            sp = nx * p[..., 0] + ny * p[..., 1]                       # two rounded products, one rounded sum: (..., 4)
            sq = nx * q[..., 0] + ny * q[..., 1]
            apart |= (sp.min(-1) > sq.max(-1)) | (sq.min(-1) > sp.max(-1))
    return ~apart


def pair_collides(P, Q, mode: str = "footprint"):
    """P, Q (..., 4, 2), broadcastable against each other -> bool (...): the pair test of the rule (fp32 input is widened, which is exact)."""
    if mode not in MODES:
        raise ValueError(f"collision: mode = {mode!r}; known: {list(MODES)}")
    P, Q = np.broadcast_arrays(np.asarray(P).astype(np.float64), np.asarray(Q).astype(np.float64))
    hit = _envelopes_meet(P, Q)
    if mode == "footprint":
        with np.errstate(invalid="ignore", over="ignore"):
            hit = hit & _no_axis_separates(P, Q)                       # (decided for every pair; the envelope test alone clears a pair)
    return hit


def collision_matrix(center_vertices, other_vertices, Ts: int = 40, mode: str = "footprint"):
    """center_vertices (G, Tc >= Ts, 4, 2) fp32 (rows j >= Ts are not read), other_vertices (N, >= Ts, 4, 2) fp64 or None / empty with no
    neighbour -> (flags (G, Ts) bool, first_actor (G, Ts) int32: the lowest colliding neighbour, or -1)."""
    cv = np.asarray(center_vertices)[:, :Ts].astype(np.float64)                         # (G, Ts, 4, 2)
    G = cv.shape[0]
    ov = np.zeros((0, Ts, 4, 2)) if other_vertices is None else np.asarray(other_vertices, dtype=np.float64)
    if mode not in MODES:
        raise ValueError(f"collision: mode = {mode!r}; known: {list(MODES)}")
    N = ov.shape[0] if ov.size else 0
    first = np.full((G, Ts), -1, dtype=np.int32)
    if N == 0:
        return first >= 0, first
    hits = pair_collides(cv[:, None], ov[None, :, :Ts], mode)                            # (G, N, Ts)
    any_hit = hits.any(1)
    first[any_hit] = hits.argmax(1).astype(np.int32)[any_hit]
    return any_hit, first
