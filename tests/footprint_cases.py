"""The cases of the footprint collision test (include/rift_footprint.h), shared by the CPU and the GPU tests.

* KNOWN: pairs of convex quadrilaterals whose coordinates are small dyadic rationals (multiples of 2^-4, |x| <= 64): every operation of the
  rule is then exact, and `exact_pair` / `exact_envelope` decide the geometric truth in exact arithmetic (fractions.Fraction) by a
  segment-crossing / containment test written separately from the host statement.
* random_problem: 2 000 seeded rectangle pairs at CARLA magnitudes laid out as one (G, Ts, N) problem.
* lane_scene: a CBV heading 45 degrees with a stationary neighbour parallel to it one lane away -- the scene the reference's envelope test
  gets wrong on every step the two are side by side.
tests/test_footprint_cases.py checks that the cases are what they claim."""
from fractions import Fraction

import numpy as np


# ---- exact arithmetic -----------------------------------------------------------------------------------------------------------------
def _fr(quad):
    return [(Fraction(float(x)), Fraction(float(y))) for x, y in np.asarray(quad, dtype=np.float64)]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _on_segment(a, b, p):
    return _cross(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def _segments_meet(a, b, c, d):
    """Closed segments ab and cd share a point."""
    d1, d2, d3, d4 = _cross(c, d, a), _cross(c, d, b), _cross(a, b, c), _cross(a, b, d)
    if ((d1 > 0) != (d2 > 0)) and d1 != 0 and d2 != 0 and ((d3 > 0) != (d4 > 0)) and d3 != 0 and d4 != 0:
        return True
    return _on_segment(c, d, a) or _on_segment(c, d, b) or _on_segment(a, b, c) or _on_segment(a, b, d)


def _inside_closed(quad, p):
    """p in the closed convex quadrilateral, whatever its winding."""
    s = [_cross(quad[k], quad[(k + 1) % 4], p) for k in range(4)]
    return all(x >= 0 for x in s) or all(x <= 0 for x in s)


def exact_pair(P, Q) -> bool:
    """The closed convex quadrilaterals P and Q share a point: two edges meet, or one holds a vertex of the other."""
    p, q = _fr(P), _fr(Q)
    for i in range(4):
        for j in range(4):
            if _segments_meet(p[i], p[(i + 1) % 4], q[j], q[(j + 1) % 4]):
                return True
    return _inside_closed(p, q[0]) or _inside_closed(q, p[0])


def exact_envelope(P, Q) -> bool:
    """The closed axis-aligned envelopes of P and Q share a point."""
    p, q = _fr(P), _fr(Q)
    lo = lambda v, k: min(x[k] for x in v)      # noqa: E731
    hi = lambda v, k: max(x[k] for x in v)      # noqa: E731
    return all(lo(q, k) <= hi(p, k) and lo(p, k) <= hi(q, k) for k in (0, 1))


# ---- known-answer pairs ---------------------------------------------------------------------------------------------------------------
def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _diamond(cx, cy, r=1.0):
    return [(cx + r, cy), (cx, cy + r), (cx - r, cy), (cx, cy - r)]


def _tilted(ox, oy, a, b):
    """A rectangle with edges a * (4, 3) and b * (-3, 4) from (ox, oy): right angles with dyadic coordinates."""
    u, v = (4 * a, 3 * a), (-3 * b, 4 * b)
    return [(ox, oy), (ox + u[0], oy + u[1]), (ox + u[0] + v[0], oy + u[1] + v[1]), (ox + v[0], oy + v[1])]


S = 2.0 ** -4
_BASE = (  # (name, P, Q, the pair collides, the envelopes meet)
    ("overlapping", _rect(0, 0, 4, 2), _tilted(1, 1, 1.0, 0.5), True, True),
    ("one inside the other", _rect(0, 0, 8, 8), _diamond(4, 4), True, True),
    ("corner to corner", _rect(0, 0, 2, 2), _rect(2, 2, 4, 4), True, True),
    ("corner to edge", _rect(0, 0, 2, 2), _diamond(3, 1), True, True),
    ("edge to edge", _rect(0, 0, 2, 2), _rect(2, 0.5, 4, 1.5), True, True),
    ("tilted edge to tilted edge", _tilted(0, 0, 1.0, 0.5), _tilted(-1.5, 2, 1.0, 0.5), True, True),
    ("apart by 2^-4 along an edge normal", _rect(0, 0, 2, 2), _rect(2 + S, 0, 4, 2), False, False),
    ("apart by (-3, 4) / 16 along a tilted edge normal", _tilted(0, 0, 1.0, 0.5), _tilted(-1.5 - 3 * S, 2 + 4 * S, 1.0, 0.5), False, True),
    ("diamonds offset diagonally", _diamond(0, 0), _diamond(1.25, 1.25), False, True),
    ("diamonds touching along an edge", _diamond(0, 0), _diamond(1, 1), True, True),
    ("diamonds apart by 2^-4 per axis", _diamond(0, 0), _diamond(1 + S, 1 + S), False, True),
    ("far from the origin", _rect(60, -64, 64, -62), _tilted(61, -63, 0.25, 0.25), True, True),
)


def known_pairs():
    """[(name, P (4, 2) f32, Q (4, 2) f64, collides, envelopes meet)]: every base pair as given, with both windings reversed, and with P and Q
    exchanged (the candidate is the fp32 one: dyadic coordinates of this size are exact in fp32)."""
    out = []
    for name, P, Q, hit, env in _BASE:
        for tag, p, q in (("", P, Q), (" (reversed winding)", P[::-1], Q[::-1]), (" (P and Q exchanged)", Q, P)):
            out.append((name + tag, np.asarray(p, dtype=np.float32), np.asarray(q, dtype=np.float64), hit, env))
    return out


# ---- random rectangles at CARLA magnitudes --------------------------------------------------------------------------------------------
RANDOM_SEED, RANDOM_SHAPE = 20, (25, 8, 10)      # (G, Ts, N): 2 000 pairs


def _boxes(g, centre, n):
    """n rectangles near `centre`: length 3.6 - 5.4 m, width 1.7 - 2.2 m, any heading -> (n, 4, 2) f64, corners FL RL RR FR."""
    c = centre + g.uniform(-4.5, 4.5, (n, 2))
    h = g.uniform(-np.pi, np.pi, n)
    hl, hw = g.uniform(1.8, 2.7, n), g.uniform(0.85, 1.1, n)
    dx, dy = np.stack([hl, -hl, -hl, hl], -1), np.stack([hw, hw, -hw, -hw], -1)
    ch, sh = np.cos(h)[:, None], np.sin(h)[:, None]
    return np.stack([dx * ch - dy * sh, dx * sh + dy * ch], -1) + c[:, None]


def random_problem():
    """center_vertices (G, Ts, 4, 2) f32 and other_vertices (N, Ts, 4, 2) f64: per step one place within +-2 000 m, G candidate and N
    neighbour rectangles within a few metres of it -- G * Ts * N = 2 000 pairs, many of them close enough for the two tests to differ."""
    G, Ts, N = RANDOM_SHAPE
    g = np.random.default_rng(RANDOM_SEED)
    cv, ov = np.empty((G, Ts, 4, 2), dtype=np.float32), np.empty((N, Ts, 4, 2))
    for j in range(Ts):
        centre = g.uniform(-2000.0, 2000.0, 2)
        cv[:, j] = _boxes(g, centre, G).astype(np.float32)
        ov[:, j] = _boxes(g, centre, N)
    return cv, ov


# ---- the lane-neighbour scene ---------------------------------------------------------------------------------------------------------
LANE_POSE = (10.0, -5.0, np.pi / 4)              # the CBV: x, y, heading (right-handed global frame)
LANE_STATE = {"speed": 6.0, "width": 2.0, "length": 4.6}
LANE_WIDTH = 3.5


def lane_scene():
    """K = 1, R = 1: twelve straight candidates at 3 .. 8.5 m/s that fan out slightly to the right, a straight reference line, and one
    stationary neighbour (4.6 m x 2.0 m before inflation) parallel to the CBV one lane to its left, side by side with it at the start.
    Returns trajectory (1, 1, 12, 80, 6) f32, the CBV's tick entry (no raster: no off-road flags) and the actor readings."""
    import torch
    t = np.arange(80, dtype=np.float64)
    traj = np.zeros((1, 1, 12, 80, 6), dtype=np.float32)
    for m in range(12):
        v, th = 3.0 + 0.5 * m, -0.004 * m
        s = v * 0.1 * t
        traj[0, 0, m] = np.stack([s * np.cos(th), s * np.sin(th), np.full(80, np.cos(th)), np.full(80, np.sin(th)), np.full(80, v * np.cos(th)),
                                  np.full(80, v * np.sin(th))], -1)
    ref_pos = np.stack([np.arange(100, dtype=np.float32), np.zeros(100, dtype=np.float32)], -1)
    ref_ang = np.zeros(100, dtype=np.float32)
    x, y, h = LANE_POSE
    nx, ny = x - LANE_WIDTH * np.sin(h), y + LANE_WIDTH * np.cos(h)
    actors = {"steer": np.zeros(1), "throttle": np.zeros(1), "brake": np.ones(1), "speed": np.zeros(1),
              "location": np.array([[nx, -ny, 0.1]]), "yaw_deg": np.array([-np.degrees(h)]), "extent": np.array([[2.3, 1.0]])}      # CARLA frame: y and yaw flipped
    entry = {"batch_index": 0, "center_state": (x, y, h, LANE_STATE["speed"], LANE_STATE["width"], LANE_STATE["length"]),
             "ref_pos": [ref_pos], "ref_angle": [ref_ang], "actors": actors, "off_road": None}
    return torch.from_numpy(traj), entry, actors
