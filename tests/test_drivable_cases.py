"""tests/drivable_cases.py -- the numpy restatement of the drivable-area rule -- against answers derived by hand, and against a rasteriser
that is not ours (Pillow's ImageDraw.polygon, tests/golden/drivable_pil.npz written by tests/golden/gen_drivable.py)."""
import os

import numpy as np
import pytest

from tests import drivable_cases as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drivable_pil.npz")


def covered(v, pts):
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    return D.polygon_covers(np.asarray(v, dtype=np.int64), pts[:, 0], pts[:, 1]).tolist()


SQUARE = [(2, 2), (6, 2), (6, 6), (2, 6)]


def test_square_boundary_is_inclusive_vertex_horizontal_and_vertical_edge():
    X, Y = np.meshgrid(np.arange(-1, 10), np.arange(-1, 10))
    got = D.polygon_covers(np.asarray(SQUARE, dtype=np.int64), X, Y)
    want = (X >= 2) & (X <= 6) & (Y >= 2) & (Y <= 6)              # 25 pixels: the interior 3 x 3 and the whole outline
    assert np.array_equal(got, want) and int(got.sum()) == 25
    #               vertex   vertex   horizontal edges   vertical edges   just outside each
    assert covered(SQUARE, [(2, 2), (6, 6), (4, 2), (4, 6), (2, 4), (6, 4), (7, 4), (1, 2), (4, 7), (4, 1)]) == [True] * 6 + [False] * 4
    assert covered(SQUARE[::-1], [(2, 2), (4, 4), (7, 4)]) == [True, True, False]        # the orientation does not matter


def test_point_on_a_slanted_edge():
    tri = [(0, 0), (8, 0), (0, 8)]                               # hypotenuse x + y = 8
    assert covered(tri, [(4, 4), (3, 5), (7, 1), (8, 0), (0, 8)]) == [True] * 5          # on it, ends included
    assert covered(tri, [(5, 4), (4, 5), (8, 1)]) == [False] * 3                          # one pixel beyond it
    assert covered(tri, [(3, 4), (1, 1)]) == [True] * 2                                   # inside
    # a slope no pixel centre lies on between the ends: (0,0) -> (7,3)
    sl = [(0, 0), (7, 3), (0, 3)]
    assert covered(sl, [(0, 0), (7, 3), (3, 1), (2, 1), (5, 2), (4, 2), (3, 3)]) == [True, True, False, True, False, True, True]


def test_ray_through_a_vertex_counts_once_or_not_at_all():
    diamond = [(4, 0), (8, 4), (4, 8), (0, 4)]
    # the row y = 4 runs through the side vertices (0,4) and (8,4); the row y = 0 touches the apex (4,0)
    assert covered(diamond, [(2, 4), (4, 4), (7, 4)]) == [True] * 3                       # inside: the ray leaves through the vertex (8,4) once
    assert covered(diamond, [(-1, 4), (-5, 4)]) == [False] * 2                            # left of it: through both side vertices, twice
    assert covered(diamond, [(9, 4)]) == [False]
    assert covered(diamond, [(1, 0), (-3, 0), (1, 8)]) == [False] * 3                     # left of an apex: zero or two crossings, never one
    assert covered(diamond, [(4, 0), (4, 8), (0, 4), (8, 4)]) == [True] * 4               # the vertices themselves
    # a vertex that is a flat step, not an extreme: the ray from the left passes (3,2) where the outline only changes slope
    step = [(3, 0), (6, 0), (6, 4), (3, 4), (3, 2)]
    assert covered(step, [(0, 2), (4, 2), (7, 2)]) == [False, True, False]


def test_concave_polygon_notch_is_outside():
    u = [(0, 0), (9, 0), (9, 9), (6, 9), (6, 3), (3, 3), (3, 9), (0, 9)]
    assert covered(u, [(1, 6), (7, 6), (4, 2), (4, 3), (3, 6), (6, 6)]) == [True] * 6     # both arms, the base, the notch's floor and walls
    assert covered(u, [(4, 6), (5, 4), (4, 9), (5, 8)]) == [False] * 4                    # inside the notch
    X, Y = np.meshgrid(np.arange(0, 10), np.arange(0, 10))
    assert int(D.polygon_covers(np.asarray(u, dtype=np.int64), X, Y).sum()) == 100 - 2 * 6      # all but the notch's open 2 x 6 pixels


def test_ring_closed_by_a_repeated_vertex_changes_nothing():
    X, Y = np.meshgrid(np.arange(-2, 12), np.arange(-2, 12))
    for ring in (SQUARE, [(4, 0), (8, 4), (4, 8), (0, 4)], [(0, 0), (9, 0), (9, 9), (6, 9), (6, 3), (3, 3), (3, 9), (0, 9)]):
        v = np.asarray(ring, dtype=np.int64)
        closed = np.concatenate([v, v[:1]], 0)
        assert np.array_equal(D.polygon_covers(v, X, Y), D.polygon_covers(closed, X, Y))
        doubled = np.concatenate([v[:2], v[1:2], v[2:]], 0)       # a zero-length edge in the middle
        assert np.array_equal(D.polygon_covers(v, X, Y), D.polygon_covers(doubled, X, Y))


def test_transform_height_goes_to_x_and_a_strip_that_rounds_to_a_line():
    # pose (0, 0, 0), res 1, H = 8, W = 16: pixel x = X + 4 (H / 2), pixel y = -Y + 8 (W / 2)
    H, W, pose = 8, 16, (0.0, 0.0, 0.0)
    assert D.rounded_vertices([[1.0, 2.0], [-4.0, -3.0]], pose, 1.0, H, W).tolist() == [[5, 6], [0, 11]]
    assert D.rounded_vertices([[0.5, 0.0], [1.5, 0.0], [2.5, -0.5]], pose, 1.0, H, W).tolist() == [[4, 8], [6, 8], [6, 8]]      # half to even
    strip = np.array([[-3.0, 0.1], [3.0, 0.1], [3.0, -0.1], [-3.0, -0.1]])          # 0.2 m wide at 1 m per pixel: rounds to y = 8, x = 1 .. 7
    m = D.off_road_mask([strip], pose, 1.0, 16, 16)                                  # (H = W = 16: x = X + 8)
    want = np.ones((16, 16), dtype=np.uint8)
    want[8, 5:12] = 0
    assert np.array_equal(m, want)
    # rotation: heading pi / 2 turns the world's +y into the raster's +x
    m = D.off_road_mask([strip], (0.0, 0.0, np.pi / 2), 1.0, 16, 16)
    want = np.ones((16, 16), dtype=np.uint8)
    want[5:12, 8] = 0
    assert np.array_equal(m, want)


def test_no_polygons_every_point_inside_the_raster_is_off_road():
    pose = (3.0, -2.0, 0.4)
    m = D.off_road_mask([], pose, 0.5, 20, 30)
    assert m.shape == (20, 30) and m.min() == 1
    pts = np.array([[3.0, -2.0], [4.0, -1.0], [500.0, 0.0], [3.0, 40.0]], dtype=np.float32)
    assert D.off_road_flags(pts, [], pose, 0.5, 20, 30).tolist() == [True, True, False, False]      # outside the raster: not off road


def test_lookup_uses_the_drawn_mask():
    sq = np.array([[-2.0, -2.0], [2.0, -2.0], [2.0, 2.0], [-2.0, 2.0]])              # pixels 6 .. 10 in x and y at (16, 16), res 1
    pts = np.array([[0.0, 0.0], [2.0, 2.0], [2.4, 0.0], [2.6, 0.0], [-2.5, 0.0], [-2.500001, 0.0]], dtype=np.float32)
    #                inside      vertex      rounds to 10  rounds to 11   5.5 -> 6 (even)  5.499 -> 5
    assert D.off_road_flags(pts, [sq], (0.0, 0.0, 0.0), 1.0, 16, 16).tolist() == [False, False, False, True, False, True]


# ---- against Pillow --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pil():
    return np.load(GOLDEN)


@pytest.mark.parametrize("i", range(len(D.PIL_CASES)))
def test_restatement_against_the_pillow_fixture(pil, i):
    """Pixels farther than half a pixel from every rounded edge are equal; inside that band the rule is never drivable where Pillow is off
    road (Pillow also sets the outline it draws along every edge: one-sided); at least 85 % of the pixels are compared."""
    seed, H, W, res = D.PIL_CASES[i]
    assert (int(pil[f"{i}.H"]), int(pil[f"{i}.W"])) == (H, W) and float(pil[f"{i}.res"]) == res
    n = int(pil[f"{i}.n_polys"])
    start = pil[f"{i}.poly_start"]
    polys = [pil[f"{i}.vertices"][start[k]:start[k + 1]] for k in range(n)]
    pose = tuple(float(x) for x in pil[f"{i}.pose"])
    gen_polys, gen_pose = D.pil_case(seed, H, W, res)                # the fixture's inputs are the generator's
    assert pose == gen_pose and all(np.array_equal(a, b) for a, b in zip(polys, gen_polys))
    theirs = pil[f"{i}.mask"]
    ours = D.off_road_mask(polys, pose, res, H, W)
    assert theirs.shape == ours.shape == (H, W)
    far = D.edge_distance(polys, pose, res, H, W) > 0.5
    print(f"case {i}: compared {far.mean():.4f}, differing in the band {(ours != theirs)[~far].mean():.4f}, drivable {np.mean(ours == 0):.3f}")
    assert far.mean() >= 0.85
    assert np.array_equal(ours[far], theirs[far])
    assert not np.any((ours == 0) & (theirs == 1))
    assert 0.1 < np.mean(ours == 0) < 0.9                              # (the case shows both kinds of pixel)
