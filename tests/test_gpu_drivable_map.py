"""Off-road flags from the device-resident drivable-area map (include/rift_drivable.h: riftdm_load and the entries behind it), on the
device, through the C-ABI.  Every comparison is bit-exact on uint8 / on the bytes of the doubles.  The reference of the rule is the
brute-force numpy restatement of tests/drivable_cases.py (no grid, no culling; tests/test_drivable_cases.py checks it by hand and against
Pillow); the reference of the lookup and of the tick are the entries that take a mask.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import drivable_cases as D
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ffi():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    _ffi.load_library()
    return _ffi


@functools.lru_cache(maxsize=None)
def _world():
    polys = D.gpu_map()
    return polys, D.gpu_poses(polys), D.grid_lists(polys, D.GPU_CELL, D.GPU_MARGIN)


@functools.lru_cache(maxsize=None)
def _want_mask(pose_name, H_, W_, res):
    polys, poses, _ = _world()
    return D.off_road_mask(polys, poses[pose_name], res, H_, W_)


@pytest.fixture(scope="module")
def eng(ffi):
    """One engine with the 40-polygon map loaded; the tests that replace or clear a map make their own."""
    e = ffi.Engine("cuda:0")
    info = e.load_drivable_map(_world()[0], cell=D.GPU_CELL, margin=D.GPU_MARGIN)
    g = _world()[2]
    assert (info["n_polys"], info["n_vertices"], info["nx"], info["ny"]) == (40, sum(len(p) for p in _world()[0]), g["nx"], g["ny"])
    assert (info["cell"], info["margin"], info["x0"], info["y0"]) == (D.GPU_CELL, D.GPU_MARGIN, g["x0"], g["y0"])
    assert info["max_cell_list"] == max(len(v) for v in g["lists"].values()) and info["device_bytes"] > 0
    yield e
    e.close()


def _cells_seen(pose, res, H_, W_, g):
    w = D.pixel_world(pose, res, H_, W_)
    ix, iy = np.floor((w[..., 0] - g["x0"]) / D.GPU_CELL), np.floor((w[..., 1] - g["y0"]) / D.GPU_CELL)
    outside = (ix < 0) | (ix >= g["nx"]) | (iy < 0) | (iy >= g["ny"])
    return set(zip(ix[~outside].astype(int).tolist(), iy[~outside].astype(int).tolist())), float(outside.mean())


@pytest.mark.parametrize("pose_name", ["axis", "corner", "far"])
def test_raster_equals_the_restatement(eng, pose_name):
    """riftdm_raster against the restatement's mask: the 40 polygons (a triangle, a 200-vertex disc, a strip five cells wide, a
    square one cell lists through the margin only) at an axis-aligned pose, a rotated one at the grid's edge (more than half the raster
    outside the grid) and a rotated one far from the grid's origin (over the margin case, with empty cells in view); rasters 64 x 64 and
    48 x 80 at 0.5 and 0.25 m per pixel, and 48 x 80 at 0.4 (no power of two: the kernels divide).  Fails on a library without the entry."""
    polys, poses, g = _world()
    pose = poses[pose_name]
    for (H_, W_), res in D.GPU_RASTERS:
        got = eng.drivable_raster(pose, (H_, W_), eng.eval_params(resolution=res)).cpu().numpy()
        want = _want_mask(pose_name, H_, W_, res)
        cells, outside = _cells_seen(pose, res, H_, W_, g)
        print(f"{pose_name} {H_}x{W_} res {res}: drivable {np.mean(want == 0):.3f}, outside the grid {outside:.3f}, cells {len(cells)}, "
              f"empty cells {sum(c not in g['lists'] for c in cells)}, differing pixels {int((got != want).sum())}")
        assert got.dtype == np.uint8 and got.shape == (H_, W_)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        if pose_name == "corner":
            assert 0.3 < outside < 0.9
        if pose_name == "far":
            margin_cell = sorted(c for c, l in g["lists"].items() if 39 in l)[1]
            assert margin_cell in cells and any(c not in g["lists"] for c in cells)
    # what the case is there to show is in the view: the disc and the triangle at "axis", the five-cell strip and the square at "far"
    if pose_name == "axis":
        assert (_want_mask("axis", 64, 64, 0.5) == 0).mean() > 0.3
        for k in (36, 37):
            assert (D.off_road_mask([polys[k]], pose, 0.5, 64, 64) == 0).mean() > 0.02, k
    if pose_name == "far":
        for k in (38, 39):
            assert (D.off_road_mask([polys[k]], pose, 0.5, 64, 64) == 0).any(), k


def _points(n, pose, res, H_, W_, seed):
    """n float32 points around the raster: most inside, some beyond every edge."""
    g = np.random.default_rng(seed)
    r = float(np.float32(res))
    px, py = g.uniform(-6.0, W_ + 6.0, n), g.uniform(-6.0, H_ + 6.0, n)
    lx, ly = (px - H_ / 2) * r, (py - W_ / 2) * -r
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return np.stack([pose[0] + lx * c - ly * s, pose[1] + lx * s + ly * c], -1).astype(np.float32)


@pytest.mark.parametrize("n", [1, 255, 257, 12 * 80 * 3])
def test_flags_equal_the_lookup_on_the_drawn_raster(eng, n):
    """riftdm_off_road_matrix against rift_off_road_matrix run on the mask riftdm_raster drew, and against the restatement, at
    n_points below, at and past one block of 256 and at a CBV's 12 x 80 x 3."""
    polys, poses, _ = _world()
    seen = 0
    for pose_name, ((H_, W_), res) in (("far", D.GPU_RASTERS[0]), ("axis", D.GPU_RASTERS[1]), ("corner", D.GPU_RASTERS[4])):
        pose = poses[pose_name]
        params = eng.eval_params(resolution=res)
        pts = _points(n, pose, res, H_, W_, seed=n + H_)
        mask = eng.drivable_raster(pose, (H_, W_), params)
        got = eng.off_road_matrix_map(torch.from_numpy(pts).view(1, n, 2), pose, (H_, W_), params).cpu().numpy()
        rf = float(np.float32(res))
        looked = eng.off_road_matrix(torch.from_numpy(pts).view(1, n, 2), mask, pose[:2], pose[2], resolution_hw=(rf, -rf), offset=(H_ / 2, W_ / 2)).cpu().numpy()
        want = D.off_road_flags(pts, polys, pose, res, H_, W_, mask=_want_mask(pose_name, H_, W_, res))
        assert got.shape == (1, n) and np.array_equal(got, looked) and np.array_equal(got[0], want)
        seen += int(got.any() and not got.all())
    assert n == 1 or seen >= 2                                   # both answers occur


def test_flags_at_half_pixel_ties_and_raster_edges(ffi):
    """The points of tests/golden/off_road.npz's first case -- on half-pixel ties and on the raster's edges, at its pose and its 400 x 400
    raster -- against a lane map drawn around that pose: map flags = lookup on the drawn mask = restatement."""
    name, _, pts, pose, _ = H.off_road_cases()[0]
    assert name == "axis_ties" and pts.dtype == np.float32
    polys = D.lane_map(21, 60, span=200.0, centre=pose[:2])
    e = ffi.Engine("cuda:0")
    try:
        e.load_drivable_map(polys)
        params = e.eval_params()
        mask = e.drivable_raster(pose, (400, 400), params)
        want_mask = D.off_road_mask(polys, pose, 0.5, 400, 400)
        assert np.array_equal(mask.cpu().numpy(), want_mask)
        got = e.off_road_matrix_map(torch.from_numpy(pts), pose, (400, 400), params).cpu().numpy()
        looked = e.off_road_matrix(torch.from_numpy(pts), mask, pose[:2], pose[2], resolution_hw=(0.5, -0.5), offset=(200.0, 200.0)).cpu().numpy()
        want = D.off_road_flags(pts, polys, pose, 0.5, 400, 400, mask=want_mask)
        assert np.array_equal(got, looked) and np.array_equal(got, want) and got.any() and not got.all()
        px, valid = D.point_pixels(pts.reshape(-1, 2), pose, 0.5, 400, 400)
        frac = np.abs(D.global_to_pixel(pts.reshape(-1, 2).astype(np.float64), pose, 0.5, 400, 400) % 1.0 - 0.5)
        assert (frac == 0).sum() >= 4 and (~valid).any() and ((px[valid] == 0) | (px[valid] == 399)).any()      # ties, outside, on the edge
    finally:
        e.close()


# ---- the tick -------------------------------------------------------------------------------------------------------------------------
TICK_SIZES = ((160, 160), (100, 150))
MAP_CBVS, MASK_CBVS, BARE_CBV = (0, 2, 3, 5, 8), (1, 4, 7), 6


@functools.lru_cache(maxsize=None)
def _tick_world():
    """Nine CBVs (one more than RIFT_TICK_CHUNK) with R = 1 in rows of Rb = 2, along the strips of the 40-polygon map at different poses;
    two of them on a 100 x 150 raster; some without neighbours."""
    _, poses, _ = _world()
    ax = poses["axis"]
    traj = torch.zeros(9, 2, 12, 80, 6)
    cbvs = []
    for k in range(9):
        tr, ref_pos, ref_ang, st = H.rollout_inputs(1200 + k, R=1)
        pos, heading = (ax[0] - 30.0 + 7.0 * k, ax[1] - 20.0 + 5.0 * k), 0.3 - 0.25 * k
        traj[k, :1] = tr
        a = None
        if k % 3 != 0:
            a = H.other_vehicle_inputs(seed=500 + k, N=4)
            g = np.random.default_rng(k)
            ahead, side = 8.0 + 7.0 * np.arange(4), g.uniform(-4.0, 4.0, 4)
            a["location"] = np.stack([pos[0] + ahead * np.cos(heading) - side * np.sin(heading),
                                      -(pos[1] + ahead * np.sin(heading) + side * np.cos(heading)), np.full(4, 0.1)], -1)
            a["yaw_deg"] = -np.degrees(heading) + g.uniform(-20, 20, 4)
        cbvs.append({"batch_index": k, "center_state": (pos[0], pos[1], heading, 6.0 + 0.2 * k, st["width"], st["length"]),
                     "ref_pos": [p.numpy() for p in ref_pos], "ref_angle": [x.numpy() for x in ref_ang], "actors": a,
                     "pose": (pos[0], pos[1], heading), "size": TICK_SIZES[1] if k in (2, 4) else TICK_SIZES[0]})
    return traj, cbvs


TICK_RES = 0.5


def _run_tick(e, which):
    """which = 'map': the mixed tick through riftdm_group_advantage_tick; 'masks': every raster uploaded, rift_group_advantage_tick_ex."""
    from rift_amd.planning.fine_tuner.rlft.traj_eval.traj_evaluator import TrajEvaluator
    traj, cbvs = _tick_world()
    params = e.eval_params(gamma=0.95, resolution=TICK_RES)
    masks = {k: e.drivable_raster(v["pose"], v["size"], params).cpu().numpy() for k, v in enumerate(cbvs) if k != BARE_CBV}
    entries = []
    for k, v in enumerate(cbvs):
        d = {key: v[key] for key in ("batch_index", "center_state", "ref_pos", "ref_angle", "actors")}
        if k == BARE_CBV:
            d["off_road"] = None
        elif which == "masks" or k in MASK_CBVS:
            d["off_road"] = (masks[k], v["pose"])
        else:
            d["off_road"], d["raster"], d["pose"] = None, v["size"], v["pose"]
        entries.append(d)
    res = e.group_advantage_tick(traj.cuda(), entries, TrajEvaluator(e).pid_state, params=params, want_returns=True, want_terms=True)
    return {k: res[k].cpu().numpy() for k in ("advantage", "returns", "terms")}, masks


def test_tick_map_equals_tick_ex_with_every_mask_uploaded(eng):
    """riftdm_group_advantage_tick with nine CBVs at different poses -- five from the map, three with uploaded masks that
    riftdm_raster drew, one with neither -- against rift_group_advantage_tick_ex with the masks of all eight uploaded: advantage,
    returns and terms equal bit for bit; rows r >= R untouched; the off-road term is at work (some candidates pay it, some do not)."""
    got, masks = _run_tick(eng, "map")
    want, _ = _run_tick(eng, "masks")
    for key in ("advantage", "returns", "terms"):
        assert got[key].tobytes() == want[key].tobytes(), key
    off = got["terms"][:, 0, :, 1]                               # (9, 12): the discounted off-road term of every candidate
    assert not got["advantage"][:, 1:].any() and not got["terms"][:, 1:].any()
    assert not off[BARE_CBV].any()
    mixed = [k for k in MAP_CBVS if off[k].any() and not off[k].all()]
    print(f"tick: off-road term nonzero for {int((off != 0).sum())} of {off.size} candidates; CBVs from the map with both kinds {mixed}; "
          f"drivable share of the masks {[round(float((m == 0).mean()), 2) for m in masks.values()]}")
    assert (off[list(MAP_CBVS)] != 0).any() and (off[list(MAP_CBVS)] == 0).any() and (off[list(MASK_CBVS)] != 0).any()


def test_poisoned_arena_changes_nothing(ffi, eng, monkeypatch):
    """An engine created with RIFT_POISON_ARENA=255: the rasters and the mixed tick are the plain engine's, bit for bit."""
    plain, plain_masks = _run_tick(eng, "map")
    monkeypatch.setenv("RIFT_POISON_ARENA", "255")
    e = ffi.Engine("cuda:0")
    try:
        e.load_drivable_map(_world()[0], cell=D.GPU_CELL, margin=D.GPU_MARGIN)
        got, masks = _run_tick(e, "map")
        assert all(np.array_equal(masks[k], plain_masks[k]) for k in masks)
        assert all(got[k].tobytes() == plain[k].tobytes() for k in got)
    finally:
        e.close()


# ---- errors and reload ----------------------------------------------------------------------------------------------------------------
def test_reload_clear_and_refusals(ffi):
    """A second load replaces the map (the answers change and are the second map's); after a clear every entry that reads the map returns
    RIFT_ERR_STATE; resolution 1.0 against margin 1.0, H or W <= 0 and a map that is refused return RIFT_ERR_ARG with the reason -- and
    nothing was launched: the output keeps the bytes it held."""
    from rift_amd import _abi
    polys, poses, _ = _world()
    pose = poses["axis"]
    e = ffi.Engine("cuda:0")
    try:
        assert e.drivable_map_info() is None
        with pytest.raises(RuntimeError, match="no drivable-area map is loaded"):
            e.drivable_raster(pose, (64, 64))
        e.load_drivable_map(polys, cell=D.GPU_CELL, margin=D.GPU_MARGIN)
        first = e.drivable_raster(pose, (64, 64)).cpu().numpy()
        moved = [p + np.array([9.0, -4.0]) for p in polys[:20]]
        info = e.load_drivable_map(moved, cell=8.0, margin=2.0)
        assert (info["n_polys"], info["cell"], info["margin"]) == (20, 8.0, 2.0)
        second = e.drivable_raster(pose, (64, 64)).cpu().numpy()
        assert np.array_equal(first, _want_mask("axis", 64, 64, 0.5)) and np.array_equal(second, D.off_road_mask(moved, pose, 0.5, 64, 64))
        assert not np.array_equal(first, second)
        # ---- refusals with a map loaded: the reason, and the output untouched
        out = torch.full((64, 64), 7, dtype=torch.uint8, device="cuda:0")
        pts = torch.zeros(1, 5, 2, device="cuda:0")
        flags = torch.full((5,), 7, dtype=torch.uint8, device="cuda:0")
        lib, ctx, p = e.lib, e.ctx, ffi._ptr

        def raster(H_, W_, params, dst=out):
            return lib.riftdm_raster(ctx, H_, W_, pose[0], pose[1], pose[2], C.byref(params) if params is not None else None, p(dst), None)

        def err():
            return lib.rift_last_error(ctx).decode()

        assert raster(64, 64, e.eval_params(resolution=1.5)) == _abi.RIFT_ERR_ARG and "margin" in err()          # 1.5 * sqrt(2) > 2.0
        assert raster(64, 64, e.eval_params(resolution=1.0)) == _abi.RIFT_OK                                     # 1.0 * sqrt(2) <= 2.0
        out.fill_(7)
        e.load_drivable_map(polys, cell=D.GPU_CELL, margin=1.0)
        assert raster(64, 64, e.eval_params(resolution=1.0)) == _abi.RIFT_ERR_ARG and "sqrt(2)" in err() and "margin" in err()
        rc = lib.riftdm_off_road_matrix(ctx, p(pts), 5, 64, 64, pose[0], pose[1], pose[2], C.byref(e.eval_params(resolution=1.0)), p(flags), None)
        assert rc == _abi.RIFT_ERR_ARG and "margin" in err()
        for H_, W_ in ((0, 64), (64, 0), (-1, 64)):
            assert raster(H_, W_, e.eval_params()) == _abi.RIFT_ERR_ARG and "H or W <= 0" in err()
        assert raster(64, 64, None) == _abi.RIFT_ERR_ARG
        assert raster(64, 64, e.eval_params(resolution=float("nan"))) == _abi.RIFT_ERR_ARG
        with pytest.raises(RuntimeError, match="fewer than 3 vertices"):
            e.load_drivable_map([polys[0], polys[1][:2]])
        with pytest.raises(RuntimeError, match="not finite"):
            e.load_drivable_map([polys[0], polys[1] * np.array([np.inf, 1.0])])
        with pytest.raises(RuntimeError, match="cell <= 0"):
            e.load_drivable_map(polys, cell=0.0)
        with pytest.raises(RuntimeError, match="margin < 0"):
            e.load_drivable_map(polys, margin=-1.0)
        assert e.drivable_map_info()["n_polys"] == 40              # a refused load leaves the loaded map in place
        # the tick: a CBV that asks for the map with a raster of no size, and a resolution the margin cannot decide
        traj, cbvs = _tick_world()
        from rift_amd.planning.fine_tuner.rlft.traj_eval.traj_evaluator import TrajEvaluator
        pid = TrajEvaluator(e).pid_state
        entry = dict({k: cbvs[0][k] for k in ("batch_index", "center_state", "ref_pos", "ref_angle", "actors")}, off_road=None, pose=cbvs[0]["pose"])
        with pytest.raises(RuntimeError, match="H or W <= 0 where the map is asked for"):
            e.group_advantage_tick(traj.cuda(), [dict(entry, raster=(0, 64))], pid, params=e.eval_params())
        with pytest.raises(RuntimeError, match="margin"):
            e.group_advantage_tick(traj.cuda(), [dict(entry, raster=(64, 64))], pid, params=e.eval_params(resolution=1.0))
        torch.cuda.synchronize()
        assert int(out.min()) == 7 and int(out.max()) == 7 and int(flags.min()) == 7 and int(flags.max()) == 7
        # ---- clear
        e.clear_drivable_map()
        assert e.drivable_map_info() is None
        assert raster(64, 64, e.eval_params()) == _abi.RIFT_ERR_STATE and "no drivable-area map is loaded" in err()
        rc = lib.riftdm_off_road_matrix(ctx, p(pts), 5, 64, 64, pose[0], pose[1], pose[2], C.byref(e.eval_params()), p(flags), None)
        assert rc == _abi.RIFT_ERR_STATE
        with pytest.raises(RuntimeError, match=r"riftdm_group_advantage_tick failed \(%d\).*no drivable-area map" % _abi.RIFT_ERR_STATE):
            e.group_advantage_tick(traj.cuda(), [dict(entry, raster=(64, 64))], pid, params=e.eval_params())
        torch.cuda.synchronize()
        assert int(out.min()) == 7 and int(out.max()) == 7 and int(flags.min()) == 7 and int(flags.max()) == 7
        e.clear_drivable_map()                                       # (twice: nothing to release)
    finally:
        e.close()


# ---- the policy -----------------------------------------------------------------------------------------------------------------------
POLICY_POSE = lambda cbv_id: (10.0 + cbv_id, -5.0, 0.3)      # noqa: E731


class _States:
    """Recorded readings of a town: the lane map around the CBVs, one oncoming neighbour and three seeded ones per CBV.  With `masks` the
    source also draws rasters (the masks Engine.drivable_raster drew for the same poses); without, it only knows poses and polygons."""

    def __init__(self, polygons, masks=None):
        self.polygons, self.masks, self.area_reads = polygons, masks, 0

    def center_state(self, env_id, cbv_id):
        from rift_amd.planning.pluto.pluto import CenterState
        return CenterState(10.0 + cbv_id, -5.0, 0.3, 6.0 + 0.1 * cbv_id, 2.0, 4.6)

    def nearby_actor_states(self, env_id, cbv_id):
        a = H.other_vehicle_inputs(seed=100 + cbv_id, N=4)
        gx, gy = 10.0 + cbv_id + 12.0 * np.cos(0.3), -5.0 + 12.0 * np.sin(0.3)
        a["location"][0], a["yaw_deg"][0], a["speed"][0] = (gx, -gy, 0.1), -np.degrees(0.3) + 180.0, 3.0
        a["steer"][0] = a["throttle"][0] = a["brake"][0] = 0.0
        return a

    def off_road_raster(self, env_id, cbv_id):
        if self.masks is None:
            raise AssertionError("the map path must not ask for a raster")
        return self.masks[cbv_id], POLICY_POSE(cbv_id)

    def drivable_area(self, env_id):
        self.area_reads += 1
        return "town-of-the-test", self.polygons

    def off_road_pose(self, env_id, cbv_id):
        return POLICY_POSE(cbv_id)


def test_policy_map_mode_equals_the_raster_path(ffi, tmp_path):
    """rift_pluto in train mode, two ticks (three CBVs, then two) from a recorded state source: with {'off_road': 'map'} -- fused and through
    the per-CBV chain -- CBVs_group_advantage is, bit for bit, what the raster path gives when fed the masks Engine.drivable_raster draws
    from the same polygons; the map is loaded once for both ticks and no raster is asked for.  Without the key and with 'off_road':
    'raster' the outputs are equal: the key's default is the call made without it.  With the breakdown on, the off-road term of these
    ticks is nonzero for some candidates of a CBV and zero for others: the flags decide these advantages."""
    import rift_amd.synthetic as syn
    from rift_amd.planning import CBV_POLICY_LIST
    from rift_amd.planning.pluto.feature_builder.pluto_feature import PlutoFeature
    torch.cuda.set_device(0)
    # (lanes beside the CBVs, and ahead of them a comb of 1 m strips every 3 m: flags that differ between the candidates of a CBV)
    polygons = D.lane_map(31, 40, span=120.0, centre=(60.0, 70.0)) + D.comb((10.0, -5.0), 0.3, pitch=3.0)
    ticks = [[1, 2, 3], [2, 5]]
    e = ffi.Engine("cuda:0")
    try:
        e.load_drivable_map(polygons)
        masks = {c: e.drivable_raster(POLICY_POSE(c), (400, 400)).cpu().numpy() for c in {c for ids in ticks for c in ids}}
    finally:
        e.close()
    assert all(0.05 < (m == 0).mean() < 0.95 for m in masks.values())
    sd = H.weights()
    runs, sources, terms = {}, {}, []
    for name, section, fused in (("none", None, True), ("raster", {'off_road': 'raster'}, True), ("map", {'off_road': 'map'}, True),
                                 ("map_chain", {'off_road': 'map', 'raster_size': (400, 400), 'map_cell': 16.0, 'map_margin': 1.0}, False),
                                 ("map_terms", {'off_road': 'map', 'breakdown': True}, True)):
        src = _States(polygons, None if name.startswith("map") else masks)
        cfg = {'num_scenario': 1, 'ROOT_DIR': str(tmp_path), 'model_path': 'ckpt', 'device': 'cuda:0', 'state_source': src, 'fused_tick': fused}
        if section is not None:
            cfg['traj_eval'] = section
        pol = CBV_POLICY_LIST['rift_pluto'](cfg, None)
        pol.pluto_model.load_state_dict(sd)
        pol.set_mode('train')
        cols = []
        for t, ids in enumerate(ticks):
            feats = {c: syn.make_scene(7000 + 16 * t + c, num_agents=12, num_polygons=8, r_min=1, r_max=3)["feature"] for c in ids}
            obs = {c: {'raw_pluto_feature': PlutoFeature(data=feats[c])} for c in ids}
            act = pol.get_action([obs], [{'env_id': 0}], deterministic=False)
            cols += [act['CBVs_group_advantage'][0][c]['advantage'] for c in ids]
            if name == "map_terms":
                for c in ids:
                    bd = pol.last_tick_breakdown[c]['terms']
                    terms.append(bd[..., 1] != 0)
                    print(f"tick {t} cbv {c}: off-road term nonzero for {int((bd[..., 1] != 0).sum())} of {bd[..., 1].size} candidates, "
                          f"steps counted {int(bd[..., 7].min())} .. {int(bd[..., 7].max())}")
        runs[name], sources[name] = cols, src
        if name.startswith("map"):
            assert pol.drivable_map_loads == 1 and pol.drivable_map_info["n_polys"] == 60 and src.area_reads == 2
        pol.pluto_model.release_engine()
    for a, b, c, d in zip(runs["none"], runs["raster"], runs["map"], runs["map_chain"]):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()
    assert sources["none"].area_reads == 0 and sources["raster"].area_reads == 0
    # the off-road term is at work in these ticks: with the breakdown on, some candidates pay it and some do not
    assert any(off.any() and not off.all() for off in terms), [float(off.mean()) for off in terms]
    for a, m in zip(runs["map"], runs["map_terms"]):
        assert a.tobytes() == m.tobytes()
