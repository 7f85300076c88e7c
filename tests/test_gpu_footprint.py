"""Collision flags from the footprints themselves (include/rift_footprint.h: riftfp_collision_matrix, riftfp_group_advantage_tick) on the
device, through the C-ABI.  The rule fixes every rounding, so every comparison is bit for bit: the kernel against the host statement
(rift_amd/planning/fine_tuner/rlft/traj_eval/footprint.py, held to exact arithmetic by tests/test_footprint_cases.py), ENVELOPE against the
entries of before, the fused tick against the composition of the separate entries.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import footprint_cases as F
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ffi():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    _ffi.load_library()
    return _ffi


@pytest.fixture(scope="module")
def eng(ffi):
    e = ffi.Engine("cuda:0")
    yield e
    e.close()


def _host(cv, ov, Ts, mode):
    from rift_amd.planning.fine_tuner.rlft.traj_eval import footprint
    return footprint.collision_matrix(cv, ov, Ts=Ts, mode=mode)


def _check(eng, cv, ov, Ts, modes=("footprint", "envelope")):
    """Engine.collision_matrix(mode, want_first=True) against the host statement: flags and first_actor, every element."""
    out = {}
    for mode in modes:
        flags, first = eng.collision_matrix(torch.from_numpy(cv), torch.from_numpy(ov) if ov is not None else torch.zeros(0, Ts, 4, 2, dtype=torch.float64),
                                            Ts=Ts, mode=mode, want_first=True)
        want_flags, want_first = _host(cv, ov, Ts, mode)
        flags, first = flags.cpu().numpy(), first.cpu().numpy()
        assert flags.shape == want_flags.shape and first.dtype == np.int32
        assert np.array_equal(flags, want_flags), (mode, np.argwhere(flags != want_flags)[:5])
        assert np.array_equal(first, want_first), (mode, np.argwhere(first != want_first)[:5])
        only = eng.collision_matrix(torch.from_numpy(cv), torch.from_numpy(ov) if ov is not None else torch.zeros(0, Ts, 4, 2, dtype=torch.float64),
                                    Ts=Ts, mode=mode).cpu().numpy()
        assert np.array_equal(only, want_flags), mode                      # (without first_actor: the same flags)
        out[mode] = (flags, first)
    return out


def _scene(seed, G, Tc, Ts, N, span=2000.0):
    """Seeded rectangles at CARLA magnitudes: per step one place, G candidates and N neighbours within a few metres of it; the candidate
    rows j >= Ts hold NaN (they must not be read)."""
    g = np.random.default_rng(seed)
    cv, ov = np.full((G, Tc, 4, 2), np.nan, dtype=np.float32), np.empty((N, Ts, 4, 2))
    for j in range(Ts):
        centre = g.uniform(-span, span, 2)
        cv[:, j] = F._boxes(g, centre, G).astype(np.float32)
        ov[:, j] = F._boxes(g, centre, N)
    return cv, ov


def test_known_answer_pairs_one_thread_each(eng):
    """G = 1, Ts = 1, N = 1: the flag and first_actor of every known-answer pair are the exact answer, in both modes."""
    for name, P, Q, hit, env in F.known_pairs():
        got = _check(eng, P[None, None].copy(), Q[None, None].copy(), 1)
        assert (bool(got["footprint"][0][0, 0]), int(got["footprint"][1][0, 0])) == (hit, 0 if hit else -1), name
        assert (bool(got["envelope"][0][0, 0]), int(got["envelope"][1][0, 0])) == (env, 0 if env else -1), name


@pytest.mark.parametrize("G,Tc,Ts,N", [(7, 80, 40, 3), (32, 8, 8, 5), (257, 1, 1, 4)])
def test_block_edges_and_unread_rows(eng, G, Tc, Ts, N):
    """280 threads (a partial second block, Tc > Ts with NaN behind Ts), exactly 256, and 257 with one step."""
    cv, ov = _scene(100 + G, G, Tc, Ts, N)
    got = _check(eng, cv, ov, Ts)
    foot, env = got["footprint"][0], got["envelope"][0]
    assert foot.any() and not foot.all() and (env & ~foot).any() and not (foot & ~env).any()


def test_no_neighbours_null_pointer(eng):
    cv, _ = _scene(5, 7, 80, 40, 1)
    for mode in ("footprint", "envelope"):
        flags, first = eng.collision_matrix(torch.from_numpy(cv), torch.zeros(0, 40, 4, 2, dtype=torch.float64), Ts=40, mode=mode, want_first=True)
        assert flags.shape == (7, 40) and not bool(flags.any()) and bool((first == -1).all())
    _check(eng, cv, None, 40)


def test_first_actor_is_the_lowest_hitting_index(eng):
    """N = 17 where only actor 16 hits, and two hitting actors behind a clear one."""
    pairs = {n: (P, Q) for n, P, Q, _, _ in F.known_pairs()}
    P, hit_q = pairs["overlapping"]
    near_miss = pairs["diamonds offset diagonally"][1] + np.array([3.0625, 1.5])     # a diamond 2^-4 off P's corner (4, 2): the envelopes meet
    far = hit_q + 50.0
    cv = np.broadcast_to(P, (3, 2, 4, 2)).copy()
    ov = np.stack([near_miss if n % 2 else far for n in range(16)] + [hit_q])[:, None].repeat(2, 1)
    got = _check(eng, cv, ov, 2)
    assert (got["footprint"][1] == 16).all() and got["footprint"][0].all()
    assert (got["envelope"][1] == 1).all()                                             # (the near miss is the envelope test's first hit)
    ov = np.stack([far, near_miss, hit_q, far, hit_q])[:, None].repeat(2, 1)
    got = _check(eng, cv, ov, 2)
    assert (got["footprint"][1] == 2).all() and (got["envelope"][1] == 1).all()


def test_random_rectangles_as_one_problem(eng):
    cv, ov = F.random_problem()
    G, Ts, N = F.RANDOM_SHAPE
    got = _check(eng, cv, ov, Ts)
    assert not (got["footprint"][0] & ~got["envelope"][0]).any()
    # every pair on its own as well: neighbour n alone against every candidate
    from rift_amd.planning.fine_tuner.rlft.traj_eval import footprint
    pairwise = footprint.pair_collides(cv[:, None], ov[None], "footprint")            # (G, N, Ts)
    for n in range(N):
        flags = eng.collision_matrix(torch.from_numpy(cv), torch.from_numpy(ov[n:n + 1].copy()), Ts=Ts, mode="footprint").cpu().numpy()
        assert np.array_equal(flags, pairwise[:, n]), n


def test_envelope_without_first_actor_is_the_kernel_and_the_bits_of_before(eng):
    cv, ov = _scene(77, 7, 80, 40, 3)
    before = eng.collision_matrix(torch.from_numpy(cv), torch.from_numpy(ov), Ts=40)
    eng.prof_enable(True)
    try:
        got = eng.collision_matrix(torch.from_numpy(cv), torch.from_numpy(ov), Ts=40, mode="envelope")
        torch.cuda.synchronize()
        assert {k: v["count"] for k, v in eng.prof_report().items()} == {"collision_matrix_kernel": 1}
        eng.prof_enable(True)
        eng.collision_matrix(torch.from_numpy(cv), torch.from_numpy(ov), Ts=40, mode="envelope", want_first=True)
        eng.collision_matrix(torch.from_numpy(cv), torch.from_numpy(ov), Ts=40, mode="footprint")
        torch.cuda.synchronize()
        assert {k: v["count"] for k, v in eng.prof_report().items()} == {"footprint_collision_kernel": 2}
    finally:
        eng.prof_enable(False)
    assert got.dtype == torch.bool and torch.equal(got, before)


# ---- the tick -------------------------------------------------------------------------------------------------------------------------
TICK_GAMMA = 0.95


def _raster():
    mask = np.ones((400, 400), dtype=np.uint8)
    mask[150:250, :300] = 0
    return mask


@functools.lru_cache(maxsize=None)
def _tick_world():
    """K = 9 (two chunks, 8 + 1) in rows of Rb = 2 with R = 1 or 2; CBVs 0, 3, 6 have no neighbours, the others four each along their
    corridor, 2 to 4.5 m to the side at up to 25 degrees to it; some CBVs carry a raster, the others no off-road flags."""
    traj = torch.zeros(9, 2, 12, 80, 6)
    cbvs = []
    for k in range(9):
        R = 2 if k % 2 else 1
        tr, ref_pos, ref_ang, st = H.rollout_inputs(2300 + k, R=R)
        pos, heading, speed = (10.0 + 3.0 * k, -5.0 + 2.0 * k), 0.3 + 0.35 * k, 6.0 + 0.2 * k
        traj[k, :R] = tr
        a = None
        if k % 3 != 0:
            a = H.other_vehicle_inputs(seed=700 + k, N=4)
            g = np.random.default_rng(k)
            ahead, side = 5.0 + 7.0 * np.arange(4) + g.uniform(-1, 1, 4), g.uniform(2.0, 4.5, 4) * g.choice([-1.0, 1.0], 4)
            ch, sh = np.cos(heading), np.sin(heading)
            a["location"] = np.stack([pos[0] + ahead * ch - side * sh, -(pos[1] + ahead * sh + side * ch), np.full(4, 0.1)], -1)
            a["yaw_deg"] = -np.degrees(heading) + g.uniform(-25, 25, 4)
            a["speed"] = g.uniform(0.0, 3.0, 4)
        pose = (pos[0], pos[1], heading)
        cbvs.append({"batch_index": k, "center_state": (pos[0], pos[1], heading, speed, st["width"], st["length"]),
                     "ref_pos": [p.numpy() for p in ref_pos], "ref_angle": [x.numpy() for x in ref_ang], "ref_pos_t": ref_pos, "ref_angle_t": ref_ang,
                     "traj": tr, "actors": a, "off_road": (_raster(), pose) if k % 4 == 1 else None})
    return traj, cbvs


def _tick_raw(eng, ffi, entry, collision=None):
    """One of the tick entries called directly on the packed world, on a fresh PID state: (rc, advantage | returns | terms as numpy, the launch record)."""
    from rift_amd import tick_pack
    traj, cbvs = _tick_world()
    dev_traj = traj.cuda()
    blob, layout = tick_pack.pack_tick(cbvs)
    up = eng.stage(blob, torch.uint8)
    arr = tick_pack.fill_tick_cbvs(layout, up.data_ptr())
    pid = eng.new_pid_state(256)
    K, Rb = traj.shape[:2]
    out = {k: torch.zeros(K, Rb, 12, *s, dtype=torch.float64, device="cuda:0") for k, s in (("advantage", ()), ("returns", ()), ("terms", (8,)))}
    params = eng.eval_params(gamma=TICK_GAMMA)
    p = ffi._ptr
    tail = [C.byref(params)] + ([] if collision is None else [C.byref(collision)]) + [p(out["advantage"]), p(out["returns"]), p(out["terms"]), None]
    eng.prof_enable(True)
    try:
        rc = getattr(eng.lib, entry)(eng.ctx, p(dev_traj), Rb, 80, arr, K, *(p(pid[k]) for k in ("turn_buf", "turn_ptr", "turn_len", "speed_buf", "speed_ptr", "speed_len")),
                                     *tail)
        torch.cuda.synchronize()
        record = {k: v["count"] for k, v in eng.prof_report().items()}
    finally:
        eng.prof_enable(False)
    return rc, {k: v.cpu().numpy() for k, v in out.items()}, record


def test_tick_envelope_is_the_map_entry_bit_for_bit_with_its_launches(eng, ffi):
    """(a) K = 9, R in {1, 2}, CBVs without neighbours: ENVELOPE through riftfp_group_advantage_tick against riftdm_group_advantage_tick."""
    rc0, want, rec0 = _tick_raw(eng, ffi, "riftdm_group_advantage_tick")
    rc1, got, rec1 = _tick_raw(eng, ffi, "riftfp_group_advantage_tick", ffi.collision_params("envelope"))
    assert (rc0, rc1) == (0, 0)
    for key in ("advantage", "returns", "terms"):
        assert got[key].tobytes() == want[key].tobytes(), key
    assert rec1 == rec0 and rec0["tick_multi_kernel_3"] == 2 and "tick_multi_kernel_8" not in rec0 and rec0["rollout8_kernel"] == 9
    assert want["terms"][..., 0].min() < 0 and want["returns"].any()


def test_tick_footprint_is_the_composition_of_the_separate_entries(eng, ffi):
    """(c) FOOTPRINT through the fused tick against ref-line info, rollout, neighbour forecast, riftfp_collision_matrix, off-road lookup and
    rift_rollout_return_ex composed per CBV, in tick order on one PID state: advantage, returns and terms bit for bit.  Stage 8 stands in
    for stage 3 and every other launch is the envelope tick's; some candidate's collision term differs between the two modes."""
    from rift_amd.planning.fine_tuner.rlft.traj_eval.traj_evaluator import TrajEvaluator
    rc, got, rec = _tick_raw(eng, ffi, "riftfp_group_advantage_tick", ffi.collision_params("footprint"))
    _, env, rec_env = _tick_raw(eng, ffi, "riftfp_group_advantage_tick", ffi.collision_params("envelope"))
    assert rc == 0
    assert rec["tick_multi_kernel_8"] == 2 and "tick_multi_kernel_3" not in rec
    assert {k: v for k, v in rec.items() if k != "tick_multi_kernel_8"} == {k: v for k, v in rec_env.items() if k != "tick_multi_kernel_3"}
    chain = TrajEvaluator(eng, gamma=TICK_GAMMA, collision="footprint")
    _, cbvs = _tick_world()
    for k, v in enumerate(cbvs):
        R = len(v["ref_pos"])
        kw = {"return_terms": True}
        if v["off_road"] is None:
            kw["off_road_matrix"] = np.zeros((12 * R, 80), dtype=np.bool_)
        else:
            kw["off_road_mask"], kw["center_pose"] = v["off_road"]
        if v["actors"] is None:
            kw["collision_matrix"] = np.zeros((12 * R, 40), dtype=np.bool_)
        else:
            kw["nearby_actor_states"] = v["actors"]
        want = chain.get_grpo_advantage(v["center_state"], v["traj"].cuda(), v["ref_pos_t"], v["ref_angle_t"], **kw)
        for key in ("advantage", "returns", "terms"):
            assert want[key].tobytes() == got[key][k, :R].tobytes(), (k, key)
            assert not got[key][k, R:].any(), (k, key)
    col_f, col_e = got["terms"][..., 0], env["terms"][..., 0]
    differ = int((col_f != col_e).sum())
    print(f"tick: collision term nonzero for {int((col_e != 0).sum())} candidates under the envelope test, {int((col_f != 0).sum())} under the "
          f"footprint test; {differ} candidates differ")
    assert differ > 0 and (col_f != 0).any() and ((col_f == 0) | (col_e != 0)).all()       # footprint <= envelope, candidate by candidate


def test_lane_neighbour_scene_through_the_engine(eng):
    """(b) K = 1, R = 1: a CBV heading 45 degrees, a stationary neighbour parallel to it one lane away.  FOOTPRINT: no candidate pays the
    collision term and every one counts all 40 steps; ENVELOPE: every candidate pays it."""
    traj, entry, _ = F.lane_scene()
    res = {}
    for mode in ("footprint", "envelope"):
        eng.prof_enable(True)
        try:
            r = eng.group_advantage_tick(traj.cuda(), [entry], eng.new_pid_state(256), collision=mode, want_returns=True, want_terms=True)
            torch.cuda.synchronize()
            rec = {k: v["count"] for k, v in eng.prof_report().items()}
        finally:
            eng.prof_enable(False)
        assert (rec.get("tick_multi_kernel_8"), rec.get("tick_multi_kernel_3")) == ((1, None) if mode == "footprint" else (None, 1))
        res[mode] = r["terms"].cpu().numpy()
    assert res["footprint"].shape == (1, 1, 12, 8)
    assert (res["footprint"][..., 0] == 0).all() and (res["footprint"][..., 7] == 40).all()
    assert (res["envelope"][..., 0] < 0).all()
    # without `collision` the call is the one of before, and 'envelope' gives its bits
    plain = eng.group_advantage_tick(traj.cuda(), [entry], eng.new_pid_state(256), params=eng.eval_params(), want_returns=True, want_terms=True)
    assert plain["terms"].cpu().numpy().tobytes() == res["envelope"].tobytes()


def test_footprint_tick_together_with_the_drivable_area_map(ffi):
    """The lane-neighbour scene with off-road flags from a loaded map -- a strip whose right edge lies 0.6 m to the right of the CBV's line: the
    candidates fan out to 0 .. 0.94 m to the right, so at 0.1 m per pixel the six straightest stay on it and the two right-most leave it.
    FOOTPRINT through riftfp_group_advantage_tick with the CBV's flags from the map against the same call with the mask riftdm_raster drew
    uploaded -- bit for bit; stage 7 and stage 8 stand in for stages 4 and 3."""
    traj, entry, _ = F.lane_scene()
    x, y, h = F.LANE_POSE
    along, left = np.array([np.cos(h), np.sin(h)]), np.array([-np.sin(h), np.cos(h)])
    strip = np.array([x, y]) + np.array([-10 * along - 0.6 * left, 60 * along - 0.6 * left, 60 * along + 10 * left, -10 * along + 10 * left])
    e = ffi.Engine("cuda:0")
    try:
        e.load_drivable_map([strip])
        params = e.eval_params(resolution=0.1)
        mask = e.drivable_raster(F.LANE_POSE, (600, 600), params).cpu().numpy()
        got = {}
        for how, d in (("map", dict(entry, raster=(600, 600), pose=F.LANE_POSE)), ("mask", dict(entry, off_road=(mask, F.LANE_POSE)))):
            e.prof_enable(True)
            try:
                r = e.group_advantage_tick(traj.cuda(), [d], e.new_pid_state(256), params=params, collision="footprint", want_returns=True, want_terms=True)
                torch.cuda.synchronize()
                rec = {k: v["count"] for k, v in e.prof_report().items()}
            finally:
                e.prof_enable(False)
            assert rec.get("tick_multi_kernel_8") == 1 and "tick_multi_kernel_3" not in rec
            assert ("tick_multi_kernel_7" in rec, "tick_multi_kernel_4" in rec) == ((True, False) if how == "map" else (False, True))
            got[how] = {k: r[k].cpu().numpy() for k in ("advantage", "returns", "terms")}
        for key in ("advantage", "returns", "terms"):
            assert got["map"][key].tobytes() == got["mask"][key].tobytes(), key
        off = got["map"]["terms"][0, 0, :, 1]
        print(f"lane scene on the strip: off-road term nonzero for {int((off != 0).sum())} of 12 candidates; drivable share of the raster {float((mask == 0).mean()):.2f}")
        assert (got["map"]["terms"][..., 0] == 0).all() and 0.0 < float((mask == 0).mean()) < 1.0
        assert (off[:6] == 0).all() and (off[10:] != 0).all()
    finally:
        e.close()


def test_refusals_through_the_engine_launch_nothing(eng, ffi):
    """A bad mode, reserved != 0 and NULL params: RIFT_ERR_ARG with a message that names the entry, decided ahead of the wrapped entry's
    own refusals; nothing is launched and nothing written."""
    from rift_amd import _abi
    cv, ov = _scene(9, 7, 40, 40, 3)
    dcv, dov = torch.from_numpy(cv).cuda(), torch.from_numpy(ov).cuda()
    flags = torch.full((7, 40), 7, dtype=torch.uint8, device="cuda:0")
    first = torch.full((7, 40), 7, dtype=torch.int32, device="cuda:0")
    p, lib, ctx = ffi._ptr, eng.lib, eng.ctx
    bad_mode, bad_res = ffi.RiftCollisionParams(2, 0), ffi.RiftCollisionParams(1, 1)

    def err():
        return (lib.rift_last_error(ctx) or b"").decode()

    eng.prof_enable(True)
    try:
        for params, why in ((C.byref(bad_mode), "mode outside {0, 1}"), (C.byref(bad_res), "reserved != 0"), (None, "params == NULL")):
            rc = lib.riftfp_collision_matrix(ctx, p(dcv), 7, 40, p(dov), 3, 40, params, p(flags), p(first), None)
            assert rc == _abi.RIFT_ERR_ARG and err().startswith("riftfp_collision_matrix: ") and why in err(), err()
            rc = lib.riftfp_collision_matrix(ctx, p(dcv), 0, 40, p(dov), 3, 40, params, p(flags), p(first), None)          # (ahead of G <= 0)
            assert rc == _abi.RIFT_ERR_ARG and why in err(), err()
            rc = lib.riftfp_group_advantage_tick(ctx, None, 1, 80, None, 0, None, None, None, None, None, None, C.byref(eng.eval_params()), params,
                                                 None, None, None, None)
            assert rc == _abi.RIFT_ERR_ARG and err().startswith("riftfp_group_advantage_tick: ") and why in err(), err()
        rc = lib.riftfp_collision_matrix(ctx, p(dcv), 0, 40, p(dov), 3, 40, C.byref(ffi.collision_params("footprint")), p(flags), p(first), None)
        assert rc == _abi.RIFT_ERR_ARG and "G <= 0" in err() and err().startswith("riftfp_collision_matrix: ")
        with pytest.raises(RuntimeError, match=r"riftfp_collision_matrix failed \(-1\).*mode outside"):
            eng.collision_matrix(dcv, dov, Ts=40, mode=bad_mode)
        with pytest.raises(RuntimeError, match=r"riftfp_group_advantage_tick failed \(-1\).*reserved != 0"):
            traj, entry, _ = F.lane_scene()
            eng.group_advantage_tick(traj.cuda(), [entry], eng.new_pid_state(256), collision=bad_res)
        with pytest.raises(ValueError, match="known.*envelope.*footprint"):
            eng.collision_matrix(dcv, dov, Ts=40, mode="sat")
        torch.cuda.synchronize()
        assert eng.prof_report() == {}
    finally:
        eng.prof_enable(False)
    assert int(flags.min()) == 7 and int(flags.max()) == 7 and int(first.min()) == 7 and int(first.max()) == 7
