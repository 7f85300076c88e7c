"""The evaluator's run-time parameters on the device, through the C-ABI: rift_rollout_return_ex and rift_group_advantage_tick_ex with
non-default reward weights, the sparse model, gamma, bbox_inflation_ratio, near_lane_change, resolution and rasters that are not 400 x 400,
the per-term breakdown, and the policies' `traj_eval` configuration.  The references are oracle.advantage with its weight dict patched and
the restatements of tests/eval_param_cases.py; tests/test_eval_params_host.py checks on the CPU that every parameter shows on these inputs.
Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import eval_param_cases as E
from tests import helpers as H
from tests import small_kernel_cases as K

pytestmark = pytest.mark.gpu

RR_GS, RR_TS = (1, 5, 9), (1, 40, 64, 65, 130)
MODELS = tuple(E.SETS) + tuple("sparse_" + n for n in E.SPARSE)
FLOATS = ("delta_dis", "delta_angle", "speed", "acc", "ang_vel", "ang_acc")


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


def _model(name):
    from rift_amd.gym_carla.reward.reward_model import DenseRewardModel, SparseRewardModel
    if name.startswith("sparse_"):
        return SparseRewardModel(**E.SPARSE[name[7:]])
    return DenseRewardModel(**{k: E.SETS[name][k] for k in E.moved(E.SETS[name])})


def _cases():
    return [(G, Ts, s) for G in RR_GS for s, Ts in enumerate(RR_TS)]


@functools.lru_cache(maxsize=None)
def _reference(name, G, Ts, s):
    """(returns (G,), terms (G, 8)) of one model on one case, computed once and shared; the case's flags cut to the horizon."""
    c = K.rollout_return_case(G, Ts, s)
    cc = dict(c, collision=c["collision"][:, :Ts], off_road=c["off_road"][:, :Ts])
    if name.startswith("sparse_"):
        w = E.SPARSE[name[7:]]
        return E.sparse_return(w, cc, K.RR_GAMMA), E.terms_ref(w, cc, K.RR_GAMMA, sparse=True)
    return E.dense_return(E.SETS[name], c, K.RR_GAMMA), E.terms_ref(E.SETS[name], cc, K.RR_GAMMA)


def _run(eng, c, **kw):
    T = torch.from_numpy
    return eng.rollout_return(*[T(c[k]) for k in FLOATS], c["collision"], c["off_road"], gamma=K.RR_GAMMA, **kw)


def _bar(ref):
    return 1e-5 * max(1.0, float(np.max(np.abs(ref))))


def test_rollout_return_with_run_time_reward_models(eng):
    """rift_rollout_return_ex for G = 1, 5, 9 and Ts = 1, 40, 64, 65, 130 (one to three rounds of 64 steps, flags wider than the horizon,
    every collision placement), gamma 0.93, under the three dense weight sets (every weight off its default, one with a centre bias) and
    the sparse model with the reference's and with edited weights: against oracle.advantage.rollout_return with P patched -- for the sparse
    model the three-line restatement of eval_param_cases.sparse_return -- to 1e-5 max(1, max |ref|), the bar of test_gpu_small_kernels.
    Measured on MI355X: the worst error over all models and shapes is 1.5e-2 of its bar."""
    worst = 0.0
    for name in MODELS:
        for G, Ts, s in _cases():
            c = K.rollout_return_case(G, Ts, s)
            ref, _ = _reference(name, G, Ts, s)
            got = _run(eng, c, reward_model=_model(name)).cpu().numpy()
            e = float(np.max(np.abs(got - ref)))
            worst = max(worst, e / _bar(ref))
            assert np.isfinite(got).all() and e < _bar(ref), (name, G, Ts, e, _bar(ref))
    print(f"rollout_return_ex: worst error / bar {worst:.2e}")


def test_dense_reward_thresholds_under_other_weights(eng):
    """REWARD_KAT (one step, inputs exactly on the reward's thresholds) with each of the three weight sets against
    oracle.advantage.dense_reward with P patched: 1e-6 absolute, the bar used there for the defaults."""
    kat = np.array(K.REWARD_KAT, dtype=np.float64)
    col = lambda j: np.ascontiguousarray(kat[:, j:j + 1].astype(np.float32))  # noqa: E731
    c = {"delta_dis": col(0), "delta_angle": col(1), "speed": col(2), "acc": col(3), "ang_vel": np.zeros((len(kat), 1), np.float32),
         "ang_acc": col(4), "collision": kat[:, 5:6] != 0, "off_road": kat[:, 6:7] != 0}
    for name, weights in E.SETS.items():
        got = _run(eng, c, reward_model=_model(name)).cpu().numpy()
        with E.patched_P(weights):
            ref = K.reward_kat_ref()
        assert float(np.max(np.abs(ref - K.reward_kat_ref()))) > 1e-3          # (the set does move these rows)
        for row, a, b in zip(K.REWARD_KAT, got, ref):
            assert abs(a - b) < 1e-6, (name, row, a, b)


def test_default_parameters_give_the_old_entrys_bits(eng, ffi):
    """rift_rollout_return_ex with rift_eval_params_default (gamma set to the call's) returns the bytes of rift_rollout_return on every
    case, and the same bytes again when `terms` is asked for; the library's defaults are the binding's."""
    p = ffi.RiftEvalParams()
    assert eng.lib.rift_eval_params_default(eng.ctx, C.byref(p)) == 0
    assert bytes(memoryview(p)) == bytes(memoryview(ffi.eval_params()))
    p.gamma = K.RR_GAMMA
    for G, Ts, s in _cases():
        c = K.rollout_return_case(G, Ts, s)
        old = _run(eng, c).cpu().numpy()
        new = _run(eng, c, reward_model=p).cpu().numpy()
        with_terms, _ = _run(eng, c, reward_model=p, terms=True)
        assert old.tobytes() == new.tobytes() == with_terms.cpu().numpy().tobytes(), (G, Ts)
    for name in MODELS:                                   # ... and with other weights the return does not depend on `terms` either
        c = K.rollout_return_case(9, 130, 0)
        a = _run(eng, c, reward_model=_model(name)).cpu().numpy()
        b, _ = _run(eng, c, reward_model=_model(name), terms=True)
        assert a.tobytes() == b.cpu().numpy().tobytes(), name


def test_reward_terms_per_candidate(eng):
    """`terms` of rift_rollout_return_ex on the same cases and models: columns 0-6 against the per-term restatement
    (eval_param_cases.dense_terms, whose sum is first held to oracle.advantage.dense_reward at 1e-12, step by step) at the bar of the
    returns; column 7, the steps counted, exactly; columns 2-6 exactly 0 for the sparse model; and the terms add up to the return:
    |sum(terms[:7]) - return| <= 1e-9 max(1, |return|) (at most 7 x 130 fp64 addends of magnitude <= ~60: ~6e-12)."""
    for name in MODELS:
        for G, Ts, s in _cases():
            c = K.rollout_return_case(G, Ts, s)
            ref, tref = _reference(name, G, Ts, s)
            ret, terms = _run(eng, c, reward_model=_model(name), terms=True)
            ret, terms = ret.cpu().numpy(), terms.cpu().numpy()
            assert terms.shape == (G, 8) and np.isfinite(terms).all()
            assert np.array_equal(terms[:, 7], tref[:, 7]), (name, G, Ts)
            assert float(np.max(np.abs(terms[:, :7] - tref[:, :7]))) < _bar(ref), (name, G, Ts)
            assert np.all(np.abs(terms[:, :7].sum(1) - ret) <= 1e-9 * np.maximum(1.0, np.abs(ret))), (name, G, Ts)
            if name.startswith("sparse_"):
                assert not terms[:, 2:7].any()


# ---- the tick -------------------------------------------------------------------------------------------------------------------------
TICK_WEIGHTS = dict(E.SETS["B"], alpha_collision=12.0, alpha_boundary=9.0, alpha_velocity=0.37)
TICK_GAMMA, TICK_INFLATION, TICK_RES = 0.93, 1.3, 0.25


def _raster(shape):
    """A drivable band around the raster's centre ROW as the reference places it -- pixel y = -y / res + W / 2, pixel x = x / res + H / 2 --
    +-7 m wide, from behind the start pose to 40 m ahead of it at 0.25 m per pixel."""
    Hh, Ww = shape
    mask = np.ones(shape, dtype=np.uint8)
    row, col0 = Ww // 2, Hh // 2
    mask[max(row - 28, 0):row + 28, :min(col0 + 160, Ww)] = 0
    return mask


def _neighbours(seed, st, N=4):
    """Actors along the candidates' corridor (CARLA frame: y and yaw flipped), two of them slower than the 1 m/s extent threshold."""
    a = H.other_vehicle_inputs(seed=seed, N=N)
    g = np.random.default_rng(seed)
    ahead, side = 6.0 + 7.0 * np.arange(N) + g.uniform(-1, 1, N), g.uniform(-4.0, 4.0, N)
    ch, sh = np.cos(st["heading"]), np.sin(st["heading"])
    gx, gy = st["pos"][0] + ahead * ch - side * sh, st["pos"][1] + ahead * sh + side * ch
    a["location"] = np.stack([gx, -gy, np.full(N, 0.1)], -1)
    a["yaw_deg"] = -np.degrees(st["heading"]) + g.uniform(-20, 20, N)
    return a


@functools.lru_cache(maxsize=None)
def _tick_world():
    """Two ticks: K = 3 with R = (1, 3, 2) in rows of Rb = 3, and K = 9 with R = 1 each in rows of Rb = 2 (past RIFT_TICK_CHUNK = 8).  Among
    the CBVs some have no neighbours, some no raster, two a 200 x 300 raster."""
    ticks = []
    for t, (Rs, Rb) in enumerate((((1, 3, 2), 3), ((1,) * 9, 2))):
        traj = torch.zeros(len(Rs), Rb, 12, 80, 6)
        cbvs = []
        for k, R in enumerate(Rs):
            tr, ref_pos, ref_ang, st = H.rollout_inputs(940 + 16 * t + k, R=R)
            st = dict(st, pos=(10.0 + k, -5.0 + 0.5 * t), heading=0.3 - 0.05 * k, speed=6.0 + 0.2 * k)
            traj[k, :R] = tr
            odd = (t, k) in ((0, 1), (1, 5))
            no_raster = (t, k) == (0, 2) or (t == 1 and k % 4 == 1 and not odd)
            no_nb = (t, k) == (0, 0) or (t == 1 and k % 3 == 0)
            pose = (st["pos"][0], st["pos"][1], st["heading"])
            cbvs.append({"batch_index": k, "center_state": (st["pos"][0], st["pos"][1], st["heading"], st["speed"], st["width"], st["length"]),
                         "ref_pos": [p.numpy() for p in ref_pos], "ref_angle": [a.numpy() for a in ref_ang], "st": st, "traj": tr,
                         "ref_pos_t": ref_pos, "ref_angle_t": ref_ang,
                         "actors": None if no_nb else _neighbours(300 + 16 * t + k, st),
                         "off_road": None if no_raster else (_raster((200, 300) if odd else (400, 400)), pose)})
        ticks.append((traj, cbvs))
    return ticks


def _chain_kwargs(v, G):
    kw = {"near_lane_change": False, "return_terms": True}
    if v["off_road"] is None:
        kw["off_road_matrix"] = np.zeros((G, 80), dtype=np.bool_)
    else:
        kw["off_road_mask"], kw["center_pose"] = v["off_road"]
    if v["actors"] is None:
        kw["collision_matrix"] = np.zeros((G, 40), dtype=np.bool_)
    else:
        kw["nearby_actor_states"] = v["actors"]
    return kw


def test_tick_ex_equals_the_evaluator_chain_and_the_oracle(eng, ffi):
    """rift_group_advantage_tick_ex with non-default weights (a centre bias among them), gamma 0.93, bbox_inflation_ratio 1.3,
    near_lane_change 0 and resolution 0.25 on two ticks of one evaluator (K = 3 with R = 1, 3, 2; K = 9 past RIFT_TICK_CHUNK; CBVs without
    neighbours, without a raster, with a 200 x 300 raster) against the per-CBV TrajEvaluator chain with the same settings from a clone of
    the PID state: advantage, returns and terms equal bit for bit, rows r >= R untouched, and the same advantage bits without the
    breakdown.  Then the chain against the oracle chain with P patched (one oracle controller carried through all twelve CBVs): first
    every collision / off-road flag equal, then the z-scores to 2e-5 (measured on MI355X: 4.3e-6 worst; 8 CBVs with mixed collision flags, 9
    with mixed off-road flags).  The 200 x 300 raster's drivable band lies around pixel row
    W / 2 = 150, where the reference's offset (H / 2 to x, W / 2 to y) puts the start pose: with H and W swapped in the offset the
    oracle's own flags of those CBVs change (asserted here), so a swapped offset in the kernels' caller turns this test red."""
    from oracle import advantage as oadv, rollout as orl, traj_flags as otf
    from rift_amd.gym_carla.reward.reward_model import DenseRewardModel
    from rift_amd.planning.fine_tuner.rlft.traj_eval.traj_evaluator import TrajEvaluator
    model = DenseRewardModel(**{k: TICK_WEIGHTS[k] for k in E.moved(TICK_WEIGHTS)})
    params = eng.eval_params(model, TICK_GAMMA, TICK_INFLATION, TICK_RES, near_lane_change=False)
    fused = TrajEvaluator(eng)
    chain = TrajEvaluator(eng, bbox_inflation_ratio=TICK_INFLATION, resolution=TICK_RES, reward_model=model, gamma=TICK_GAMMA)
    plain = TrajEvaluator(eng)
    oracle_ro = orl.Rollout()
    seen = {"col": 0, "off": 0, "odd": 0}
    worst = 0.0
    for traj, cbvs in _tick_world():
        K_, Rb = traj.shape[:2]
        res = eng.group_advantage_tick(traj.cuda(), cbvs, fused.pid_state, params=params, want_returns=True, want_terms=True)
        adv, ret, terms = (res[k].cpu().numpy() for k in ("advantage", "returns", "terms"))
        only = eng.group_advantage_tick(traj.cuda(), cbvs, plain.pid_state, params=params).cpu().numpy()
        assert only.tobytes() == adv.tobytes()
        for k, v in enumerate(cbvs):
            R = len(v["ref_pos"])
            G = 12 * R
            if v["off_road"] is not None:
                chain.map_height, chain.map_width = v["off_road"][0].shape
            got = chain.get_grpo_advantage(v["center_state"], v["traj"].cuda(), v["ref_pos_t"], v["ref_angle_t"], **_chain_kwargs(v, G))
            assert got["advantage"].tobytes() == adv[k, :R].tobytes(), k
            assert got["returns"].tobytes() == ret[k, :R].tobytes() and got["terms"].tobytes() == terms[k, :R].tobytes(), k
            assert not adv[k, R:].any() and not ret[k, R:].any() and not terms[k, R:].any()
            assert np.array_equal(terms[k, :R, :, 7], np.rint(terms[k, :R, :, 7])) and terms[k, :R, :, 7].min() >= 1 and terms[k, :R, :, 7].max() <= 40
            # ---- the oracle chain on its own rollout
            st, ro_dev = v["st"], chain.last_rollout
            t40 = v["traj"][:, :, :40, :]
            dd, da, _ = orl.ref_line_info(t40, v["ref_pos_t"], v["ref_angle_t"])
            gpos, ghead = orl.to_global(t40, torch.tensor(st["pos"]), torch.tensor(st["heading"]))
            ref = oracle_ro.propagate(gpos, ghead, st["speed"], st["width"], st["length"])
            col, off = np.zeros((G, 40), dtype=bool), np.zeros((G, 80), dtype=bool)
            if v["actors"] is not None:
                other = otf.get_other_vehicle_rollout(num_future_frames=40, near_lane_change=False, bbox_inflation_ratio=TICK_INFLATION, **v["actors"])
                col = otf.get_collision_matrix(ref["vertices"].numpy(), other)
                other_dev = eng.other_vehicle_rollout(near_lane_change=False, bbox_inflation_ratio=TICK_INFLATION, **v["actors"])
                assert np.array_equal(eng.collision_matrix(ro_dev["vertices"], other_dev, Ts=40).cpu().numpy(), col), k
            if v["off_road"] is not None:
                mask, pose = v["off_road"]
                Hh, Ww = mask.shape
                off = otf.get_off_road_matrix(ref["center"].numpy(), mask, pose[:2], pose[2], map_width=Ww, map_height=Hh, resolution=TICK_RES)
                off_dev = eng.off_road_matrix(ro_dev["center"], mask, pose[:2], pose[2], resolution_hw=(TICK_RES, -TICK_RES), offset=(Hh / 2, Ww / 2))
                assert np.array_equal(off_dev.cpu().numpy(), off), k
                if Hh != Ww:
                    swapped = otf.get_off_road_matrix(ref["center"].numpy(), mask, pose[:2], pose[2], map_width=Hh, map_height=Ww, resolution=TICK_RES)
                    assert (swapped[:, :40] != off[:, :40]).mean() > 0.25 and off[:, :40].any() and not off[:, :40].all()
                    seen["odd"] += 1
            seen["col"] += int(col.any() and not col.all())
            seen["off"] += int(off[:, :40].any() and not off[:, :40].all())
            with E.patched_P(TICK_WEIGHTS):
                want_ret = oadv.rollout_return(dd.numpy(), da.numpy(), ref["speed"][:, :40].numpy(), ref["acc"][:, :40].numpy(),
                                               ref["ang_vel"][:, :40].numpy(), ref["ang_acc"][:, :40].numpy(), col, off, TICK_GAMMA)
            want = oadv.group_zscore(want_ret).reshape(R, 12)
            e = float(np.max(np.abs(got["advantage"] - want)))
            worst = max(worst, e)
            assert e < 2e-5, (k, e)
    print(f"tick_ex chain vs oracle: worst z-score error {worst:.2e}; CBVs with mixed collision flags {seen['col']}, off-road {seen['off']}")
    assert seen["col"] >= 2 and seen["off"] >= 2 and seen["odd"] == 2


# ---- the policy -----------------------------------------------------------------------------------------------------------------------
class _States:
    """Recorded readings: an oncoming neighbour on the CBV's axis (12 m ahead, 3 m/s towards it, controls released: it sweeps the corridor,
    so candidates collide at different steps or not at all), three seeded ones, and a raster with a drivable band."""

    def center_state(self, env_id, cbv_id):
        from rift_amd.planning.pluto.pluto import CenterState
        return CenterState(10.0 + cbv_id, -5.0, 0.3, 6.0 + 0.1 * cbv_id, 2.0, 4.6)

    def nearby_actor_states(self, env_id, cbv_id):
        a = H.other_vehicle_inputs(seed=100 + cbv_id, N=4)
        gx, gy = 10.0 + cbv_id + 12.0 * np.cos(0.3), -5.0 + 12.0 * np.sin(0.3)
        a["location"][0], a["yaw_deg"][0], a["speed"][0] = (gx, -gy, 0.1), -np.degrees(0.3) + 180.0, 3.0       # (CARLA frame: y and yaw flipped)
        a["steer"][0] = a["throttle"][0] = a["brake"][0] = 0.0
        return a

    def off_road_raster(self, env_id, cbv_id):
        mask = np.ones((400, 400), dtype=np.uint8)
        mask[150:250, :300] = 0
        return mask, (10.0 + cbv_id, -5.0, 0.3)


def test_policy_traj_eval_settings_in_train_mode(tmp_path):
    """RIFTPluto in train mode, two ticks (three CBVs, then two): without config['traj_eval'] and with every key at its default the
    advantages are equal bit for bit; with reward_params = {'alpha_collision': 0.0} they differ; with breakdown: True
    last_tick_breakdown[cbv_id] holds 'returns' (R, 12) and 'terms' (R, 12, 8) whose term sums reproduce the returns (1e-9 max(1, |return|))
    and whose z-scores are the advantages (1e-9); the per-CBV chain (fused_tick False) gives the fused call's bits under the same settings."""
    import rift_amd.synthetic as syn
    from oracle import advantage as oadv
    from rift_amd.planning import CBV_POLICY_LIST
    from rift_amd.planning.pluto.feature_builder.pluto_feature import PlutoFeature
    torch.cuda.set_device(0)
    sd = H.weights()
    explicit = {'gamma': 0.98, 'reward_model': 'dense', 'reward_params': dict(E.DEFAULTS), 'bbox_inflation_ratio': 1.1, 'resolution': 0.5,
                'near_lane_change': True, 'breakdown': False}
    edited = {'reward_params': {'alpha_collision': 0.0}, 'breakdown': True}
    runs = {}
    for name, section, fused in (("none", None, True), ("explicit", explicit, True), ("edited", edited, True), ("edited_chain", edited, False)):
        cfg = {'num_scenario': 1, 'ROOT_DIR': str(tmp_path), 'model_path': 'ckpt', 'device': 'cuda:0', 'state_source': _States(), 'fused_tick': fused}
        if section is not None:
            cfg['traj_eval'] = section
        pol = CBV_POLICY_LIST['rift_pluto'](cfg, None)
        pol.pluto_model.load_state_dict(sd)
        pol.set_mode('train')
        cols = []
        for t, ids in enumerate([[1, 2, 3], [2, 5]]):
            feats = {c: syn.make_scene(7000 + 16 * t + c, num_agents=12, num_polygons=8, r_min=1, r_max=3)["feature"] for c in ids}
            obs = {c: {'raw_pluto_feature': PlutoFeature(data=feats[c])} for c in ids}
            act = pol.get_action([obs], [{'env_id': 0}], deterministic=False)
            for c in ids:
                adv = act['CBVs_group_advantage'][0][c]['advantage']
                R = int(np.asarray(feats[c]["reference_line"]["valid_mask"]).any(-1).sum())
                assert adv.shape == (R, 12) and adv.dtype == np.float64 and np.isfinite(adv).all()
                bd = pol.last_tick_breakdown.get(c)
                assert (bd is not None) == bool(section and section.get('breakdown')) and set(pol.last_tick_breakdown) <= set(ids)
                if bd is not None:
                    ret, terms = bd['returns'], bd['terms']
                    assert ret.shape == (R, 12) and terms.shape == (R, 12, 8) and ret.dtype == terms.dtype == np.float64
                    assert np.all(np.abs(terms[..., :7].sum(-1) - ret) <= 1e-9 * np.maximum(1.0, np.abs(ret)))
                    assert float(np.max(np.abs(oadv.group_zscore(ret.reshape(-1)).reshape(R, 12) - adv))) < 1e-9
                    assert terms[..., 7].min() >= 1 and terms[..., 7].max() <= 40
                    print(f"{name} tick {t} cbv {c}: steps counted {int(terms[..., 7].min())} .. {int(terms[..., 7].max())}, returns {ret.min():.2f} .. {ret.max():.2f}")
                cols.append((adv, bd))
        runs[name] = cols
        pol.pluto_model.release_engine()
    assert any(not np.array_equal(a, c) for (a, _), (c, _) in zip(runs["none"], runs["edited"]))              # the weight shows
    for (a, _), (b, _), (c, bc), (d, bd) in zip(runs["none"], runs["explicit"], runs["edited"], runs["edited_chain"]):
        assert a.tobytes() == b.tobytes()
        assert c.tobytes() == d.tobytes() and bc['returns'].tobytes() == bd['returns'].tobytes() and bc['terms'].tobytes() == bd['terms'].tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(eng, ffi):
    """A NaN weight, reward_model = 2 and resolution = 0 are refused by both _ex entries on the host: RuntimeError with the reason through
    the binding, RIFT_ERR_ARG with it in rift_last_error through the library, and the output tensors keep their fill value."""
    c = K.rollout_return_case(5, 40, 1)
    bad = {"a field is not finite": dict(alpha_comfort=float("nan")), "reward_model outside": dict(reward_model=2), "resolution <= 0": dict(resolution=0.0)}
    f = [torch.from_numpy(c[k]).cuda() for k in FLOATS]
    col, off = torch.from_numpy(c["collision"]).cuda(), torch.from_numpy(c["off_road"]).cuda()
    for why, fields in bad.items():
        p = ffi.eval_params(gamma=K.RR_GAMMA)
        for k, v in fields.items():
            setattr(p, k, v)
        with pytest.raises(RuntimeError, match="rift_rollout_return_ex.*" + why):
            _run(eng, c, reward_model=p)
        traj, cbvs = _tick_world()[0]
        pid = eng.new_pid_state(64)
        with pytest.raises(RuntimeError, match="rift_group_advantage_tick_ex.*" + why):
            eng.group_advantage_tick(traj.cuda(), cbvs, pid, params=p, want_returns=True)
        out, terms = torch.full((5,), 7.5, dtype=torch.float64, device="cuda"), torch.full((5, 8), -3.25, dtype=torch.float64, device="cuda")
        rc = eng.lib.rift_rollout_return_ex(eng.ctx, *[C.c_void_p(t.data_ptr()) for t in f], C.c_void_p(col.data_ptr()), col.shape[1],
                                            C.c_void_p(off.data_ptr()), off.shape[1], 5, 40, C.byref(p), C.c_void_p(out.data_ptr()),
                                            C.c_void_p(terms.data_ptr()), None)
        assert rc == -1 and why in eng.lib.rift_last_error(eng.ctx).decode()
        adv = torch.full((3, 3, 12), 1.5, dtype=torch.float64, device="cuda")
        rc = eng.lib.rift_group_advantage_tick_ex(eng.ctx, None, 3, 80, None, 3, None, None, None, None, None, None, C.byref(p),
                                                  C.c_void_p(adv.data_ptr()), None, None, None)
        assert rc == -1 and why in eng.lib.rift_last_error(eng.ctx).decode()
        torch.cuda.synchronize()
        assert bool((out == 7.5).all()) and bool((terms == -3.25).all()) and bool((adv == 1.5).all())
    rc = eng.lib.rift_rollout_return_ex(eng.ctx, *[None] * 7, 0, None, 0, 5, 40, None, None, None, None)
    assert rc == -1 and "params == NULL" in eng.lib.rift_last_error(eng.ctx).decode()
    assert torch.isfinite(_run(eng, c, reward_model=ffi.eval_params(gamma=K.RR_GAMMA))).all()          # the engine works on after a refusal
