"""riftcs_control_tick (include/rift_select.h) -- the rollout tick's decisions with the executed candidate chosen at run time -- against
rift_control_tick (GREEDY: the same bits), against the host statement of the sampled choice (sample_candidate,
rift_amd/planning/pluto/inference.py) on every case of tests/select_cases.py, and the policy-level setting
(config['action_selection']) on the device path against the host path."""
import ctypes as C

import numpy as np
import pytest
import torch

from rift_amd import synthetic as syn
from rift_amd.planning.pluto import inference as inf
from rift_amd.planning.pluto.controller.pid_controller import PIDController
from rift_amd.planning.pluto.feature_builder.pluto_feature import PlutoFeature
from tests import helpers as H
from tests import select_cases as S

pytestmark = pytest.mark.gpu

INTERVAL = 10
POSE = (12.5, -3.25, 0.6, 4.0)          # x, y, heading, speed of every CBV of a case


@pytest.fixture(scope="module")
def engine():
    from rift_amd import _ffi
    torch.cuda.set_device(0)
    eng = _ffi.Engine("cuda:0")
    yield eng
    eng.close()


def raw_outputs(cand, ref_free=None, scale=1.0):
    """fp32 `trajectory` (R, 12, T, 6) and `ref_free_trajectory` (T, 4) of rift_forward from (x, y, heading) paths, x and y scaled."""
    traj = np.zeros(cand.shape[:-1] + (6,), dtype=np.float32)
    traj[..., 0], traj[..., 1] = cand[..., 0] * scale, cand[..., 1] * scale
    traj[..., 2], traj[..., 3] = np.cos(cand[..., 2]), np.sin(cand[..., 2])
    if ref_free is None:
        return traj, None
    rf = np.stack([ref_free[:, 0] * scale, ref_free[:, 1] * scale, np.cos(ref_free[:, 2]), np.sin(ref_free[:, 2])], -1).astype(np.float32)
    return traj, rf


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host_controls(traj, flat, pose):
    """The host path (trim_candidates' transform + global_to_local + a fresh PIDController) on candidate `flat` of the fp32 `traj`:
    -> [throttle, steer, brake, desired_speed, delta_angle] and the margin of its discontinuous choices (aim point, the two brake tests)."""
    x, y, angle, speed = pose
    a = traj.reshape(-1, traj.shape[-2], 6)[flat].astype(np.float64)
    xyh = np.concatenate([a[:, :2], np.arctan2(a[:, 3], a[:, 2])[:, None]], -1)
    origin = np.array([x, y], dtype=np.float64)
    kept = inf.trim_candidates(xyh[None, None], np.zeros((1, 1), dtype=np.float32), origin, float(angle), None, 1)[0]
    local = inf.global_to_local(kept[0, 1:], origin, float(angle))
    ctrl = PIDController(sample_interval=INTERVAL)
    throttle, steer, brake = ctrl.control_pid(local[:, :2], float(speed))
    pts = local[INTERVAL - 1::INTERVAL, :2]
    aim = min(max(0.5 * speed + 2.5, 5.0), 8.0)
    miss = np.sort(np.abs(np.sqrt((pts[:-1] ** 2).sum(1)) - aim))
    margin = min(miss[1] - miss[0], abs(ctrl.desired_speed - 0.4), abs(speed / ctrl.desired_speed - 1.1))
    return np.array([throttle, steer, float(brake), ctrl.desired_speed, ctrl.delta_angle], dtype=np.float64), margin


def sampled(engine, traj, logits, rf, us, topk, temperature, pose=POSE):
    """One riftcs_control_tick in SAMPLE mode: len(us) CBVs on batch row 0, slots 0.., fresh controllers -> (K, 8) on the host."""
    K = len(us)
    engine.control_state(K).zero_()
    cbvs = [(0, k) + tuple(pose) for k in range(K)]
    dec = engine.control_tick(dev(traj[None]), dev(logits[None]), None if rf is None else dev(rf[None]), cbvs, topk, INTERVAL,
                              select={'mode': 'sample', 'temperature': temperature}, u=us)
    return dec.cpu().numpy()


def test_greedy_mode_is_bitwise_rift_control_tick(engine):
    """GREEDY through the new entry against rift_control_tick on the same inputs and a copy of the same controller state: the decision and
    the state behind the call, at a shape of each kernel instantiation (<2>, <4>, <16>), with and without a ref-free trajectory."""
    for Rb, with_rf in ((4, True), (1, False), (11, True), (22, False)):
        inp = H.inference_inputs(seed=300 + Rb, R=Rb)
        traj, rf = raw_outputs(inp["candidates"], inp["ref_free"] if with_rf else None)
        prob = inp["probability"].copy()
        if Rb == 11:
            prob[3, 7] = 3.5                                           # (a learned choice beside the ref-free fallback of Rb = 4)
        t, p, r = dev(traj[None]), dev(prob[None]), None if rf is None else dev(rf[None])
        cbvs = [(0, 2, 12.5, -3.25, 0.6, 4.0), (0, 5, -40.0, 7.5, -2.1, 0.3), (0, 9, 3.0, 88.0, 1.3, 9.0)]
        engine.control_reset(range(16))
        for _ in range(2):                                             # a state with a history
            engine.control_tick(t, p, r, cbvs, 10, INTERVAL)
        start = engine.control_state(16).clone()
        plain = engine.control_tick(t, p, r, cbvs, 10, INTERVAL).clone()
        plain_state = engine.control_state(16).clone()
        engine.control_state(16).copy_(start)
        for select in ({'mode': 'greedy'}, {'mode': 'greedy', 'temperature': 0.3}, engine_select_default()):
            engine.control_state(16).copy_(start)
            got = engine.control_tick(t, p, r, cbvs, 10, INTERVAL, select=select)
            assert torch.equal(got, plain) and torch.equal(engine.control_state(16), plain_state), (Rb, select)
        assert not torch.equal(plain_state, start)
    engine.control_reset(range(16))


def engine_select_default():
    from rift_amd import _abi_select, _ffi
    p = _abi_select.RiftSelectParams(5, 5, -2.0)
    assert _ffi.load_library().riftcs_params_default(C.byref(p)) == 0
    return p


@pytest.mark.parametrize("name", list(S.CASES))
def test_every_case_matches_the_host_statement(engine, name):
    """One call per case, a CBV per constructed u.  Elements 3 and 4 exactly, element 5 to 1e-6, the controls and the controller's
    diagnostics to 1e-9 of the host path run on the chosen candidate (brake exactly): the bounds tests/test_gpu_control_tick.py gives the
    greedy decision."""
    c = S.case(name)
    us = S.draws(c)
    traj, _ = raw_outputs(H.inference_inputs(seed=500 + c["Rb"], R=c["Rb"])["candidates"])
    want = [inf.sample_candidate(c["logits"], c["topk"], c["temperature"], u) for u in us]
    assert min(S.edge_distance(c["logits"], c["topk"], c["temperature"], u) for u in us) >= S.EDGE_MARGIN
    host = {flat: host_controls(traj, flat, POSE) for flat in {w[0] for w in want}}
    assert min(m for _, m in host.values()) >= 1e-6                   # (no chosen path sits on an aim-point or brake threshold)
    dec = sampled(engine, traj, c["logits"], None, us, c["topk"], c["temperature"])
    assert dec.shape == (len(us), 8)
    idx_ok = np.array_equal(dec[:, 3], [w[0] for w in want])
    pos_ok = np.array_equal(dec[:, 4], [w[1] for w in want])
    p_err = np.abs(dec[:, 5] - np.array([w[2] for w in want])).max()
    ctl = np.stack([host[w[0]][0] for w in want])
    c_err = np.abs(dec[:, [0, 1, 6, 7]] - ctl[:, [0, 1, 3, 4]]).max()
    print(f"{name}: {len(us)} CBVs, {len(host)} candidates chosen; index {idx_ok} position {pos_ok} |p - host| {p_err:.3e} controls {c_err:.3e}")
    assert idx_ok, (dec[:, 3], [w[0] for w in want])
    assert pos_ok, (dec[:, 4], [w[1] for w in want])
    assert p_err < 1e-6 and c_err < 1e-9 and np.array_equal(dec[:, 2], ctl[:, 2])
    if name in S.GREEDY_FOR_EVERY_U:
        assert (dec[:, 3] == np.argmax(c["logits"])).all() and (dec[:, 4] == 0).all() and (dec[:, 5] == 1.0).all()


def test_the_ref_free_rule_comes_first_for_every_u(engine):
    """Flat logits: the best learned score is 0.1 < 0.25, so the ref-free candidate is executed whatever u and T are -- elements 3 to 5 are
    -1, topk, 0.25 and the row is rift_control_tick's, bit for bit."""
    inp = H.inference_inputs(R=4)
    traj, rf = raw_outputs(inp["candidates"], inp["ref_free"])
    logits = np.zeros((4, 12), dtype=np.float32)
    us = np.array([0.0, 0.03, 0.25, 0.55, 0.77, 1.0 - 2.0 ** -53])
    engine.control_state(8).zero_()
    plain = engine.control_tick(dev(traj[None]), dev(logits[None]), dev(rf[None]), [(0, k) + POSE for k in range(len(us))], 10, INTERVAL).cpu().numpy()
    assert (plain[:, 3] == -1).all()
    for T in (0.05, 1.0, 100.0):
        dec = sampled(engine, traj, logits, rf, us, 10, T)
        assert (dec[:, 3] == -1).all() and (dec[:, 4] == 10).all() and (dec[:, 5] == 0.25).all()
        assert np.array_equal(dec, plain)
    # without a ref-free trajectory the same logits are drawn from: ten equal weights
    dec = sampled(engine, traj, logits, None, us, 10, 1.0)
    assert dec[:, 3].tolist() == [0, 0, 2, 5, 7, 9] and np.abs(dec[:, 5] - 0.1).max() < 1e-6 and dec[:, 4].tolist() == dec[:, 3].tolist()


def test_many_cbvs_on_one_row_draw_the_hosts_counts(engine):
    """256 CBVs on one batch row, slots 0..255, u_k = (k + 0.5) / 256: sixteen chunked launches, u indexed across the chunks."""
    m = S.many_case()
    assert min(S.edge_distance(m["logits"], m["topk"], m["temperature"], u) for u in m["u"]) >= S.EDGE_MARGIN
    traj, _ = raw_outputs(H.inference_inputs(seed=611, R=m["Rb"])["candidates"])
    want = np.array([inf.sample_candidate(m["logits"], m["topk"], m["temperature"], u)[0] for u in m["u"]])
    dec = sampled(engine, traj, m["logits"], None, m["u"], m["topk"], m["temperature"])
    got = dec[:, 3].astype(np.int64)
    assert np.array_equal(np.bincount(got, minlength=m["G"]), np.bincount(want, minlength=m["G"]))
    assert np.array_equal(got, want) and len(set(want.tolist())) == m["topk"]


def test_distinct_u_across_the_chunk_seam(engine):
    s = S.seam_case()
    assert len(s["u"]) == 17 and min(S.edge_distance(s["logits"], s["topk"], s["temperature"], u) for u in s["u"]) >= S.EDGE_MARGIN
    traj, _ = raw_outputs(H.inference_inputs(seed=612, R=s["Rb"])["candidates"])
    want = [inf.sample_candidate(s["logits"], s["topk"], s["temperature"], u) for u in s["u"]]
    assert want[15][0] != want[16][0] and want[16][0] != want[0][0]                      # (the CBV behind the seam is told from its neighbours)
    dec = sampled(engine, traj, s["logits"], None, s["u"], s["topk"], s["temperature"])
    assert dec[:, 3].tolist() == [w[0] for w in want] and dec[:, 4].tolist() == [w[1] for w in want]
    assert np.abs(dec[:, 5] - [w[2] for w in want]).max() < 1e-6


def test_refusals_are_decided_before_any_launch(engine):
    from rift_amd import _abi_select, _ffi
    inp = H.inference_inputs()
    traj, rf = raw_outputs(inp["candidates"], inp["ref_free"])
    t, p, r = dev(traj[None]), dev(inp["probability"][None]), dev(rf[None])
    state = torch.full((8, 44), 2.5, dtype=torch.float64, device="cuda")
    dec = torch.full((2, 8), -7.0, dtype=torch.float64, device="cuda")
    lib, st = engine.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    NULL = object()

    def call(mode=1, reserved=0, temperature=1.0, u=(0.25, 0.75), params=True, K=2, topk=10, cbvs=((0, 2), (0, 5))):
        arr = (_ffi.RiftControlCBV * max(len(cbvs), 1))()
        for a, (b, s) in zip(arr, cbvs):
            a.batch_index, a.slot, a.x, a.y, a.heading, a.speed = b, s, 1.0, 2.0, 0.3, 4.0
        sel = _abi_select.RiftSelectParams(mode, reserved, temperature)
        un = None if u is NULL else (C.c_double * max(len(u), 1))(*u)
        rc = lib.riftcs_control_tick(engine.ctx, t.data_ptr(), p.data_ptr(), r.data_ptr(), 4, 80, arr, K, topk, INTERVAL, state.data_ptr(), 8,
                                     C.byref(sel) if params else None, None if un is None else C.cast(un, C.c_void_p), dec.data_ptr(), st)
        return rc, (lib.rift_last_error(engine.ctx) or b"").decode()

    nan, inf_ = float("nan"), float("inf")
    refused = {"params == NULL": dict(params=False), "mode outside": dict(mode=2), "mode outside ": dict(mode=-1), "reserved != 0": dict(reserved=1),
               "temperature not finite or <= 0": dict(temperature=0.0), "temperature not finite or <= 0 ": dict(temperature=-1.0),
               "temperature not finite or <= 0  ": dict(temperature=nan), "temperature not finite or <= 0   ": dict(temperature=inf_),
               "temperature not finite or <= 0    ": dict(mode=0, temperature=nan),
               "u == NULL in SAMPLE": dict(u=NULL), "u[k] NaN or outside [0, 1)": dict(u=(0.25, nan)), "u[k] NaN or outside [0, 1) ": dict(u=(1.0, 0.5)),
               "u[k] NaN or outside [0, 1)  ": dict(u=(0.5, -1e-300)), "u[k] NaN or outside [0, 1)   ": dict(u=(0.5, inf_)),
               # rift_control_tick's own refusals apply on top, under this entry's name
               "topk outside [1, Rb * 12]": dict(topk=0), "two CBVs with the same slot": dict(cbvs=((0, 3), (0, 3))), "K < 0": dict(K=-1),
               "slot outside [0, n_slots)": dict(mode=0, cbvs=((0, 2), (0, 8)))}
    for what, kw in refused.items():
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("riftcs_control_tick: " + what.strip()), (what, rc, msg)
    for kw in (dict(K=0, cbvs=()), dict(K=0, cbvs=(), u=NULL), dict(K=0, cbvs=(), mode=0, u=NULL)):
        assert call(**kw)[0] == 0                                                   # K == 0: RIFT_OK without a launch
    torch.cuda.synchronize()
    assert (state == 2.5).all().item() and (dec == -7.0).all().item()              # nothing was launched
    for kw in (dict(), dict(mode=0, u=NULL)):                                       # (the harness itself is sound: accepted calls write)
        dec.fill_(-7.0)
        rc, msg = call(**kw)
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert (dec != -7.0).all().item() and (state[[0, 1, 3, 4, 6, 7]] == 2.5).all().item()


class _Recorded:
    def __init__(self):
        from rift_amd.planning.pluto.pluto import CenterState
        self.CenterState = CenterState

    def center_state(self, env_id, cbv_id):
        return self.CenterState(10.0 + cbv_id, -5.0 + 0.5 * env_id, 0.3 - 0.1 * cbv_id, 4.0 + 0.3 * cbv_id, 2.0, 4.6, 4.1 + 0.3 * cbv_id)


POLICY_TOPK = 3         # (the best of three softmax scores is at least 1/3 > 0.25: every decision of the test is a learned, drawn one)
POLICY_SEED = {'pluto': 0, 'ppo_pluto': 0}      # (chosen with runs of the host path alone: the closest of its 11 draws is 3.0e-2 W from an edge)
TICK_IDS = [[5, 6, 7], [5, 7], [5, 7, 8], [5, 7, 8]]


def policy_pair(name, root, seed):
    """The host-path and the device-path policy of the test under the same weights and config['action_selection']; the host one records, per
    drawn decision, the distance of its u to the nearest CDF edge (in units of W) and the kept position drawn."""
    from rift_amd.planning import CBV_POLICY_LIST
    torch.cuda.set_device(0)
    sd = H.weights()

    class Probe(CBV_POLICY_LIST[name]):
        def _decide(self, out, index, env_id, cbv_id, state, u=None):
            d = super()._decide(out, index, env_id, cbv_id, state, u)
            if u is not None:
                self.distances.append(S.edge_distance(d.probability, self._topk, self._selection['temperature'], u))
                self.positions.append(d.best)
            return d

    pols = {}
    for on in (False, True):
        cfg = {'num_scenario': 2, 'device': 'cuda:0', 'state_source': _Recorded(), 'ROOT_DIR': str(root), 'model_path': 'ckpt', 'device_control': on,
               'topk': POLICY_TOPK, 'action_selection': {'mode': 'sample', 'temperature': 1.0, 'seed': seed}}
        pols[on] = Probe(cfg, None)
        pols[on].pluto_model.load_state_dict(sd)
        pols[on].mode = 'train'         # (set directly: plain PLUTO has no train mode of its own, and no tick reads RLFTPluto's training model)
        pols[on].distances, pols[on].positions = [], []
    return pols


def policy_observations(t, ids):
    feats = {c: syn.make_scene(4100 + 16 * t + c, num_agents=12, num_polygons=8, r_min=2, r_max=4)["feature"] for c in ids}
    return [{}, {c: {'raw_pluto_feature': PlutoFeature(data=f)} for c, f in feats.items()}]


@pytest.mark.parametrize("name", ["pluto", "ppo_pluto"])
def test_policy_sampling_on_the_device_path_equals_the_host_path(name, tmp_path):
    """config['action_selection'] with config['device_control'] against the host path: same weights, same synthetic scenes, same seed, four
    ticks with a CBV leaving and one arriving (the fixtures of test_policy_device_control_equals_the_host_path).  Controls to 1e-9, the
    chosen mode exactly, the old log-probability to 1e-6 -- given that no host draw lies within 1e-4 W of a CDF edge, which is asserted."""
    pols = policy_pair(name, tmp_path, POLICY_SEED[name])
    infos = [{'env_id': 0}, {'env_id': 1}]
    for t, ids in enumerate(TICK_IDS):
        obs = policy_observations(t, ids)
        a, b = pols[False].get_action(obs, infos), pols[True].get_action(obs, infos)
        assert set(a) == set(b)
        for c in ids:
            ha, da = a['CBVs_actions'][1][c], b['CBVs_actions'][1][c]
            assert bool(ha[2]) == da[2] and abs(ha[0] - da[0]) < 1e-9 and abs(ha[1] - da[1]) < 1e-9, (t, c, ha, da)
            if name == 'ppo_pluto':
                assert tuple(a['CBVs_actions_mode'][1][c]) == tuple(b['CBVs_actions_mode'][1][c])
                assert abs(a['CBVs_actions_old_log_prob'][1][c] - b['CBVs_actions_old_log_prob'][1][c]) < 1e-6
    host = pols[False]
    print(f"{name}: {len(host.distances)} draws, closest to an edge {min(host.distances):.3e} W, positions {host.positions}")
    assert len(host.distances) == sum(len(i) for i in TICK_IDS) and min(host.distances) >= S.EDGE_MARGIN
    assert any(p > 0 for p in host.positions)                                     # sampling shows: not every draw is the greedy candidate
    assert not pols[True].distances and not pols[True].controllers                # the device path never ran _decide
    assert pols[False]._select_rng.bit_generator.state == pols[True]._select_rng.bit_generator.state
    # a deterministic call is greedy on both paths and draws nothing
    state = pols[True]._select_rng.bit_generator.state
    obs = policy_observations(4, [5, 7])
    a, b = pols[False].get_action(obs, infos, deterministic=True), pols[True].get_action(obs, infos, deterministic=True)
    for c in (5, 7):
        assert abs(a['CBVs_actions'][1][c][1] - b['CBVs_actions'][1][c][1]) < 1e-9
    assert pols[True]._select_rng.bit_generator.state == state and len(host.distances) == sum(len(i) for i in TICK_IDS)
    for p in pols.values():
        p.pluto_model.release_engine()
