"""rift_control_tick -- candidate choice and waypoint PID of a tick's CBVs as one device call -- against the reference's own numbers
(tests/golden/inference.npz) and against the host path it replaces (trim_candidates + global_to_local + PIDController, itself pinned by that
fixture), and the policy-level opt-in (config['device_control']) against the default host path."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from rift_amd import synthetic as syn
from rift_amd.planning.pluto import inference as inf
from rift_amd.planning.pluto.controller.pid_controller import PIDController
from rift_amd.planning.pluto.feature_builder.pluto_feature import PlutoFeature
from tests import helpers as H

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "inference.npz")
TOPK, INTERVAL = 10, 10


@pytest.fixture(scope="module")
def engine():
    from rift_amd import _ffi
    torch.cuda.set_device(0)
    eng = _ffi.Engine("cuda:0")
    yield eng
    eng.close()


def raw_outputs(cand, ref_free, scale=1.0):
    """fp32 `trajectory` (R, 12, T, 6) and `ref_free_trajectory` (T, 4) of rift_forward from (x, y, heading) paths, x and y scaled."""
    traj = np.zeros(cand.shape[:-1] + (6,), dtype=np.float32)
    traj[..., 0], traj[..., 1] = cand[..., 0] * scale, cand[..., 1] * scale
    traj[..., 2], traj[..., 3] = np.cos(cand[..., 2]), np.sin(cand[..., 2])
    rf = np.stack([ref_free[:, 0] * scale, ref_free[:, 1] * scale, np.cos(ref_free[:, 2]), np.sin(ref_free[:, 2])], -1).astype(np.float32)
    return traj, rf


def host_decision(ctrl, traj, prob, rf, origin, angle, speed):
    """The host path on the same fp32 tensors (PLUTO._decide): -> the decision row and the margins of its two discontinuous choices."""
    def xyh(a):
        a = a.astype(np.float64)
        return np.concatenate([a[..., :2], np.arctan2(a[..., 3], a[..., 2])[..., None]], -1)
    origin = np.asarray(origin, dtype=np.float64)
    kept, score, flat, _, _ = inf.trim_candidates(xyh(traj), prob, origin, float(angle), None if rf is None else xyh(rf), TOPK)
    best = int(score.argmax())
    local = inf.global_to_local(kept[best, 1:], origin, float(angle))
    throttle, steer, brake = ctrl.control_pid(local[:, :2], float(speed))
    pts = local[INTERVAL - 1::INTERVAL, :2]
    aim = min(max(0.5 * speed + 2.5, 5.0), 8.0)
    miss = np.sort(np.abs(np.sqrt((pts[:-1] ** 2).sum(1)) - aim))
    row = np.array([throttle, steer, float(brake), flat[best], best, score[best], ctrl.desired_speed, ctrl.delta_angle], dtype=np.float64)
    return row, {"aim": miss[1] - miss[0], "score": abs(float(score[:TOPK].max()) - 0.25)}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def test_six_calls_match_the_reference_generated_actions(engine):
    """The reference's pid_controller.py generated `actions` of inference.npz on local * (1 + 0.05 k) at speeds 3.0 + 0.5 k, one controller
    over the six calls.  Here the same paths enter as fp32 model outputs (every candidate and the ref-free path scaled), pose from the same
    helper; the ref-free candidate wins (best learned score 0.2368 < 0.25).  Bound 1e-8: the host path on these fp32 inputs is 1e-10 from the
    fixture, the device adds libm differences of a few ulp."""
    gold = np.load(GOLD)
    inp = H.inference_inputs()
    slot = 3
    engine.control_reset([slot])
    for k in range(6):
        traj, rf = raw_outputs(inp["candidates"], inp["ref_free"], 1.0 + 0.05 * k)
        dec = engine.control_tick(dev(traj[None]), dev(inp["probability"][None]), dev(rf[None]),
                                  [(0, slot, inp["origin"][0], inp["origin"][1], inp["angle"], 3.0 + 0.5 * k)], TOPK, INTERVAL).cpu().numpy()
        err = np.abs(dec[0, :3] - gold["actions"][k]).max()
        print(f"call {k}: decision {dec[0]} |actions - fixture| {err:.3e}")
        assert dec.shape == (1, 8) and err < 1e-8, (k, dec[0], gold["actions"][k])
        assert dec[0, 3] == -1 and dec[0, 4] == TOPK and dec[0, 5] == 0.25


def branch_case():
    """Three batch rows, four CBVs, five ticks: inputs of the learned-choice / controller-branch test and, per tick, the host decisions."""
    inp = H.inference_inputs()
    g = np.random.default_rng(5)
    prob = np.stack([inp["probability"], inp["probability"], g.normal(size=(4, 12)).astype(np.float32)])
    prob[1, 1, 3] = 3.0                                      # rows 1 and 2: a learned candidate clearly above the ref-free score
    prob[2, 2, 7] = 3.5
    prob[2, 3] = -1e6                                        # a padded reference line, as the model emits it
    cand = np.stack([inp["candidates"], inp["candidates"] * np.array([0.03, 0.03, 1.0]), H.inference_inputs(seed=911)["candidates"]])
    poses = {"cruise": (0, 1, (12.5, -3.25, 0.6)), "crawl": (1, 4, (-40.0, 7.5, -2.1)), "fast": (0, 7, (3.0, 88.0, 1.3)), "stand": (2, 10, (250.0, -130.0, 2.9))}
    ticks = []
    ctrls = {name: PIDController(sample_interval=INTERVAL) for name in poses}
    for t in range(5):
        scale = 1.0 + 0.04 * t
        tr, rfs = zip(*[raw_outputs(cand[b], inp["ref_free"] * np.array([1.0, 1.0 + 0.5 * b, 1.0]), scale) for b in range(3)])
        traj, rf = np.stack(tr), (None if t == 2 else np.stack(rfs))            # one call without a ref-free candidate
        rows, margins, cbvs = [], [], []
        for name, (b, slot, (x, y, h)) in poses.items():
            # target speed of the path this CBV will choose (a scratch controller: the real one steps once per tick)
            target = host_decision(PIDController(sample_interval=INTERVAL), traj[b], prob[b], None if rf is None else rf[b], (x, y), h, 1.0)[0][6]
            speed = {"cruise": target - 0.05 - 0.01 * t, "crawl": 0.3, "fast": 1.5 * target, "stand": 0.005}[name]
            row, m = host_decision(ctrls[name], traj[b], prob[b], None if rf is None else rf[b], (x, y), h, speed)
            rows.append(row); margins.append(m); cbvs.append((b, slot, x, y, h, speed))
        ticks.append({"traj": traj, "rf": rf, "cbvs": cbvs, "host": np.stack(rows), "margins": margins})
    return prob, ticks


def test_learned_choice_and_controller_branches_match_the_host_path(engine):
    prob, ticks = branch_case()
    names = ["cruise", "crawl", "fast", "stand"]
    host = np.stack([t["host"] for t in ticks])             # (tick, CBV, 8)
    # ---- the HOST result has the properties this test is about
    i = {n: k for k, n in enumerate(names)}
    assert ((host[:, i["cruise"], 0] > 0) & (host[:, i["cruise"], 0] < 1)).sum() >= 3 and not host[:, i["cruise"], 2].any()
    assert host[:, i["crawl"], 2].all() and (host[:, i["crawl"], 6] < 0.4).all()                      # braking: target speed below 0.4
    assert host[:, i["fast"], 2].all() and (host[:, i["fast"], 6] >= 0.4).all()                       # braking: by the speed ratio
    assert not host[:, i["stand"], 2].any() and (host[:, i["stand"], 7] == 0).all() and (host[:, i["stand"], 0] == 1).all()
    assert ticks[0]["cbvs"][i["cruise"]][0] == ticks[0]["cbvs"][i["fast"]][0]                         # two CBVs share a batch row
    assert (host[2, [i["cruise"], i["fast"]], 3] == 41).all() and (host[[0, 1, 3, 4]][:, [i["cruise"], i["fast"]], 3] == -1).all()
    assert (host[:, i["crawl"], 3] == 15).all() and (host[:, i["stand"], 3] == 31).all() and (host[:, [i["crawl"], i["stand"]], 4] == 0).all()
    assert np.abs(host[:, i["cruise"], 1]).max() > 1e-3                                                # the turn PID has something to do
    for t in ticks:
        for m in t["margins"]:
            assert m["aim"] >= 1e-3
            assert t["rf"] is None or m["score"] >= 1e-3
    # ---- the device, on non-adjacent slots of a state whose other rows hold a pattern
    state = engine.control_state(16)
    slots = [c[1] for c in ticks[0]["cbvs"]]
    assert slots == [1, 4, 7, 10]
    pattern = torch.arange(16 * 44, dtype=torch.float64, device="cuda").view(16, 44) * 0.37 + 1.0
    state[:16].copy_(pattern)
    engine.control_reset(slots)
    p = dev(prob)
    for k, t in enumerate(ticks):
        dec = engine.control_tick(dev(t["traj"]), p, None if t["rf"] is None else dev(t["rf"]), t["cbvs"], TOPK, INTERVAL).cpu().numpy()
        want = t["host"]
        err = np.abs(dec - want)
        print(f"tick {k}: max |device - host| throttle/steer/speed/angle {err[:, [0, 1, 6, 7]].max():.3e} score {err[:, 5].max():.3e}")
        assert np.array_equal(dec[:, [2, 3, 4]], want[:, [2, 3, 4]]), (k, dec, want)
        assert err[:, [0, 1, 6, 7]].max() < 1e-9, (k, dec, want)
        assert err[:, 5].max() < 1e-6, (k, dec[:, 5], want[:, 5])
    after = engine.control_state(16)[:16].cpu()
    untouched = [s for s in range(16) if s not in slots]
    assert torch.equal(after[untouched], pattern.cpu()[untouched])
    assert not torch.equal(after[slots], torch.zeros(4, 44, dtype=torch.float64))
    engine.control_reset(range(16))


def test_a_zeroed_slot_is_a_fresh_controller(engine):
    inp = H.inference_inputs()
    traj, rf = raw_outputs(inp["candidates"], inp["ref_free"])
    t, p, r = dev(traj[None]), dev(inp["probability"][None]), dev(rf[None])
    slot = 6
    engine.control_reset([slot])
    first = [(0, slot, 1.0, 2.0, 0.4, 4.0)]
    for _ in range(3):
        engine.control_tick(t, p, r, first, TOPK, INTERVAL)
    other = (0, slot, -7.0, 11.0, -1.2, 4.6)
    used = engine.control_tick(t, p, r, [other], TOPK, INTERVAL).cpu().numpy()[0]
    engine.control_reset([slot])
    assert not engine.control_state()[slot].any().item()
    fresh = engine.control_tick(t, p, r, [other], TOPK, INTERVAL).cpu().numpy()[0]
    want, _ = host_decision(PIDController(sample_interval=INTERVAL), traj, inp["probability"], rf, other[2:4], other[4], other[5])
    assert np.array_equal(fresh[[2, 3, 4]], want[[2, 3, 4]]) and np.abs(fresh - want)[[0, 1, 6, 7]].max() < 1e-9
    assert abs(used[1] - fresh[1]) > 1e-6                    # (the state the slot held before did matter)


def test_argument_checks_refuse_before_any_launch(engine):
    from rift_amd import _ffi
    inp = H.inference_inputs()
    traj, rf = raw_outputs(inp["candidates"], inp["ref_free"])
    t, p, r = dev(traj[None]), dev(inp["probability"][None]), dev(rf[None])
    state = torch.full((8, 44), 2.5, dtype=torch.float64, device="cuda")
    dec = torch.full((2, 8), -7.0, dtype=torch.float64, device="cuda")
    lib, st = engine.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(Rb=4, Tfull=80, cbvs=((0, 0),), K=None, topk=TOPK, interval=INTERVAL, n_slots=8):
        arr = (_ffi.RiftControlCBV * max(len(cbvs), 1))()
        for a, (b, s) in zip(arr, cbvs):
            a.batch_index, a.slot, a.x, a.y, a.heading, a.speed = b, s, 1.0, 2.0, 0.3, 4.0
        rc = lib.rift_control_tick(engine.ctx, t.data_ptr(), p.data_ptr(), r.data_ptr(), Rb, Tfull, arr, len(cbvs) if K is None else K, topk,
                                   interval, state.data_ptr(), n_slots, dec.data_ptr(), st)
        return rc, (lib.rift_last_error(engine.ctx) or b"").decode()

    refused = {"K < 0": dict(K=-1), "topk < 1": dict(topk=0), "topk > Rb * 12": dict(topk=49), "sample_interval < 1": dict(interval=0),
               "Tfull < 2 * sample_interval": dict(Tfull=19), "slot below 0": dict(cbvs=((0, -1),)), "slot at n_slots": dict(cbvs=((0, 8),)),
               "the same slot twice": dict(cbvs=((0, 3), (0, 3))), "batch_index < 0": dict(cbvs=((-1, 0),)),
               "Rb * 12 above the register budget": dict(Rb=86)}
    for what, kw in refused.items():
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("rift_control_tick:"), (what, rc, msg)
    rc, _ = call(cbvs=(), K=0)
    assert rc == 0
    torch.cuda.synchronize()
    assert (state == 2.5).all().item() and (dec == -7.0).all().item()          # nothing was launched
    rc, _ = call(cbvs=((0, 2), (0, 5)))                                         # (the harness itself is sound: the same call, accepted, writes)
    assert rc == 0
    torch.cuda.synchronize()
    assert (dec != -7.0).all().item() and (state[[0, 1, 3, 4, 6, 7]] == 2.5).all().item()


class _Recorded:
    def __init__(self):
        from rift_amd.planning.pluto.pluto import CenterState
        self.CenterState = CenterState

    def center_state(self, env_id, cbv_id):
        return self.CenterState(10.0 + cbv_id, -5.0 + 0.5 * env_id, 0.3 - 0.1 * cbv_id, 4.0 + 0.3 * cbv_id, 2.0, 4.6, 4.1 + 0.3 * cbv_id)


@pytest.mark.parametrize("name", ["pluto", "ppo_pluto"])
def test_policy_device_control_equals_the_host_path(name, tmp_path):
    """config['device_control'] against the default: same weights, same synthetic scenes, three ticks; a CBV leaves after the first tick
    and a new one arrives at the third (it gets the row the departed one left, zeroed)."""
    from rift_amd.planning import CBV_POLICY_LIST
    torch.cuda.set_device(0)
    sd = H.weights()

    class Probe(CBV_POLICY_LIST[name]):
        def _finish_env(self, env_id, data, out):
            self.seen = out
            super()._finish_env(env_id, data, out)

    pols = {}
    for on in (False, True):
        cfg = {'num_scenario': 2, 'device': 'cuda:0', 'state_source': _Recorded(), 'ROOT_DIR': str(tmp_path), 'model_path': 'ckpt', 'device_control': on}
        pols[on] = Probe(cfg, None)
        pols[on].pluto_model.load_state_dict(sd)
        pols[on].set_mode('eval')
    assert pols[True].device_control and not pols[False].device_control
    pols[True]._render = True                                                          # rendering keeps the host path
    assert not pols[True].device_control
    pols[True]._render = False
    infos = [{'env_id': 0}, {'env_id': 1}]
    slot_of_6 = None
    for t, ids in enumerate([[5, 6, 7], [5, 7], [5, 7, 8]]):
        feats = {c: syn.make_scene(4100 + 16 * t + c, num_agents=12, num_polygons=8, r_min=2, r_max=4)["feature"] for c in ids}
        obs = [{}, {c: {'raw_pluto_feature': PlutoFeature(data=f)} for c, f in feats.items()}]
        a, b = pols[False].get_action(obs, infos), pols[True].get_action(obs, infos)
        assert set(a) == set(b)
        for c in ids:
            ha, da = a['CBVs_actions'][1][c], b['CBVs_actions'][1][c]
            assert bool(ha[2]) == da[2] and abs(ha[0] - da[0]) < 1e-9 and abs(ha[1] - da[1]) < 1e-9, (t, c, ha, da)
            if name == 'ppo_pluto':
                assert 'CBVs_actions_mode' in b and 'CBVs_actions_old_log_prob' in b
                assert tuple(a['CBVs_actions_mode'][1][c]) == tuple(b['CBVs_actions_mode'][1][c])
                assert abs(a['CBVs_actions_old_log_prob'][1][c] - b['CBVs_actions_old_log_prob'][1][c]) < 1e-6
        host_cache = pols[True].seen.get("_host", {})
        assert "candidate_trajectories" not in host_cache and "output_ref_free_trajectory" not in host_cache
        assert "candidate_trajectories" in pols[False].seen["_host"]
        slots = pols[True]._control_slots
        assert sorted(k[1] for k in slots.keys()) == ids and not pols[True].controllers
        if t == 0:
            slot_of_6 = slots.slot((1, 6))
        if t == 1:
            assert (1, 6) not in slots and slots.pending() == [slot_of_6]
        if t == 2:
            assert slots.pending() == [] and slots.slot((1, 8)) == slot_of_6 and slots.rows == 3
    for p in pols.values():
        p.pluto_model.release_engine()


class _RecordedWithFlags(_Recorded):
    def nearby_actor_states(self, env_id, cbv_id):
        return H.other_vehicle_inputs(seed=100 + cbv_id, N=4) if cbv_id % 2 else None

    def off_road_raster(self, env_id, cbv_id):
        mask = np.ones((400, 400), dtype=np.uint8)
        mask[150:250, :300] = 0
        return mask, (10.0 + cbv_id, -5.0, 0.3)


def test_group_relative_train_tick_with_device_control(tmp_path):
    """RIFTPluto in train mode: the control tick is issued ahead of rift_group_advantage_tick on the same stream.  Against the host path on
    the same weights and scenes: controls to 1e-9, the old-policy logits and the group advantages equal bit for bit (the same kernels on the
    same inputs -- the control tick writes nothing they read), and neither big array in the host cache."""
    from rift_amd.planning import CBV_POLICY_LIST
    torch.cuda.set_device(0)
    sd = H.weights()

    class Probe(CBV_POLICY_LIST['rift_pluto']):
        def _finish_env(self, env_id, data, out):
            self.seen = out
            super()._finish_env(env_id, data, out)

    pols = {}
    for on in (False, True):
        cfg = {'num_scenario': 1, 'device': 'cuda:0', 'state_source': _RecordedWithFlags(), 'ROOT_DIR': str(tmp_path), 'model_path': 'ckpt',
               'device_control': on}
        pols[on] = Probe(cfg, None)
        pols[on].pluto_model.load_state_dict(sd)
        pols[on].set_mode('train')
    for t, ids in enumerate([[1, 2, 3], [2, 3]]):
        feats = {c: syn.make_scene(5200 + 16 * t + c, num_agents=12, num_polygons=8, r_min=1, r_max=4)["feature"] for c in ids}
        obs = [{c: {'raw_pluto_feature': PlutoFeature(data=f)} for c, f in feats.items()}]
        a, b = pols[False].get_action(obs, [{'env_id': 0}]), pols[True].get_action(obs, [{'env_id': 0}])
        assert set(a) == set(b) == {'CBVs_actions', 'CBVs_actions_old_group_logits', 'CBVs_group_advantage'}
        for c in ids:
            ha, da = a['CBVs_actions'][0][c], b['CBVs_actions'][0][c]
            assert bool(ha[2]) == da[2] and abs(ha[0] - da[0]) < 1e-9 and abs(ha[1] - da[1]) < 1e-9, (t, c, ha, da)
            assert np.array_equal(a['CBVs_actions_old_group_logits'][0][c]['logits'], b['CBVs_actions_old_group_logits'][0][c]['logits'])
            adv = b['CBVs_group_advantage'][0][c]['advantage']
            assert np.isfinite(adv).all() and np.array_equal(a['CBVs_group_advantage'][0][c]['advantage'], adv)
        host_cache = pols[True].seen["_host"]
        assert "probability" in host_cache and "candidate_trajectories" not in host_cache and "output_ref_free_trajectory" not in host_cache
    for p in pols.values():
        p.pluto_model.release_engine()
