"""The evaluator's run-time parameters on the host: the C-ABI declarations and the RiftEvalParams layout, the references for non-default
reward weights against the reference's own numbers (tests/golden/reward_params.npz), the visibility of every parameter on the inputs of
tests/test_gpu_eval_params.py, and the policy's `traj_eval` configuration.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import advantage as oadv
from tests import eval_param_cases as E
from tests import helpers as H
from tests import small_kernel_cases as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = dict(np.load(os.path.join(H.GOLDEN, "reward_params.npz")))
NEW = ("rift_eval_params_default", "rift_rollout_return_ex", "rift_group_advantage_tick_ex")


def test_header_declares_the_entries_and_the_struct_matches_a_c_compiler(tmp_path):
    """include/rift_hip.h declares the three new functions, _ffi.EXPORTS holds them, and _ffi.RiftEvalParams has gcc's sizeof (104) and
    field offsets (the approach of tests/test_host_api.py)."""
    from rift_amd import _ffi
    hdr = open(os.path.join(REPO, "include", "rift_hip.h")).read()
    declared = set(re.findall(r"^int\s+(rift_[a-z_0-9]+)\s*\(", hdr, re.M))
    for name in NEW:
        assert name in declared and name in _ffi.EXPORTS, name
    assert ctypes.sizeof(_ffi.RiftEvalParams) == 104
    assert [f for f, _ in _ffi.RiftEvalParams._fields_][3:12] == list(E.KEYS)          # the nine weights in the reference's order
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rift_hip.h"', 'int main(void) {',
             '  printf("%zu %d %d", sizeof(RiftEvalParams), RIFT_REWARD_DENSE, RIFT_REWARD_SPARSE);']
    lines += [f'  printf(" %zu", offsetof(RiftEvalParams, {f}));' for f, _ in _ffi.RiftEvalParams._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.check_call([gcc, "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "layout")])
    size, dense, sparse, *offs = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")], text=True).split()]
    assert size == ctypes.sizeof(_ffi.RiftEvalParams) and (dense, sparse) == (_ffi.REWARD_MODELS["dense"], _ffi.REWARD_MODELS["sparse"])
    assert [getattr(_ffi.RiftEvalParams, f).offset for f, _ in _ffi.RiftEvalParams._fields_] == offs


def test_eval_params_defaults_and_refusals_on_the_host():
    """_ffi.eval_params: the reference's defaults without arguments, a model's weights by name, the sparse model's two weights, and a
    reward model with a parameter the struct does not have is refused."""
    from rift_amd import _ffi
    from rift_amd.gym_carla.reward.reward_model import DenseRewardModel, SparseRewardModel
    p = _ffi.eval_params()
    assert (p.reward_model, p.near_lane_change, p.gamma, p.bbox_inflation_ratio, p.resolution) == (0, 1, 0.98, 1.1, 0.5)
    assert {k: getattr(p, k) for k in E.KEYS} == E.DEFAULTS == DenseRewardModel().get_params()
    m = DenseRewardModel()
    m.params.update(E.SETS["B"])
    p = _ffi.eval_params(m, 0.9, 1.3, 0.25, False)
    assert {k: getattr(p, k) for k in E.KEYS} == E.SETS["B"] and (p.gamma, p.near_lane_change, p.bbox_inflation_ratio, p.resolution) == (0.9, 0, 1.3, 0.25)
    p = _ffi.eval_params(SparseRewardModel())
    assert (p.reward_model, p.alpha_collision, p.alpha_boundary) == (1, 15.0, 15.0) and SparseRewardModel().get_params() == E.SPARSE["reference"]
    m.params["alpha_typo"] = 1.0
    with pytest.raises(ValueError, match="alpha_typo"):
        _ffi.eval_params(m)
    with pytest.raises(ValueError, match="alpha_typo"):
        DenseRewardModel(alpha_typo=1.0)


def test_oracle_and_host_models_agree_with_the_reference_under_edited_weights():
    """The reference's get_rollout_return with DenseRewardModel.params edited (three sets, gamma 0.98 and 0.9; reward_params.npz) against
    oracle.advantage with P patched and against rift_amd's host DenseRewardModel: returns 2e-6 relative /(1 + |gold|), z-scores 1e-5 -- the
    bars of tests/test_oracle_advantage.py (the fixture was produced under numpy 2.x promotion, see there).  The sparse model, which has no
    float32 arithmetic, to 1e-12."""
    from rift_amd.gym_carla.reward import reward_model as rm
    i = H.advantage_inputs()
    args = (i["delta_dis"], i["delta_angle"], i["speed"], i["acc"], i["ang_vel"], i["ang_acc"], i["collision"], i["off_road"])
    before = dict(oadv.P)
    worst = [0.0, 0.0]
    for name, weights in E.SETS.items():
        assert np.array_equal(GOLD[f"weights_{name}"], [weights[k] for k in E.KEYS])
        for g in E.GAMMAS:
            gold, gold_z = GOLD[f"ret_{name}_{g}"], GOLD[f"z_{name}_{g}"]
            model = rm.DenseRewardModel(**{k: weights[k] for k in E.moved(weights)})
            for ret in (E.dense_return(weights, i, g, Ts=40), rm.rollout_return(model, *args, gamma=g)):
                e, ez = np.max(np.abs(ret - gold) / (1 + np.abs(gold))), np.max(np.abs(oadv.group_zscore(ret) - gold_z))
                worst = [max(worst[0], e), max(worst[1], ez)]
                assert e < 2e-6 and ez < 1e-5, (name, g, e, ez)
    print(f"edited weights: returns {worst[0]:.2e} relative, z-scores {worst[1]:.2e}")
    assert oadv.P == before == E.DEFAULTS
    c = dict(i, off_road=i["off_road"][:, :40])
    for name, w in E.SPARSE.items():
        assert np.array_equal(GOLD[f"weights_sparse_{name}"], [w["alpha_collision"], w["alpha_boundary"]])
        for g in E.GAMMAS:
            gold = GOLD[f"ret_sparse_{name}_{g}"]
            assert np.max(np.abs(E.sparse_return(w, c, g) - gold)) < 1e-12
            assert np.max(np.abs(rm.rollout_return(rm.SparseRewardModel(**w), *args, gamma=g) - gold)) < 1e-12
    assert np.abs(GOLD["ret_sparse_reference_0.98"]).max() > 10          # the fixture's inputs do collide and leave the road


def test_every_parameter_shows_on_the_gpu_tests_inputs():
    """On rollout_return_case(9, Ts, .) for Ts = 40, 64, 65, 130 -- inputs of the device test -- at gamma 0.93: each weight a set moves,
    put back to its default ALONE, moves the reference return by more than 100 bars of that test (bar = 1e-5 max(1, max |ref|)); so does
    gamma (0.93 against 0.98) and the sparse switch, and the sparse model keeping |speed| in its collision term.  No thresholded quantity
    sits within RR_MARGIN of its threshold."""
    shown = set()
    for s, Ts in ((1, 40), (4, 64), (5, 65), (6, 130)):
        c = K.rollout_return_case(9, Ts, s)
        assert all(v > K.RR_MARGIN for v in K.rollout_return_margins(c).values())
        for name, weights in E.SETS.items():
            ref = E.dense_return(weights, c, K.RR_GAMMA)
            bar = 1e-5 * max(1.0, float(np.max(np.abs(ref))))
            for k in E.moved(weights):
                d = float(np.max(np.abs(E.dense_return(dict(weights, **{k: E.DEFAULTS[k]}), c, K.RR_GAMMA) - ref)))
                assert d > 100 * bar, (Ts, name, k, d, bar)
                shown.add(k)
            assert float(np.max(np.abs(E.dense_return(weights, c, 0.98) - ref))) > 100 * bar, (Ts, name, "gamma")
        cc = dict(c, collision=c["collision"][:, :Ts], off_road=c["off_road"][:, :Ts])
        for w in E.SPARSE.values():
            ref = E.sparse_return(w, cc, K.RR_GAMMA)
            bar = 1e-5 * max(1.0, float(np.max(np.abs(ref))))
            dense = E.dense_return(dict(E.DEFAULTS, **w), c, K.RR_GAMMA)
            assert float(np.max(np.abs(dense - ref))) > 100 * bar                              # the sparse switch
            assert float(np.max(np.abs(E.sparse_return(w, cc, 0.98) - ref))) > 100 * bar       # gamma
            for k in w:                                                                        # each of its two weights
                assert float(np.max(np.abs(E.sparse_return(dict(w, **{k: w[k] + 3.0}), cc, K.RR_GAMMA) - ref))) > 100 * bar, k
            speedy = ref.copy()                                                                # |speed| kept in the collision term
            for i in range(9):
                hit = np.nonzero(cc["collision"][i])[0]
                if hit.size:
                    speedy[i] -= abs(float(c["speed"][i, hit[0]])) * K.RR_GAMMA ** int(hit[0])
            assert float(np.max(np.abs(speedy - ref))) > 100 * bar
    assert shown == set(E.KEYS)


class _Tick:
    """An engine stub: records how group_advantage_tick is called."""

    def __init__(self):
        self.calls = []

    def group_advantage_tick(self, *a, **kw):
        self.calls.append((a, kw))
        K, Rb = len(a[1]), a[0].shape[1]
        if kw.get("want_returns") or kw.get("want_terms"):
            packed = torch.zeros(K * Rb * 12 * 10, dtype=torch.float64)
            return {"packed": packed, "advantage": packed[:K * Rb * 12].view(K, Rb, 12)}
        return torch.zeros(K, Rb, 12, dtype=torch.float64)


def _tick_calls(section, monkeypatch):
    import types
    import rift_amd.synthetic as syn
    from rift_amd.planning import CBV_POLICY_LIST
    from rift_amd.planning.pluto.feature_builder.pluto_feature import PlutoFeature
    from rift_amd.planning.pluto.pluto import CenterState, NoFlagSource

    class Source:
        def nearby_actor_states(self, env_id, cbv_id):
            return NoFlagSource.ALL_CLEAR

        def off_road_raster(self, env_id, cbv_id):
            return NoFlagSource.ALL_CLEAR

    cfg = {'num_scenario': 1, 'device': 'cpu', 'state_source': Source()}
    if section is not None:
        cfg['traj_eval'] = section
    pol = CBV_POLICY_LIST['rift_pluto'](cfg, None)
    pol.mode = 'train'
    eng = _Tick()
    pol._traj_evaluator = types.SimpleNamespace(engine=eng, pid_state={})
    monkeypatch.setattr(type(pol.pluto_model), "_engine", None, raising=False)
    feat = syn.make_scene(5001, num_agents=12, num_polygons=8, r_min=2, r_max=2)["feature"]
    obs = {7: {'raw_pluto_feature': PlutoFeature(data=feat)}}
    out = {"trajectory": torch.zeros(1, 2, 12, 80, 6)}
    pol._begin_env(0, obs, None, out, {7: CenterState(1.0, 2.0, 0.3, 6.0, 2.0, 4.6)})
    return pol, eng.calls


def test_policy_traj_eval_configuration(monkeypatch):
    """config['traj_eval'] of the group-relative policies: an unknown key raises and names the known ones; without the key the engine sees
    the call made before the key existed (three positional arguments, no `params`); {} and explicit defaults go through `params` with the
    reference's defaults; the settings reach the struct."""
    from rift_amd import _ffi
    from rift_amd.planning import CBV_POLICY_LIST
    with pytest.raises(ValueError, match="unknown key.*gama.*known.*gamma.*reward_model.*reward_params.*bbox_inflation_ratio.*resolution.*near_lane_change.*breakdown"):
        CBV_POLICY_LIST['rift_pluto']({'num_scenario': 1, 'device': 'cpu', 'traj_eval': {'gama': 0.9}}, None)
    with pytest.raises(ValueError, match="reward_model"):
        CBV_POLICY_LIST['grpo_pluto']({'num_scenario': 1, 'device': 'cpu', 'traj_eval': {'reward_model': 'dens'}}, None)
    with pytest.raises(ValueError, match="alpha_colision"):
        CBV_POLICY_LIST['rift_pluto']({'num_scenario': 1, 'device': 'cpu', 'traj_eval': {'reward_params': {'alpha_colision': 1.0}}}, None)
    pol, calls = _tick_calls(None, monkeypatch)
    (a, kw), = calls
    assert len(a) == 3 and kw == {} and pol._eval is None
    raw = lambda p: bytes(memoryview(p))  # noqa: E731
    explicit = {'gamma': 0.98, 'reward_model': 'dense', 'reward_params': dict(E.DEFAULTS), 'bbox_inflation_ratio': 1.1, 'resolution': 0.5,
                'near_lane_change': True, 'breakdown': False}
    for section in ({}, explicit):
        _, calls = _tick_calls(section, monkeypatch)
        (a, kw), = calls
        assert len(a) == 4 and a[3] == 0.98 and kw["want_returns"] is False and kw["want_terms"] is False
        assert raw(kw["params"]) == raw(_ffi.eval_params())
    section = {'gamma': 0.9, 'reward_model': 'sparse', 'reward_params': {'alpha_boundary': 11.0}, 'bbox_inflation_ratio': 1.3, 'resolution': 0.25,
               'near_lane_change': False, 'breakdown': True}
    _, calls = _tick_calls(section, monkeypatch)
    (a, kw), = calls
    p = kw["params"]
    assert (p.reward_model, p.near_lane_change, p.gamma, p.alpha_collision, p.alpha_boundary, p.bbox_inflation_ratio, p.resolution) == \
        (1, 0, 0.9, 15.0, 11.0, 1.3, 0.25) and kw["want_returns"] is True and kw["want_terms"] is True
