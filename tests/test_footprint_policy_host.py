"""config['traj_eval']['collision'] on the group-relative policies, on the CPU: the key is read and validated, an engine stub records what
the policy asks of it -- without the key the tick call is made without `collision`, with it the mode travels with the call, together with
the map -- and the per-CBV evaluator is built with the mode.  The device side is tests/test_gpu_footprint.py."""
import types

import numpy as np
import pytest
import torch

from tests import drivable_cases as D


class _Engine:
    """Records load_drivable_map and group_advantage_tick."""

    def __init__(self):
        self.loads, self.ticks = [], []

    def load_drivable_map(self, polygons, cell=16.0, margin=1.0):
        self.loads.append(len(polygons))
        return {"n_polys": len(polygons)}

    def group_advantage_tick(self, *a, **kw):
        self.ticks.append((a, kw))
        return torch.zeros(len(a[1]), a[0].shape[1], 12, dtype=torch.float64)


class _Source:
    def nearby_actor_states(self, env_id, cbv_id):
        from rift_amd.planning.pluto.pluto import NoFlagSource
        return NoFlagSource.ALL_CLEAR

    def off_road_raster(self, env_id, cbv_id):
        return np.ones((400, 400), dtype=np.uint8), (1.0, 2.0, 0.3)

    def drivable_area(self, env_id):
        return "Town05", D.lane_map(2, 5)

    def off_road_pose(self, env_id, cbv_id):
        return 1.5 + cbv_id, 2.5, 0.25


def _policy(section, monkeypatch, name='rift_pluto'):
    from rift_amd.planning import CBV_POLICY_LIST
    cfg = {'num_scenario': 1, 'device': 'cpu', 'state_source': _Source()}
    if section is not None:
        cfg['traj_eval'] = section
    pol = CBV_POLICY_LIST[name](cfg, None)
    pol.mode = 'train'
    eng = _Engine()
    pol._traj_evaluator = types.SimpleNamespace(engine=eng, pid_state={})
    monkeypatch.setattr(type(pol.pluto_model), "_engine", None, raising=False)
    return pol, eng


def _tick(pol, ids=(7,)):
    import rift_amd.synthetic as syn
    from rift_amd.planning.pluto.feature_builder.pluto_feature import PlutoFeature
    from rift_amd.planning.pluto.pluto import CenterState
    feat = syn.make_scene(5001, num_agents=12, num_polygons=8, r_min=2, r_max=2)["feature"]
    obs = {c: {'raw_pluto_feature': PlutoFeature(data=feat)} for c in ids}
    pol._begin_env(0, obs, None, {"trajectory": torch.zeros(len(ids), 2, 12, 80, 6)}, {c: CenterState(1.0, 2.0, 0.3, 6.0, 2.0, 4.6) for c in ids})


def test_key_is_read_and_validated():
    from rift_amd.planning import CBV_POLICY_LIST
    for name in ('rift_pluto', 'grpo_pluto'):
        cls = CBV_POLICY_LIST[name]
        assert cls.TRAJ_EVAL_KEYS[-1] == 'collision'
        assert cls._read_traj_eval(None) is None
        assert cls._read_traj_eval({})['collision'] is None
        for mode in ('envelope', 'footprint'):
            assert cls._read_traj_eval({'collision': mode})['collision'] == mode
        for bad in ('sat', 'Footprint', 1, ''):
            with pytest.raises(ValueError, match=r"traj_eval.*collision.*known.*'envelope'.*'footprint'"):
                cls._read_traj_eval({'collision': bad})


def test_unknown_key_message_still_lists_the_earlier_keys_in_their_order():
    from rift_amd.planning import CBV_POLICY_LIST
    order = "gamma.*reward_model.*reward_params.*bbox_inflation_ratio.*resolution.*near_lane_change.*breakdown.*off_road.*raster_size.*map_cell.*map_margin.*collision"
    with pytest.raises(ValueError, match="unknown key.*colision.*known.*" + order):
        CBV_POLICY_LIST['rift_pluto']._read_traj_eval({'colision': 'footprint'})


def test_without_the_key_the_tick_call_is_made_without_collision(monkeypatch):
    for section in (None, {}, {'gamma': 0.9}, {'off_road': 'map'}):
        pol, eng = _policy(section, monkeypatch)
        _tick(pol)
        (a, kw), = eng.ticks
        assert "collision" not in kw, section
        assert (len(a), kw) == (3, {}) if section is None else "params" in kw


def test_with_the_key_the_mode_travels_with_the_tick_together_with_the_map(monkeypatch):
    for mode in ('envelope', 'footprint'):
        pol, eng = _policy({'collision': mode}, monkeypatch)
        _tick(pol, (7, 9))
        (a, kw), = eng.ticks
        assert kw["collision"] == mode and kw["params"] is pol._eval['params'] and eng.loads == []
        assert all(v["raster"] is None and v["off_road"] is not None for v in a[1])
        pol, eng = _policy({'collision': mode, 'off_road': 'map', 'raster_size': (200, 300)}, monkeypatch)
        _tick(pol)
        (a, kw), = eng.ticks
        assert kw["collision"] == mode and eng.loads == [5]
        assert a[1][0]["off_road"] is None and a[1][0]["raster"] == (200, 300) and a[1][0]["pose"] == (8.5, 2.5, 0.25)


def test_the_evaluator_of_the_chain_is_built_with_the_mode(monkeypatch):
    """The non-fused path: TrajEvaluator(..., collision=mode); without the key it is built without the argument."""
    from rift_amd.planning.fine_tuner.rlft.traj_eval import traj_evaluator as te
    from rift_amd.planning import CBV_POLICY_LIST
    made = []

    class Stub:
        def __init__(self, engine, **kw):
            made.append(kw)
            self.engine = engine

    monkeypatch.setattr(te, "TrajEvaluator", Stub)
    for section, want in ((None, None), ({'gamma': 0.9}, None), ({'collision': 'envelope'}, 'envelope'), ({'collision': 'footprint'}, 'footprint')):
        cfg = {'num_scenario': 1, 'device': 'cpu', 'state_source': _Source()}
        if section is not None:
            cfg['traj_eval'] = section
        pol = CBV_POLICY_LIST['rift_pluto'](cfg, None)
        monkeypatch.setattr(pol.pluto_model, "engine", lambda: "engine", raising=False)
        monkeypatch.setattr(type(pol.pluto_model), "_engine", None, raising=False)
        pol.traj_evaluator
        assert made[-1].get("collision") == want and ("collision" in made[-1]) == (want is not None), section


def test_evaluator_takes_the_mode_and_uses_a_callers_matrix_as_it_is():
    """TrajEvaluator(collision=...): an unknown mode raises and names the two; 'envelope' makes Engine.collision_matrix's call of before,
    'footprint' passes mode=; a caller-supplied collision_matrix is not replaced."""
    from rift_amd.planning.fine_tuner.rlft.traj_eval.traj_evaluator import TrajEvaluator
    calls = []

    class Eng:
        def new_pid_state(self, n):
            return {}

        def ref_line_info(self, *a, **kw):
            return torch.zeros(12, 40), torch.zeros(12, 40), None

        def rollout(self, *a, **kw):
            return {k: torch.zeros(12, 80) for k in ("speed", "acc", "ang_vel", "ang_acc")} | {"vertices": torch.zeros(12, 80, 4, 2), "center": torch.zeros(12, 80, 2)}

        def collision_matrix(self, *a, **kw):
            calls.append(kw)
            return torch.zeros(12, 40, dtype=torch.bool)

        def rollout_return(self, *a, **kw):
            calls.append(("return", a[6]))
            return torch.zeros(12, dtype=torch.float64)

        def group_advantage(self, r):
            return r

    with pytest.raises(ValueError, match="collision.*'sat'.*known.*envelope.*footprint"):
        TrajEvaluator(Eng(), collision="sat")
    off = np.zeros((12, 80), dtype=np.bool_)
    args = ((0, 0, 0, 6, 2, 4.6), torch.zeros(1, 12, 80, 6), [torch.zeros(5, 2)], [torch.zeros(5)])
    for mode, want in (("envelope", {"Ts": 40}), ("footprint", {"Ts": 40, "mode": "footprint"})):
        calls.clear()
        ev = TrajEvaluator(Eng(), collision=mode)
        ev.get_grpo_advantage(*args, other_vehicle_vertices=np.zeros((1, 40, 4, 2)), off_road_matrix=off)
        assert calls[0] == want
        calls.clear()
        mine = np.ones((12, 40), dtype=np.bool_)
        ev.get_grpo_advantage(*args, collision_matrix=mine, off_road_matrix=off)
        assert len(calls) == 1 and calls[0][0] == "return" and bool(calls[0][1].all())
    assert TrajEvaluator(Eng()).collision == "envelope"
