"""config['traj_eval']['off_road_extent'] on the group-relative policies, on the CPU: the key is read and validated, policies without a group
objective refuse it, an engine stub records what the policy asks of it -- without the key the tick call is the one made before, with it the
extent travels with the call, together with the map and the collision test -- and the per-CBV evaluator is built with the extent and hands
the rollout's corners to the lookup.  The device side is tests/test_gpu_offroad_extent.py."""
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
        keys = list(cls.TRAJ_EVAL_KEYS)
        assert 'off_road_extent' in keys and keys.index('off_road') < keys.index('off_road_extent') < keys.index('collision')
        assert cls._read_traj_eval(None) is None
        assert cls._read_traj_eval({})['off_road_extent'] is None
        for extent in ('center', 'footprint'):
            assert cls._read_traj_eval({'off_road_extent': extent})['off_road_extent'] == extent
        for bad in ('area', 'Footprint', 'centre', 1, ''):
            with pytest.raises(ValueError, match=r"traj_eval.*off_road_extent.*known.*'center'.*'footprint'"):
                cls._read_traj_eval({'off_road_extent': bad})


def test_unknown_key_message_lists_the_key_among_the_known_ones():
    from rift_amd.planning import CBV_POLICY_LIST
    with pytest.raises(ValueError, match="unknown key.*off_road_extend.*known.*off_road.*map_margin.*off_road_extent.*collision"):
        CBV_POLICY_LIST['rift_pluto']._read_traj_eval({'off_road_extend': 'footprint'})


def test_policies_without_a_group_objective_refuse_the_key():
    from rift_amd.planning import CBV_POLICY_LIST
    refused = 0
    for name, cls in CBV_POLICY_LIST.items():
        if getattr(cls, "GROUP_OBJECTIVE", False):
            continue
        for extent in ('center', 'footprint'):
            with pytest.raises(ValueError, match=rf"traj_eval.*off_road_extent.*rift_pluto, grpo_pluto.*{name} evaluates no group advantage"):
                cls({'num_scenario': 1, 'device': 'cpu', 'traj_eval': {'off_road_extent': extent}}, None)
        refused += 1
    assert refused >= 1 and not CBV_POLICY_LIST['pluto'].GROUP_OBJECTIVE


def test_without_the_key_the_tick_call_is_the_one_made_before(monkeypatch):
    for section in (None, {}, {'gamma': 0.9}, {'off_road': 'map'}, {'collision': 'footprint'}):
        pol, eng = _policy(section, monkeypatch)
        _tick(pol)
        (a, kw), = eng.ticks
        assert "off_road_extent" not in kw, section
        if section is None:
            assert (len(a), kw) == (3, {})
        else:
            want = {"params", "want_returns", "want_terms"} | ({"collision"} if "collision" in section else set())
            assert set(kw) == want and kw["params"] is pol._eval['params']


def test_with_the_key_the_extent_travels_with_the_tick_together_with_map_and_collision(monkeypatch):
    for extent in ('center', 'footprint'):
        pol, eng = _policy({'off_road_extent': extent}, monkeypatch)
        _tick(pol, (7, 9))
        (a, kw), = eng.ticks
        assert kw["off_road_extent"] == extent and "collision" not in kw and kw["params"] is pol._eval['params'] and eng.loads == []
        assert all(v["raster"] is None and v["off_road"] is not None for v in a[1])
        pol, eng = _policy({'off_road_extent': extent, 'collision': 'footprint', 'off_road': 'map', 'raster_size': (200, 300)}, monkeypatch)
        _tick(pol)
        (a, kw), = eng.ticks
        assert kw["off_road_extent"] == extent and kw["collision"] == 'footprint' and eng.loads == [5]
        assert a[1][0]["off_road"] is None and a[1][0]["raster"] == (200, 300) and a[1][0]["pose"] == (8.5, 2.5, 0.25)


def test_the_engine_makes_the_call_of_before_for_the_centre(monkeypatch):
    """Engine.group_advantage_tick picks riftof_group_advantage_tick only when the extent is not 'center': with None or 'center' the entry and
    its arguments are those of the call without the argument."""
    from rift_amd import _ffi, tick_pack
    calls = []

    class Lib:
        def __getattr__(self, name):
            def fn(*a):
                calls.append((name, len(a), [type(x).__name__ for x in a[12:-1]]))
                return 0
            return fn

    eng = _ffi.Engine.__new__(_ffi.Engine)
    eng.lib, eng.ctx, eng.device = Lib(), None, torch.device("cpu")
    monkeypatch.setattr(_ffi.Engine, "stage", lambda self, blob, dtype: torch.as_tensor(np.asarray(blob)).clone(), raising=False)
    monkeypatch.setattr(_ffi.Engine, "_check", lambda self, rc, name: None, raising=False)
    monkeypatch.setattr(_ffi, "_stream", lambda: None)
    monkeypatch.setattr(_ffi, "_dev", lambda t, dtype, dev: torch.as_tensor(t, dtype=dtype))
    monkeypatch.setattr(tick_pack, "fill_tick_cbvs", lambda layout, base: None)
    entry = {"batch_index": 0, "center_state": (0.0, 0.0, 0.0, 6.0, 2.0, 4.6), "ref_pos": [np.zeros((5, 2), dtype=np.float32)],
             "ref_angle": [np.zeros(5, dtype=np.float32)], "actors": None, "off_road": None}
    pid = {k: torch.zeros(256, 4) for k in ("turn_buf", "turn_ptr", "turn_len", "speed_buf", "speed_ptr", "speed_len")}
    traj = torch.zeros(1, 1, 12, 80, 6)

    def call(**kw):
        calls.clear()
        eng.group_advantage_tick(traj, [entry], pid, **kw)
        (c,), = [calls[:]]
        return c

    assert call()[0] == "rift_group_advantage_tick" == call(off_road_extent=None)[0] == call(off_road_extent="center")[0]
    assert call(off_road_extent="center") == call()
    assert call(off_road_extent="center", collision="footprint") == call(collision="footprint") and call(collision="footprint")[0] == "riftfp_group_advantage_tick"
    assert call(off_road_extent="center", want_returns=True) == call(want_returns=True) and call(want_returns=True)[0] == "rift_group_advantage_tick_ex"
    name, n, tail = call(off_road_extent="footprint")
    assert (name, n) == ("riftof_group_advantage_tick", 19) and tail[:3] == ["CArgObject", "CArgObject", "CArgObject"]
    assert call(off_road_extent="footprint", collision="footprint")[:2] == ("riftof_group_advantage_tick", 19)
    with pytest.raises(ValueError, match="extent.*'area'.*known.*center.*footprint"):
        call(off_road_extent="area")


def test_the_evaluator_of_the_chain_is_built_with_the_extent(monkeypatch):
    """The non-fused path: TrajEvaluator(..., off_road_extent=extent); without the key it is built without the argument."""
    from rift_amd.planning.fine_tuner.rlft.traj_eval import traj_evaluator as te
    from rift_amd.planning import CBV_POLICY_LIST
    made = []

    class Stub:
        def __init__(self, engine, **kw):
            made.append(kw)
            self.engine = engine

    monkeypatch.setattr(te, "TrajEvaluator", Stub)
    for section, want in ((None, None), ({'gamma': 0.9}, None), ({'collision': 'footprint'}, None), ({'off_road_extent': 'center'}, 'center'),
                          ({'off_road_extent': 'footprint'}, 'footprint')):
        cfg = {'num_scenario': 1, 'device': 'cpu', 'state_source': _Source()}
        if section is not None:
            cfg['traj_eval'] = section
        pol = CBV_POLICY_LIST['rift_pluto'](cfg, None)
        monkeypatch.setattr(pol.pluto_model, "engine", lambda: "engine", raising=False)
        monkeypatch.setattr(type(pol.pluto_model), "_engine", None, raising=False)
        pol.traj_evaluator
        assert made[-1].get("off_road_extent") == want and ("off_road_extent" in made[-1]) == (want is not None), section


def test_evaluator_takes_the_extent_and_hands_the_corners_to_the_lookup():
    """TrajEvaluator(off_road_extent=...): an unknown extent raises and names the two; 'center' makes the lookups' calls of before,
    'footprint' passes the rollout's vertices and the extent, for the raster and for the map; a caller-supplied off_road_matrix is not replaced."""
    from rift_amd.planning.fine_tuner.rlft.traj_eval.traj_evaluator import TrajEvaluator
    calls = []
    vertices = torch.zeros(12, 80, 4, 2)

    class Eng:
        def new_pid_state(self, n):
            return {}

        def ref_line_info(self, *a, **kw):
            return torch.zeros(12, 40), torch.zeros(12, 40), None

        def rollout(self, *a, **kw):
            return {k: torch.zeros(12, 80) for k in ("speed", "acc", "ang_vel", "ang_acc")} | {"vertices": vertices, "center": torch.zeros(12, 80, 2)}

        def eval_params(self, **kw):
            return "params"

        def off_road_matrix(self, *a, **kw):
            calls.append(("raster", kw))
            return torch.zeros(12, 80, dtype=torch.bool)

        def off_road_matrix_map(self, *a, **kw):
            calls.append(("map", kw))
            return torch.zeros(12, 80, dtype=torch.bool)

        def rollout_return(self, *a, **kw):
            calls.append(("return", a[7]))
            return torch.zeros(12, dtype=torch.float64)

        def group_advantage(self, r):
            return r

    with pytest.raises(ValueError, match="off_road_extent.*'area'.*known.*center.*footprint"):
        TrajEvaluator(Eng(), off_road_extent="area")
    col = np.zeros((12, 40), dtype=np.bool_)
    args = ((0, 0, 0, 6, 2, 4.6), torch.zeros(1, 12, 80, 6), [torch.zeros(5, 2)], [torch.zeros(5)])
    for extent in ("center", "footprint"):
        ev = TrajEvaluator(Eng(), off_road_extent=extent)
        calls.clear()
        ev.get_grpo_advantage(*args, collision_matrix=col, off_road_mask=np.zeros((400, 400), dtype=np.uint8), center_pose=(0.0, 0.0, 0.0))
        ev.get_grpo_advantage(*args, collision_matrix=col, drivable_map=True, center_pose=(0.0, 0.0, 0.0))
        looked = [c for c in calls if c[0] != "return"]
        assert [c[0] for c in looked] == ["raster", "map"]
        for _, kw in looked:
            if extent == "center":
                assert "vertices" not in kw and "extent" not in kw and "which" not in kw
            else:
                assert kw["vertices"] is vertices and kw["extent"] == "footprint" and "which" not in kw
        calls.clear()
        mine = np.ones((12, 80), dtype=np.bool_)
        ev.get_grpo_advantage(*args, collision_matrix=col, off_road_matrix=mine)
        assert len(calls) == 1 and calls[0][0] == "return" and bool(calls[0][1].all())
    assert TrajEvaluator(Eng()).off_road_extent == "center"
