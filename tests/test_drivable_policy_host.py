"""config['traj_eval'] = {'off_road': 'map'} on the group-relative policies, on the CPU: an engine stub records what the policy asks of it --
the map is loaded when the source's key changes and not per tick, poses go up instead of masks, a source without the two methods is named,
and a policy without a group advantage refuses the key.  The device side is tests/test_gpu_drivable_map.py."""
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
        self.loads.append((len(polygons), cell, margin))
        return {"n_polys": len(polygons)}

    def group_advantage_tick(self, *a, **kw):
        self.ticks.append((a, kw))
        return torch.zeros(len(a[1]), a[0].shape[1], 12, dtype=torch.float64)


class _Source:
    def __init__(self, key="Town05", polygons=None):
        self.key, self.polygons, self.rasters = key, D.lane_map(2, 5) if polygons is None else polygons, 0

    def nearby_actor_states(self, env_id, cbv_id):
        from rift_amd.planning.pluto.pluto import NoFlagSource
        return NoFlagSource.ALL_CLEAR

    def off_road_raster(self, env_id, cbv_id):
        self.rasters += 1
        return np.ones((400, 400), dtype=np.uint8), (1.0, 2.0, 0.3)

    def drivable_area(self, env_id):
        return None if self.key is None else (self.key, self.polygons)

    def off_road_pose(self, env_id, cbv_id):
        return 1.5 + cbv_id, 2.5, 0.25


def _policy(section, src, monkeypatch, name='rift_pluto'):
    from rift_amd.planning import CBV_POLICY_LIST
    cfg = {'num_scenario': 1, 'device': 'cpu', 'state_source': src}
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


def test_map_mode_loads_once_per_town_and_sends_poses(monkeypatch):
    src = _Source()
    pol, eng = _policy({'off_road': 'map', 'raster_size': (200, 300), 'map_cell': 8.0, 'map_margin': 1.5}, src, monkeypatch)
    _tick(pol, (7, 9))
    _tick(pol, (7,))
    assert eng.loads == [(5, 8.0, 1.5)] and src.rasters == 0          # one load for two ticks; no raster drawn
    (a, kw), _ = eng.ticks
    assert kw["params"] is pol._eval['params']
    for v, c in zip(a[1], (7, 9)):
        assert v["off_road"] is None and v["raster"] == (200, 300) and v["pose"] == (1.5 + c, 2.5, 0.25)
    src.key = "Town10"                                                 # the next town: the next load
    _tick(pol)
    assert eng.loads == [(5, 8.0, 1.5), (5, 8.0, 1.5)]
    _tick(pol)
    assert len(eng.loads) == 2
    # defaults of the three optional keys
    pol, eng = _policy({'off_road': 'map'}, _Source(), monkeypatch)
    _tick(pol)
    assert eng.loads == [(5, 16.0, 1.0)] and eng.ticks[0][0][1][0]["raster"] == (400, 400)


def test_raster_mode_and_no_key_make_the_call_made_before(monkeypatch):
    for section in (None, {'off_road': 'raster'}):
        src = _Source()
        pol, eng = _policy(section, src, monkeypatch)
        _tick(pol)
        (a, kw), = eng.ticks
        assert eng.loads == [] and src.rasters == 1
        v = a[1][0]
        assert v["off_road"] is not None and v["raster"] is None and v["pose"] is None
        assert (len(a), kw) == (3, {}) if section is None else "params" in kw


def test_refusals(monkeypatch):
    from rift_amd.planning import CBV_POLICY_LIST
    with pytest.raises(ValueError, match="off_road.*'drawn'.*known.*map.*raster"):
        _policy({'off_road': 'drawn'}, _Source(), monkeypatch)
    pol, _ = _policy({'off_road': 'map'}, _Source(key=None), monkeypatch)
    with pytest.raises(RuntimeError, match="_Source.drivable_area returned None"):
        _tick(pol)

    class Old:                                                          # a source written before the two methods existed
        nearby_actor_states = _Source.nearby_actor_states
        off_road_raster = _Source.off_road_raster

    pol, _ = _policy({'off_road': 'map'}, Old(), monkeypatch)
    with pytest.raises(RuntimeError, match="Old.drivable_area"):
        _tick(pol)

    class Half(Old):
        def drivable_area(self, env_id):
            return "t", D.lane_map(2, 3)

    pol, _ = _policy({'off_road': 'map'}, Half(), monkeypatch)
    with pytest.raises(RuntimeError, match="Half has no off_road_pose"):
        _tick(pol)
    # the base class: drivable_area defaults to None, off_road_pose names itself
    from rift_amd.planning.pluto.pluto import CBVStateSource
    assert CBVStateSource().drivable_area(0) is None
    with pytest.raises(NotImplementedError, match="off_road_pose"):
        CBVStateSource().off_road_pose(0, 1)
    # any other policy refuses the key, as it does for `objective`
    for name in CBV_POLICY_LIST:
        if name in ('rift_pluto', 'grpo_pluto'):
            continue
        with pytest.raises(ValueError, match=r"traj_eval.*off_road.*rift_pluto, grpo_pluto"):
            CBV_POLICY_LIST[name]({'num_scenario': 1, 'device': 'cpu', 'traj_eval': {'off_road': 'map'}}, None)
