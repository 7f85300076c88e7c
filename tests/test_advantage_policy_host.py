"""config['advantage'] of the group-relative policies on the host, with a fake engine (as tests/test_eval_params_host.py does for
config['traj_eval']): the ticks ask for the returns and keep them in the column, the rollout buffer and the replay carry them as
'group_return', the update makes one arena_advantage call over the arena -- and without the key every call and column is today's.  No GPU."""
import types

import numpy as np
import pytest
import torch

R, RB = 2, 2          # valid reference lines of the one CBV, rows of the tick's batch


class _Engine:
    """An engine stub: records how group_advantage_tick and arena_advantage are called."""

    def __init__(self):
        self.ticks, self.arena = [], []

    def group_advantage_tick(self, *a, **kw):
        self.ticks.append((a, kw))
        K, Rb = len(a[1]), a[0].shape[1]
        n = K * Rb * 12
        if kw.get("want_returns") or kw.get("want_terms"):
            packed = torch.arange(n * 10, dtype=torch.float64)
            res = {"packed": packed, "advantage": packed[:n].view(K, Rb, 12)}
            if kw.get("want_returns"):
                res["returns"] = packed[n:2 * n].view(K, Rb, 12)
            if kw.get("want_terms"):
                res["terms"] = packed[2 * n:].view(K, Rb, 12, 8)
            return res
        return torch.arange(n, dtype=torch.float64).view(K, Rb, 12)

    def arena_advantage(self, *a, **kw):
        self.arena.append((a, kw))
        return kw["out"], torch.arange(8, dtype=torch.float64)


def _tick(monkeypatch, **sections):
    """One train-mode tick of rift_pluto with one CBV under config[sections]; -> (policy, engine stub, chain calls, the CBV's column)."""
    import rift_amd.synthetic as syn
    from rift_amd.planning import CBV_POLICY_LIST
    from rift_amd.planning.pluto.feature_builder.pluto_feature import PlutoFeature
    from rift_amd.planning.pluto.pluto import CenterState, NoFlagSource

    class Source:
        def nearby_actor_states(self, env_id, cbv_id):
            return NoFlagSource.ALL_CLEAR

        def off_road_raster(self, env_id, cbv_id):
            return NoFlagSource.ALL_CLEAR

    pol = CBV_POLICY_LIST['rift_pluto'](dict({'num_scenario': 1, 'device': 'cpu', 'state_source': Source()}, **sections), None)
    pol.mode = 'train'
    eng, chain = _Engine(), []

    def get_grpo_advantage(*a, **kw):
        chain.append((a, kw))
        out = {"advantage": torch.arange(R * 12, dtype=torch.float64).view(R, 12), "valid_mask": np.ones((R, 12), dtype=np.bool_)}
        if kw.get("return_terms") or kw.get("return_returns"):
            out["returns"] = 100.0 + torch.arange(R * 12, dtype=torch.float64).view(R, 12)
        if kw.get("return_terms"):
            out["terms"] = torch.zeros(R, 12, 8, dtype=torch.float64)
        return out

    pol._traj_evaluator = types.SimpleNamespace(engine=eng, pid_state={}, get_grpo_advantage=get_grpo_advantage)
    monkeypatch.setattr(type(pol.pluto_model), "_engine", None, raising=False)
    feat = syn.make_scene(5001, num_agents=12, num_polygons=8, r_min=R, r_max=R)["feature"]
    obs = {7: {'raw_pluto_feature': PlutoFeature(data=feat)}}
    out = {"trajectory": torch.zeros(1, RB, 12, 80, 6)}
    pol._begin_env(0, obs, None, out, {7: CenterState(1.0, 2.0, 0.3, 6.0, 2.0, 4.6)})
    column = pol._tick_columns[7]
    pol._finish_columns({})
    return pol, eng, chain, column


def test_unknown_keys_and_names_are_refused():
    from rift_amd.planning import CBV_POLICY_LIST
    base = {'num_scenario': 1, 'device': 'cpu'}
    with pytest.raises(ValueError, match=r"config\['advantage'\]: unknown key.*clipp.*known.*baseline.*scale.*clip.*eps"):
        CBV_POLICY_LIST['rift_pluto'](dict(base, advantage={'clipp': 1.0}), None)
    with pytest.raises(ValueError, match="baseline.*loo.*known.*mean.*leave_one_out.*none"):
        CBV_POLICY_LIST['grpo_pluto'](dict(base, advantage={'baseline': 'loo'}), None)
    with pytest.raises(ValueError, match="scale.*std.*known.*group_std.*batch_rms.*none"):
        CBV_POLICY_LIST['rift_pluto'](dict(base, advantage={'scale': 'std'}), None)
    pol = CBV_POLICY_LIST['rift_pluto'](dict(base, advantage={}), None)
    p = pol._advantage['params']
    assert (p.baseline, p.scale, p.eps, p.clip) == (0, 0, 1e-5, 0.0)
    pol = CBV_POLICY_LIST['rift_pluto'](dict(base, advantage={'baseline': 'leave_one_out', 'scale': 'batch_rms', 'clip': 1.5, 'eps': 0.0}), None)
    p = pol._advantage['params']
    assert (p.baseline, p.scale, p.eps, p.clip) == (1, 1, 0.0, 1.5)
    assert CBV_POLICY_LIST['rift_pluto'](base, None)._advantage is None


def test_fused_tick_asks_for_the_returns_and_the_column_carries_them(monkeypatch):
    from rift_amd import _ffi
    raw = lambda p: bytes(memoryview(p))  # noqa: E731
    n = RB * 12
    # without config['traj_eval']: the _ex entry under the default parameters
    _, eng, chain, col = _tick(monkeypatch, advantage={})
    (a, kw), = eng.ticks
    assert not chain and len(a) == 4 and a[3] == 0.98 and kw["want_returns"] is True and kw["want_terms"] is False
    assert raw(kw["params"]) == raw(_ffi.eval_params())
    assert set(col) == {"advantage", "valid_mask", "returns"}
    assert np.array_equal(col["advantage"], np.arange(n, dtype=np.float64).reshape(RB, 12)[:R])
    assert np.array_equal(col["returns"], (n + np.arange(n, dtype=np.float64)).reshape(RB, 12)[:R]) and col["returns"].dtype == np.float64
    # with it: its parameters, the returns on top
    pol, eng, _, col = _tick(monkeypatch, advantage={'clip': 1.5}, traj_eval={'gamma': 0.9})
    (a, kw), = eng.ticks
    assert a[3] == 0.9 and kw["params"].gamma == 0.9 and kw["want_returns"] is True and kw["want_terms"] is False
    assert "returns" in col and pol.last_tick_breakdown == {}
    # with the breakdown: returns and terms, both uses served by the one read-back
    pol, eng, _, col = _tick(monkeypatch, advantage={}, traj_eval={'breakdown': True})
    (a, kw), = eng.ticks
    assert kw["want_returns"] is True and kw["want_terms"] is True
    assert np.array_equal(col["returns"], pol.last_tick_breakdown[7]["returns"]) and pol.last_tick_breakdown[7]["terms"].shape == (R, 12, 8)


def test_chain_tick_asks_for_the_returns_and_the_column_carries_them(monkeypatch):
    _, eng, chain, col = _tick(monkeypatch, advantage={}, fused_tick=False)
    (a, kw), = chain
    assert not eng.ticks and kw["return_returns"] is True and "return_terms" not in kw
    assert np.array_equal(col["advantage"], np.arange(R * 12, dtype=np.float64).reshape(R, 12))
    assert np.array_equal(col["returns"], 100.0 + np.arange(R * 12, dtype=np.float64).reshape(R, 12))
    pol, _, chain, col = _tick(monkeypatch, advantage={}, fused_tick=False, traj_eval={'breakdown': True})
    (a, kw), = chain
    assert kw["return_terms"] is True and "returns" in col and np.array_equal(pol.last_tick_breakdown[7]["returns"], col["returns"])


def test_without_the_key_the_calls_and_columns_are_todays(monkeypatch):
    pol, eng, chain, col = _tick(monkeypatch)
    (a, kw), = eng.ticks
    assert len(a) == 3 and kw == {} and not chain and set(col) == {"advantage", "valid_mask"} and pol._advantage is None
    _, eng, _, col = _tick(monkeypatch, traj_eval={})
    (a, kw), = eng.ticks
    assert len(a) == 4 and kw["want_returns"] is False and kw["want_terms"] is False and set(col) == {"advantage", "valid_mask"}
    _, eng, chain, col = _tick(monkeypatch, fused_tick=False)
    (a, kw), = chain
    assert not eng.ticks and "return_returns" not in kw and "return_terms" not in kw and set(col) == {"advantage", "valid_mask"}
    # and the update calls nothing
    fake = _Engine()
    assert pol.preprocess_buffer(types.SimpleNamespace(engine=fake), types.SimpleNamespace(t={}, r_count=None)) == {} and not fake.arena


def _scene(i, with_return=True):
    import rift_amd.synthetic as syn
    feat = syn.make_scene(6000 + i, num_agents=6, num_polygons=4, r_min=1 + i % 3, r_max=1 + i % 3)["feature"]
    Ri = feat["reference_line"]["position"].shape[0]
    ex = {"group_advantage": np.full((Ri, 12), 0.5), "group_advantage_mask": np.ones((Ri, 12), dtype=np.bool_),
          "old_group_logits": np.zeros((Ri, 12), dtype=np.float32)}
    if with_return:
        ex["group_return"] = (i + np.arange(Ri * 12, dtype=np.float64) / 7.0).reshape(Ri, 12)
    return feat, ex


def test_buffer_and_replay_carry_the_returns():
    from rift_amd.gym_carla.buffer.cbv_rollout_buffer import CBVRolloutBuffer
    from rift_amd.planning.pluto.feature_builder.pluto_feature import PlutoFeature
    from rift_amd.replay import DeviceReplay, HostReplay
    feat, ex = _scene(1)
    col = {"advantage": ex["group_advantage"], "valid_mask": ex["group_advantage_mask"], "returns": ex["group_return"]}
    row = {'CBVs_obs': {'raw_pluto_feature': PlutoFeature(data=feat)}, 'CBVs_group_advantage': col}
    _, got = CBVRolloutBuffer._row_scene(row, 'CBVs_obs')
    assert np.array_equal(got["group_return"], ex["group_return"])
    row['CBVs_group_advantage'] = {k: v for k, v in col.items() if k != "returns"}
    assert "group_return" not in CBVRolloutBuffer._row_scene(row, 'CBVs_obs')[1]
    # the host replay allocates the field when a scene brings it
    host = HostReplay(4, pin=False)
    for i in range(4):
        host.put(i, *_scene(i, with_return=False))
    assert "group_return" not in host.t and host.has_group_return() is False
    dev = DeviceReplay.from_host(host, "cpu")
    assert "group_return" not in dev.t
    for i in range(4):
        host.put(i, *_scene(i))
    t = host.t["group_return"]
    assert t.dtype == torch.float64 and tuple(t.shape) == (4, host.caps["R"], 12) and host.has_group_return() is True
    for i in range(4):
        want = _scene(i)[1]["group_return"]
        assert np.array_equal(t[i, :want.shape[0]].numpy(), want) and not t[i, want.shape[0]:].any()
    dev.upload(host)
    assert torch.equal(dev.t["group_return"], t) and dev.t["group_return"].shape == dev.t["group_advantage"].shape
    # a mixed replay is refused when it goes up, by the first row without the field
    host.put(2, *_scene(2, with_return=False))
    assert not host.t["group_return"][2].any()
    with pytest.raises(ValueError, match=r"row 2 carries no 'group_return'"):
        dev.upload(host)
    # the scene-list constructor carries it too
    scenes = [{"feature": f, "extras": {k: torch.as_tensor(v) for k, v in e.items()}} for f, e in (_scene(i) for i in range(3))]
    dev = DeviceReplay(scenes, "cpu")
    assert dev.t["group_return"].dtype == torch.float64 and dev.t["group_return"].shape == dev.t["group_advantage"].shape
    assert torch.equal(dev.t["group_return"][1, :2], scenes[1]["extras"]["group_return"])
    del scenes[1]["extras"]["group_return"]
    with pytest.raises(ValueError, match=r"scene 1 carries no 'group_return'"):
        DeviceReplay(scenes, "cpu")


def test_the_update_makes_one_arena_call_with_the_configured_parameters():
    from rift_amd.planning import CBV_POLICY_LIST
    pol = CBV_POLICY_LIST['rift_pluto']({'num_scenario': 1, 'device': 'cpu', 'advantage': {'scale': 'none', 'clip': 1.5}}, None)
    fake = _Engine()
    t = {"group_return": torch.zeros(3, 2, 12, dtype=torch.float64), "group_valid_mask": torch.ones(3, 2, 12, dtype=torch.bool),
         "group_advantage": torch.zeros(3, 2, 12, dtype=torch.float64)}
    replay = types.SimpleNamespace(t=t, r_count=torch.tensor([2, 1, 2], dtype=torch.int32))
    assert pol.preprocess_buffer(types.SimpleNamespace(engine=fake), replay) == {}
    (a, kw), = fake.arena
    assert a[0] is t["group_return"] and a[1] is replay.r_count and a[2] is t["group_valid_mask"] and kw["out"] is t["group_advantage"]
    assert kw["params"] is pol._advantage["params"] and (kw["params"].scale, kw["params"].clip) == (2, 1.5) and kw["want_stats"] is True
    assert torch.equal(pol._advantage_stats, torch.arange(8, dtype=torch.float64))
    del t["group_return"]
    with pytest.raises(ValueError, match=r"config\['advantage'\].*group_return"):
        pol.preprocess_buffer(types.SimpleNamespace(engine=fake), replay)
    assert len(fake.arena) == 1
