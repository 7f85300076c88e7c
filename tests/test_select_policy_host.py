"""config['action_selection'] of the policies on the host, with the forward and the engine stubbed (as tests/test_advantage_policy_host.py does
for config['advantage']): what the section may hold, when a tick samples (mode 'sample', train mode, not deterministic), that the policy
draws one uniform number per CBV and tick in the tick's CBV order on both paths, also when the ref-free rule fires -- and that without the
key no generator exists and rift_control_tick's entry is the one called.  No GPU."""
import types

import numpy as np
import pytest
import torch

from rift_amd.planning.pluto import inference as inf
from tests import helpers as H
from tests import select_cases as S

R, TOPK = 4, 10
BASE = {'num_scenario': 1, 'device': 'cpu', 'seed': 11}


class _Issued(Exception):
    """Raised by the engine stub once control_tick was recorded: what follows it in _issue_control (pinned memory, an event) needs a GPU."""


class _Engine:
    def __init__(self):
        self.calls = []

    def control_reset(self, slots):
        pass

    def control_tick(self, *a, **kw):
        self.calls.append((a, kw))
        raise _Issued()

    def check_finite(self):
        pass


def _outputs(ids, ref_free_wins=()):
    """Finished outputs of one forward for the CBVs `ids`: seeded candidates, logits with a learned candidate clearly above the ref-free score
    -- except for the CBVs in `ref_free_wins`, whose logits are flat (best score 0.1 < 0.25)."""
    cand, prob, rf = [], [], []
    for c in ids:
        inp = H.inference_inputs(seed=700 + c, R=R)
        p = inp["probability"].copy()
        p.reshape(-1)[[(13 * c) % 48, (13 * c + 17) % 48, (13 * c + 30) % 48]] = 4.0, 3.8, 3.6      # (best score about 0.36)
        if c in ref_free_wins:
            p[:] = 0.0
        cand.append(inp["candidates"]); prob.append(p); rf.append(inp["ref_free"])
    return {"candidate_trajectories": torch.as_tensor(np.stack(cand)), "probability": torch.as_tensor(np.stack(prob)),
            "output_ref_free_trajectory": torch.as_tensor(np.stack(rf)), "trajectory": torch.zeros(len(ids), R, 12, 80, 6)}


def _policy(name='ppo_pluto', mode='train', **cfg):
    from rift_amd.planning import CBV_POLICY_LIST
    from rift_amd.planning.pluto.pluto import CenterState

    class Source:
        def center_state(self, env_id, cbv_id):
            return CenterState(10.0 + cbv_id, -5.0, 0.3 - 0.1 * cbv_id, 4.0 + 0.3 * cbv_id, 2.0, 4.6)

    class Probe(CBV_POLICY_LIST[name]):
        ref_free_wins = ()

        def _forward(self, CBVs_obs):
            return None, _outputs(list(CBVs_obs), self.ref_free_wins)

    pol = Probe(dict(BASE, state_source=Source(), **cfg), None)
    pol.mode = mode                       # (set directly: set_mode('train') builds the training model, which no tick reads)
    pol.pluto_model._engine = _Engine()
    return pol


def _tick(pol, ids, deterministic=False):
    return pol.get_action([{c: {} for c in ids}], [{'env_id': 0}], deterministic=deterministic)


def test_unknown_keys_and_values_are_refused():
    from rift_amd.planning import CBV_POLICY_LIST
    for name in ('pluto', 'ppo_pluto', 'rift_pluto'):
        with pytest.raises(ValueError, match=r"config\['action_selection'\]: unknown key.*temp.*known.*mode.*temperature.*seed"):
            CBV_POLICY_LIST[name](dict(BASE, action_selection={'temp': 1.0}), None)
    with pytest.raises(ValueError, match=r"config\['action_selection'\]\['mode'\].*softmax.*known.*greedy.*sample"):
        CBV_POLICY_LIST['pluto'](dict(BASE, action_selection={'mode': 'softmax'}), None)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match=r"config\['action_selection'\]\['temperature'\]"):
            CBV_POLICY_LIST['pluto'](dict(BASE, action_selection={'mode': 'sample', 'temperature': bad}), None)
    for bad in (-1, 1.5, 'x', True):
        with pytest.raises(ValueError, match=r"config\['action_selection'\]\['seed'\]"):
            CBV_POLICY_LIST['pluto'](dict(BASE, action_selection={'mode': 'sample', 'seed': bad}), None)
    pol = CBV_POLICY_LIST['ppo_pluto'](dict(BASE, action_selection={'mode': 'sample'}), None)
    assert pol._selection == {'mode': 'sample', 'temperature': 1.0, 'seed': 11} and pol._select_rng is not None      # the seed defaults to the config's
    pol = CBV_POLICY_LIST['ppo_pluto'](dict(BASE, action_selection={'mode': 'sample', 'temperature': 0.5, 'seed': 3}), None)
    assert pol._selection == {'mode': 'sample', 'temperature': 0.5, 'seed': 3}
    pol = CBV_POLICY_LIST['ppo_pluto'](dict(BASE, action_selection={}), None)
    assert pol._selection['mode'] == 'greedy' and pol._select_rng is None
    assert CBV_POLICY_LIST['ppo_pluto'](BASE, None)._selection is None


def test_a_tick_samples_in_train_mode_unless_deterministic():
    ids = [1, 2, 3]
    greedy = _tick(_policy(), ids)
    on = {'action_selection': {'mode': 'sample', 'temperature': 1.0, 'seed': 5}}
    # the gate: each of the three conditions alone keeps the tick greedy, bit for bit, and draws nothing
    for pol, det in ((_policy(mode='eval', **on), False), (_policy(**on), True), (_policy(action_selection={'mode': 'greedy', 'seed': 5}), False)):
        state = None if pol._select_rng is None else pol._select_rng.bit_generator.state
        got = _tick(pol, ids, deterministic=det)
        assert got == greedy
        assert pol._select_rng is None or pol._select_rng.bit_generator.state == state
    # all three: the choice is sample_candidate's under the policy's own stream
    pol = _policy(**on)
    us = np.random.default_rng(5).random(2 * len(ids))
    moved = 0
    for t in range(2):
        got = _tick(pol, ids)
        out = _outputs(ids)
        for k, c in enumerate(ids):
            flat, pos, p = inf.sample_candidate(out["probability"][k].numpy(), TOPK, 1.0, us[t * len(ids) + k])
            assert tuple(got['CBVs_actions_mode'][0][c]) == divmod(flat, 12)
            assert got['CBVs_actions_old_log_prob'][0][c] == np.log(p + 1e-12)
            moved += tuple(got['CBVs_actions_mode'][0][c]) != tuple(greedy['CBVs_actions_mode'][0][c])
    assert moved >= 1                                          # (the seed is one under which sampling shows)
    # the executed candidate is the sampled one: the controls are those of a policy whose logits make that candidate the greedy choice
    pol = _policy(**on)
    got = _tick(pol, [2])
    flat = got['CBVs_actions_mode'][0][2][0] * 12 + got['CBVs_actions_mode'][0][2][1]

    class Forced(type(_policy())):
        def _forward(self, CBVs_obs):
            out = _outputs(list(CBVs_obs))
            out["probability"].view(len(CBVs_obs), -1)[0, flat] = 9.0
            return None, out

    forced = Forced(dict(BASE, state_source=pol.state_source), None)
    forced.pluto_model._engine = _Engine()
    assert _tick(forced, [2])['CBVs_actions'][0][2] == got['CBVs_actions'][0][2]


def test_a_drawn_candidate_that_trim_candidates_did_not_keep_is_still_executed(monkeypatch):
    """Equal logits at the edge of the kept set: sample_candidate keeps the lower flat index, trim_candidates (numpy's default sort) may keep
    another of them.  Here it is made to -- the lower one is nudged down in what trim_candidates sees -- and u points at the lower one: the
    policy executes it all the same, with the controls of a policy for which it is the greedy choice."""
    import rift_amd.planning.pluto.pluto as P
    on = {'action_selection': {'mode': 'sample', 'temperature': 1.0, 'seed': 1}}
    logits = _outputs([2])["probability"][0].numpy().copy()
    order = np.argsort(-logits.reshape(-1), kind="stable")
    low, high = sorted(int(j) for j in order[TOPK - 1:TOPK + 1])            # the last kept candidate and the first one left out
    tied = logits.copy()
    tied.reshape(-1)[[low, high]] = logits.reshape(-1)[order[TOPK - 1]]

    class Tied(type(_policy())):
        def _forward(self, CBVs_obs):
            out = _outputs(list(CBVs_obs))
            out["probability"][0] = torch.as_tensor(tied)
            return None, out

    real = P.trim_candidates

    def nudged(cand, prob, *a, **kw):
        if prob.size > 1:
            prob = prob.copy()
            prob.reshape(-1)[low] -= 1e-3
        return real(cand, prob, *a, **kw)

    monkeypatch.setattr(P, "trim_candidates", nudged)
    iv = {j: (lo, hi) for j, lo, hi in S.intervals({"logits": tied, "topk": TOPK, "temperature": 1.0})}
    assert low in iv and high not in iv
    pol = Tied(dict(BASE, state_source=_policy().state_source, **on), None)
    pol.mode, pol.pluto_model._engine = 'train', _Engine()
    pol._select_rng = types.SimpleNamespace(random=lambda n: np.full(n, 0.5 * sum(iv[low])))
    seen = []
    decide = pol._decide
    pol._decide = lambda *a: seen.append(decide(*a)) or seen[-1]
    got = _tick(pol, [2])
    assert tuple(got['CBVs_actions_mode'][0][2]) == divmod(low, 12)
    d = seen[0]             # trim_candidates kept `high`; the drawn `low` joined the kept set behind the ref-free entry, and kept[best] is what is executed
    assert d.flat_index.tolist()[TOPK:] == [-1, low] and high in d.flat_index.tolist()[:TOPK] and d.best == TOPK + 1 and d.chosen_flat == low
    assert d.kept.shape[0] == d.score.shape[0] == TOPK + 2 and np.array_equal(d.kept[d.best, 1:], d.trajectory)
    monkeypatch.setattr(P, "trim_candidates", real)

    class Forced(type(_policy())):
        def _forward(self, CBVs_obs):
            out = _outputs(list(CBVs_obs))
            out["probability"].view(len(CBVs_obs), -1)[0, low] = 9.0
            return None, out

    forced = Forced(dict(BASE, state_source=pol.state_source), None)
    forced.pluto_model._engine = _Engine()
    want = _tick(forced, [2])['CBVs_actions'][0][2]
    assert want[2] == got['CBVs_actions'][0][2][2] and np.abs(np.array(want[:2]) - np.array(got['CBVs_actions'][0][2][:2])).max() < 1e-12


def test_one_draw_per_cbv_and_tick_in_order_also_when_the_ref_free_rule_fires():
    on = {'action_selection': {'mode': 'sample', 'temperature': 2.0, 'seed': 9}}
    ids = [4, 5, 6]
    us = np.random.default_rng(9).random(9)
    # host path: CBV 5's ref-free candidate is executed, its number is consumed all the same
    pol = _policy(**on)
    pol.ref_free_wins = (5,)
    for t, these in enumerate([ids, [4, 6], ids, [6]]):
        at = {0: 0, 1: 3, 2: 5, 3: 8}[t]
        got = _tick(pol, these)
        out = _outputs(these, (5,))
        for k, c in enumerate(these):
            if c == 5:
                assert tuple(got['CBVs_actions_mode'][0][c]) == divmod(-1, 12) and got['CBVs_actions_old_log_prob'][0][c] == np.log(0.25 + 1e-12)
            else:
                flat, _, p = inf.sample_candidate(out["probability"][k].numpy(), TOPK, 2.0, us[at + k])
                assert tuple(got['CBVs_actions_mode'][0][c]) == divmod(flat, 12) and got['CBVs_actions_old_log_prob'][0][c] == np.log(p + 1e-12)
    assert pol._select_rng.random() == np.random.default_rng(9).random(10)[9]           # nine numbers were drawn, no more
    # device path: the same numbers, in the same order, ride with the one call of the environment
    pol = _policy(device_control=True, **on)
    eng = pol.pluto_model._engine
    for t, these in enumerate([ids, [4, 6]]):
        with pytest.raises(_Issued):
            _tick(pol, these)
        a, kw = eng.calls[t]
        assert kw["select"] == {'mode': 'sample', 'temperature': 2.0} and kw["topk"] == TOPK
        assert np.array_equal(kw["u"], us[3 * t:3 * t + len(these)]) and [v[0] for v in a[3]] == list(range(len(these)))
    # ... and a deterministic call on that path is rift_control_tick's
    with pytest.raises(_Issued):
        _tick(pol, ids, deterministic=True)
    assert "select" not in eng.calls[2][1] and "u" not in eng.calls[2][1]


def test_without_the_key_no_generator_exists_and_the_greedy_entry_is_called(monkeypatch):
    with monkeypatch.context() as m:
        m.setattr(np.random, "default_rng", lambda *a, **k: pytest.fail("a generator was made"))
        pol = _policy(device_control=True)
    assert pol._selection is None and pol._select_rng is None
    with pytest.raises(_Issued):
        _tick(pol, [1, 2])
    (a, kw), = pol.pluto_model._engine.calls
    assert set(kw) == {"topk", "sample_interval"}
    # the engine turns such a call into rift_control_tick, and one with `select` into riftcs_control_tick
    from rift_amd import _ffi
    eng = _ffi.Engine.__new__(_ffi.Engine)
    called = []

    def entry(name):
        def fn(*args):
            called.append((name, args))
            return 0
        return fn

    eng.lib = types.SimpleNamespace(rift_control_tick=entry("rift_control_tick"), riftcs_control_tick=entry("riftcs_control_tick"))
    eng.ctx, eng.device, eng._ctl_state = None, torch.device("cpu"), None
    eng._check = lambda rc, what: None
    monkeypatch.setattr(_ffi, "_stream", lambda: None)
    traj, prob = torch.zeros(1, R, 12, 80, 6), torch.zeros(1, R, 12)
    cbvs = [(0, 0, 1.0, 2.0, 0.3, 4.0), (0, 1, 1.0, 2.0, 0.3, 4.0)]
    eng.control_tick(traj, prob, None, cbvs)
    eng.control_tick(traj, prob, None, cbvs, select={'mode': 'sample', 'temperature': 0.5}, u=[0.25, 0.75])
    eng.control_tick(traj, prob, None, cbvs, select=_ffi.select_params())
    assert [n for n, _ in called] == ["rift_control_tick", "riftcs_control_tick", "riftcs_control_tick"]
    assert len(called[0][1]) == 14 and len(called[1][1]) == 16 and called[2][1][13] is None
    p = called[1][1][12]._obj
    assert (p.mode, p.reserved, p.temperature) == (1, 0, 0.5)
    with pytest.raises(ValueError, match="unknown key"):
        eng.control_tick(traj, prob, None, cbvs, select={'temp': 1.0})
    with pytest.raises(ValueError, match="1 numbers in `u` for 2 CBVs"):
        eng.control_tick(traj, prob, None, cbvs, select={'mode': 'sample'}, u=[0.5])
    with pytest.raises(ValueError, match="`u` is read with select"):
        eng.control_tick(traj, prob, None, cbvs, u=[0.5, 0.5])
