"""riftga_arena_advantage (include/rift_advantage.h) on the device: every case of tests/advantage_param_cases.py against its fp64
restatement, the default parameters against the existing z-score entry bit for bit, zeros outside the groups, run-to-run equality, and
one policy update under config['advantage'].  tests/test_advantage_param_cases.py checks on the CPU what the inputs must satisfy.  Needs a
real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

from tests import advantage_param_cases as A

pytestmark = pytest.mark.gpu

TOL = 1e-9            # max-abs on the advantage: the bar tests/test_gpu_small_kernels.py holds the z-score kernel to on these distributions
NAN_BYTE = 0xFF


@pytest.fixture(scope="module")
def eng():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    e = _ffi.Engine("cuda:0")
    yield e
    e.close()


def _device(c):
    T = lambda a: None if a is None else torch.from_numpy(a).cuda()  # noqa: E731
    return T(c["returns"]), T(c["r_count"]), T(c["mask"])


def _poisoned(ret):
    out = torch.empty_like(ret)
    out.view(torch.uint8).fill_(NAN_BYTE)
    assert torch.isnan(out).all()
    return out


@pytest.mark.parametrize("k", range(len(A.SHAPES)), ids=A.case_ids())
def test_every_case_against_the_restatement(eng, k):
    """Advantage 1e-9 max-abs; the counts of `stats` exact, its rms 1e-12 relative; what belongs to no group exactly 0 in an output
    pre-filled with NaN bytes; the call without `stats` gives the same bits as the call with."""
    from rift_amd import _ffi
    c = A.case(k)
    ret, rc, mask = _device(c)
    valid = A.valid_of(c)
    worst, ran = 0.0, 0
    for s in A.settings(k):
        if not A.is_case(c, *s):
            continue
        baseline, scale, clip, eps = s
        want, _, want_stats = A.restate(c, *s)
        p = _ffi.advantage_params(baseline, scale, clip=clip, eps=eps)
        got, stats = eng.arena_advantage(ret, rc, mask, params=p, out=_poisoned(ret), want_stats=True)
        plain = eng.arena_advantage(ret, rc, mask, params=p, out=_poisoned(ret))
        assert torch.equal(got, plain), s
        got, stats = got.cpu().numpy(), stats.cpu().numpy()
        assert np.isfinite(got).all(), s
        e = float(np.max(np.abs(got - want)))
        print(f"{A.case_ids()[k]} {c['mask_kind']:>12} {c['dist']:>8} {s}: {e:.2e}  stats {stats[:5].tolist()}")
        assert e < TOL, (s, e)
        assert np.all(got[~valid] == 0.0), s
        assert stats[[0, 1, 2, 4]].tolist() == want_stats[[0, 1, 2, 4]].tolist() and not stats[5:].any(), (s, stats, want_stats)
        assert abs(stats[3] - want_stats[3]) <= 1e-12 * abs(want_stats[3]), (s, stats[3], want_stats[3])
        worst, ran = max(worst, e), ran + 1
    assert ran >= 9
    print(f"{A.case_ids()[k]}: {ran} settings, max error {worst:.3e}")


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask_of_ones"])
def test_default_parameters_give_the_bits_of_the_zscore_entry(eng, masked):
    """Scenes whose valid lines are a fully valid prefix, under the default parameters: torch.equal to Engine.group_advantage on the
    scene's (1, r_count * 12) returns -- every shape of the table, both distributions; padded lines are exactly 0."""
    compared = 0
    for k in range(len(A.SHAPES)):
        c = A.case(k)
        if c["n"] > 9:
            continue
        for shifted in (False, True):
            ret = torch.from_numpy(-300.0 + 0.5 * c["returns"] if shifted else c["returns"]).cuda()
            rc = None if c["r_count"] is None else torch.from_numpy(c["r_count"]).cuda()
            mask = torch.full(ret.shape, 3, dtype=torch.uint8, device="cuda") if masked else None
            got = eng.arena_advantage(ret, rc, mask, out=_poisoned(ret))
            for i in range(c["n"]):
                r = c["Rcap"] if c["r_count"] is None else int(c["r_count"][i])
                assert not got[i, r:].any()
                if r:
                    assert torch.equal(got[i, :r].reshape(1, -1), eng.group_advantage(ret[i, :r].reshape(1, -1))), (k, shifted, i)
                    compared += 1
    assert compared > 150


def test_two_calls_give_the_same_bits(eng):
    from rift_amd import _ffi
    for k in (len(A.SHAPES) - 1, 24, 13):
        c = A.case(k)
        ret, rc, mask = _device(c)
        for scale in A.SCALES:
            p = _ffi.advantage_params("mean", scale, clip=1.5)
            a, sa = eng.arena_advantage(ret, rc, mask, params=p, want_stats=True)
            b, sb = eng.arena_advantage(ret, rc, mask, params=p, want_stats=True)
            assert torch.equal(a, b) and torch.equal(sa, sb), (k, scale)


def test_refusals_reach_the_caller_with_a_reason(eng):
    from rift_amd import _ffi
    ret = torch.zeros(2, 3, 12, dtype=torch.float64, device="cuda")
    p = _ffi.advantage_params()
    p.baseline = 5
    with pytest.raises(RuntimeError, match="riftga_arena_advantage.*baseline"):
        eng.arena_advantage(ret, params=p)
    with pytest.raises(RuntimeError, match="riftga_arena_advantage.*clip"):
        eng.arena_advantage(ret, params=_ffi.advantage_params(clip=-1.0))
    with pytest.raises(RuntimeError, match="riftga_arena_advantage.*advantage == returns"):
        eng.arena_advantage(ret, out=ret)
    assert eng.arena_advantage(torch.zeros(0, 3, 12, dtype=torch.float64, device="cuda")).shape == (0, 3, 12)


def _buffer_with_returns(eng, n):
    """A rift_pluto buffer of n synthetic scenes filled through store(): every candidate's return is drawn, the stored advantage is the
    existing entry's z-score of it (what the tick stores), and the column carries both."""
    import rift_amd.synthetic as syn
    from rift_amd.gym_carla.buffer.cbv_rollout_buffer import CBVRolloutBuffer
    from rift_amd.planning.pluto.feature_builder.pluto_feature import PlutoFeature
    keys = ['CBVs_obs', 'CBVs_reward', 'CBVs_done', 'CBVs_actions_old_group_logits', 'CBVs_group_advantage']
    buf = CBVRolloutBuffer(1, 'train_cbv', {'buffer_capacity': n, 'data_keys': keys})
    rng = np.random.default_rng(4242)
    t = 0
    while not buf.buffer_full:
        for k in range(8):
            s = syn.make_scene(9000 + t, num_agents=12, num_polygons=8, r_min=1, r_max=3)
            ex = s["extras"]
            Rs = ex["old_group_logits"].shape[0]
            ret = rng.standard_normal((Rs, 12)) * 2.0 - 1.0
            adv = eng.group_advantage(torch.from_numpy(ret).reshape(1, -1)).reshape(Rs, 12).cpu().numpy()
            buf.store({'CBV_ids': [[3]], 'CBVs_obs': [{3: {'raw_pluto_feature': PlutoFeature(data=s["feature"])}}],
                       'CBVs_reward': [{3: float(ex["return"])}], 'CBVs_done': [{3: k == 7}],
                       'CBVs_actions_old_group_logits': [{3: {'logits': ex["old_group_logits"].numpy(), 'valid_mask': ex["old_group_logits_mask"].numpy()}}],
                       'CBVs_group_advantage': [{3: {'advantage': adv, 'valid_mask': np.ones((Rs, 12), dtype=np.bool_), 'returns': ret}}]})
            t += 1
    return buf


def test_policy_update_under_the_advantage_settings(eng, tmp_path):
    """A 64-scene replay whose stored advantage is the z-score of its stored returns, two epochs: config['advantage'] = {} trains to the
    losses of the run without the key, bit for bit; {'scale': 'none', 'clip': 1.5} trains to other losses, and the arena's group_advantage
    is the restatement's."""
    from rift_amd.planning import CBV_POLICY_LIST
    hist, arena, fits = {}, {}, {}
    for name, section in (("without", None), ("default", {}), ("clipped", {'scale': 'none', 'clip': 1.5})):
        cfg = {'num_scenario': 1, 'ROOT_DIR': str(tmp_path / name), 'model_path': 'ckpt', 'device': 'cuda:0',
               'rlft': {'epochs': 2, 'warmup_epochs': 1, 'train_batch_size': 32, 'val_batch_size': 32, 'lr': 1e-3}}
        if section is not None:
            cfg['advantage'] = section
        torch.manual_seed(0)                   # (ahead of the policy: Conv1d biases of a fresh PlanningModel come from the global generator)
        pol = CBV_POLICY_LIST['rift_pluto'](cfg, None)
        with torch.no_grad():
            for p in pol.pluto_model.parameters():
                if p.dim() > 1:
                    p.normal_(0, 0.05)
        pol.load_model(resume=True)
        pol.set_mode('train')
        pol.set_buffer(_buffer_with_returns(eng, 64))
        fit = pol.train(3)
        hist[name] = [(h["train_loss"], h["val_loss"]) for h in fit["history"]]
        arena[name], fits[name] = pol._arenas['CBVs_obs'], fit
    assert len(hist["without"]) == 2 and all(np.isfinite(v) for h in hist["without"] for v in h)
    assert hist["default"] == hist["without"]
    assert hist["clipped"] != hist["without"]
    assert "advantage_stats" not in fits["without"] and len(fits["default"]["advantage_stats"]) == 8
    rep = arena["clipped"]
    c = {"n": rep.n, "Rcap": rep.Rcap, "returns": rep.t["group_return"].cpu().numpy(), "r_count": rep.r_count.cpu().numpy(),
         "mask": rep.t["group_valid_mask"].cpu().numpy().astype(np.uint8)}
    want, _, want_stats = A.restate(c, "mean", "none", 1.5, 1e-5)      # (the baseline stays the default: the mean)
    e = float(np.max(np.abs(rep.t["group_advantage"].cpu().numpy() - want)))
    print(f"arena advantage under scale none, clip 1.5: {e:.2e}; stats {fits['clipped']['advantage_stats']}")
    assert e < TOL and want_stats[4] > 0
    assert fits["clipped"]["advantage_stats"] == want_stats.tolist()
    assert torch.equal(arena["default"].t["group_advantage"], arena["without"].t["group_advantage"])
