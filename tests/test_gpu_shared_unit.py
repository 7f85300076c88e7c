"""The operand-format-free entries (rift_amd/csrc/shared.hip: one definition per library) called through contexts of BOTH engine builds alive
in one process: a bf16-operand and an fp16-operand Engine.  The entries' code is the same whatever context they are given, so the two
answer bit for bit; what belongs to a context (last error, profiler record, destructor) stays with that context.  Tiny shapes, chosen for
the kernels' edges: a tail workgroup and an odd group size, one element and one past a 256-thread pass, one row past a 16-row tile.
Nothing here provokes a fault: every call is a valid one or a refusal decided on the host."""
import ctypes as C

import pytest
import torch

from rift_amd import _ffi
from rift_amd import synthetic as syn
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pair():
    engs = {"bf16": _ffi.Engine(DEV, operands="bf16"), "fp16": _ffi.Engine(DEV, operands="fp16")}
    assert [e.lib.rift_ctx_operand_format(e.ctx) for e in engs.values()] == [_ffi.OPERANDS["bf16"], _ffi.OPERANDS["fp16"]]
    yield engs
    torch.cuda.synchronize()
    for e in engs.values():
        e.close()


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what      # (bit patterns: a NaN equals itself)


def _two_tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(DEV) for n in (1, 300)]


def test_both_contexts_answer_bit_for_bit(pair):
    g = torch.Generator().manual_seed(18)
    returns = torch.randn(3, 5, generator=g, dtype=torch.float64).to(DEV)           # 3 groups (4 per workgroup: a tail workgroup), odd G
    norm_in = {n: torch.randn(n, generator=g).to(DEV) for n in (1, 257)}            # one element; one past a 256-thread pass
    csd = {k: v.to(DEV) for k, v in H.critic_weights().items()}
    state = H.critic_inputs(17)["state"].to(DEV)                                    # one row past a 16-row tile
    got = {}
    for name, eng in pair.items():
        r = {"group_advantage": eng.group_advantage(returns).clone()}
        for n, x in norm_in.items():
            r[f"normalize_{n}"] = eng.normalize_advantage_(x.clone())
        r["critic_forward"] = eng.critic_forward(csd, state).clone()
        p, grads = _two_tensors(1), _two_tensors(2)
        m, v = ([torch.zeros_like(t) for t in p] for _ in range(2))
        steps = [torch.zeros(1, device=DEV) for _ in p]
        eng.adamw_step_raw(eng.make_adam_list(p, grads, m, v, steps), [1e-3, 2e-3], [0.01, 0.0], 1.0, 0.9, 0.999, 1e-8)
        for k, ts in (("adam_p", p), ("adam_m", m), ("adam_v", v), ("adam_step", steps)):
            for i, t in enumerate(ts):
                r[f"{k}{i}"] = t
        clipped, tn = _two_tensors(3), torch.full((1,), -1.0, device=DEV)
        eng.clip_grad_norm_raw(eng.make_clip_list(clipped), 0.5, tn)
        r["clip0"], r["clip1"], r["clip_norm"] = clipped[0], clipped[1], tn
        torch.cuda.synchronize()
        got[name] = r
    assert set(got["bf16"]) == set(got["fp16"])
    for k in got["bf16"]:
        _same_bits(got["bf16"][k], got["fp16"][k], k)
    # (the calls did something: the advantages are not the returns, the parameters moved, the norm was written, the gradients were scaled)
    assert not torch.equal(got["bf16"]["group_advantage"], returns) and float(got["bf16"]["clip_norm"]) > 0.5
    assert not torch.equal(got["bf16"]["adam_p1"], _two_tensors(1)[1]) and not torch.equal(got["bf16"]["clip1"], _two_tensors(3)[1])
    assert float(got["bf16"]["adam_step0"]) == 1.0


@pytest.mark.parametrize("refused, other", [("bf16", "fp16"), ("fp16", "bf16")])
def test_a_refusal_stays_with_its_context(pair, refused, other):
    """rift_control_tick with two CBVs on the one slot there is: refused on the host, before any launch; the message is that context's."""
    eng, quiet = pair[refused], pair[other]
    traj = torch.zeros(1, 1, 12, 20, 6, device=DEV)
    prob = torch.zeros(1, 1, 12, device=DEV)
    assert quiet.control_tick(traj, prob, None, []).shape == (0, 8)      # (an accepted tick, here an empty one, leaves an empty message)
    state = torch.zeros(1, _ffi.CONTROL_STATE, dtype=torch.float64, device=DEV)
    dec = torch.full((2, 8), -7.0, dtype=torch.float64, device=DEV)
    cbvs = (_ffi.RiftControlCBV * 2)()
    for t in cbvs:
        t.batch_index, t.slot, t.x, t.y, t.heading, t.speed = 0, 0, 0.0, 0.0, 0.0, 1.0
    rc = eng.lib.rift_control_tick(eng.ctx, traj.data_ptr(), prob.data_ptr(), None, 1, 20, cbvs, 2, 1, 10, state.data_ptr(), 1, dec.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1
    assert (eng.lib.rift_last_error(eng.ctx) or b"").decode() == "rift_control_tick: two CBVs with the same slot"
    assert (quiet.lib.rift_last_error(quiet.ctx) or b"") == b""
    assert bool((dec == -7.0).all()) and not bool(state.any())


def test_launch_bookkeeping_reaches_the_shared_unit_through_the_core(pair):
    """The profiler switch of the fp16 context records the shared unit's launch on that context; the bf16 context's record stays empty."""
    eng = pair["fp16"]
    eng.prof_enable(True)
    try:
        p, grads = _two_tensors(1), _two_tensors(2)
        m, v = ([torch.zeros_like(t) for t in p] for _ in range(2))
        steps = [torch.zeros(1, device=DEV) for _ in p]
        eng.adamw_step_raw(eng.make_adam_list(p, grads, m, v, steps), [1e-3, 2e-3], [0.01, 0.0], 1.0, 0.9, 0.999, 1e-8)
        report = eng.prof_report()
    finally:
        eng.prof_enable(False)
    assert list(report) == ["adamw_kernel"] and report["adamw_kernel"]["count"] == 1
    assert pair["bf16"].prof_report() == {}


def test_contexts_of_both_formats_are_destroyed_by_their_own_build():
    """Both formats load a model and run a forward at batch 1; the fp16 context goes first, then the bf16 one; a new context of each format
    still loads and runs.  (Each build's table entry deletes its own context type.)"""
    sd = {k: v.to(DEV) for k, v in H.weights().items()}
    feat = syn.collate_scenes([syn.make_scene(7318, r_min=1, r_max=3)])["cur_pluto_feature_torch"]

    def run(operands):
        eng = _ffi.Engine(DEV, operands=operands)
        eng.load_state_dict(sd)
        out = eng.forward(feat, no_drop=True, bn_update=False)["probability"].clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        return eng, out

    bf, out_bf = run("bf16")
    hf, out_hf = run("fp16")
    hf.close()
    bf.close()
    torch.cuda.synchronize()
    for operands, want in (("fp16", out_hf), ("bf16", out_bf)):
        eng, out = run(operands)
        assert torch.equal(out, want), operands
        eng.close()
