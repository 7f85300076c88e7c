"""rift_loss_backward_ex (loss_kernel<MAXPL, true>, rift_amd/csrc/loss.h): the settings of the RIFT / GRPO objective at run time, on the
designed inputs of tests/objective_cases.py -- the four batches that hit every dispatch (`one`: G 12, 52 idle lanes; `std`: a second
workgroup with one live wave, G 72 across lanes 63 / 64; `dense`: <4>; `wide`: <16>) in the modes of tests/test_gpu_objectives.py.  The
references are tests/objective_param_cases.py's fp64 restatement on the DEVICE's q_final; tests/test_objective_param_cases.py proves on
the CPU that every setting used here moves that restatement by 100 loss bars and 25 - 50 gradient bars, so a kernel that ignores a field
fails.  Bars: |loss - ref| < 1e-5, max |g - ref| < 1e-5 + 1e-4 max |ref| per tensor.  Needs a real MI355X: `pytest -m gpu`.

MEASURED on MI355X (profiles/NOTES_r16.md has the table per setting and mode): MEASURED below."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import losses
from tests import helpers as H
from tests import objective_cases as O
from tests import objective_param_cases as P

pytestmark = pytest.mark.gpu

MODES = {"one": ("fp32", "bf16", "fp16"), "std": ("fp32", "bf16", "fp16"), "dense": ("fp32", "bf16"), "wide": ("fp32",)}
CASES = [(n, m) for n in P.ALL for m in MODES[n]]
KINDS = ("rift", "grpo")

MEASURED = """Worst over the batches of a mode (profiles/NOTES_r16.md has the table per setting): |loss - restatement| and the worst gradient
error in bars of its own tensor (1e-5 + 1e-4 max |ref|).
  kind   settings                         fp32                 default build (bf16)   fp16
  rift   every setting, combined          6.5e-07  0.100 bars  6.1e-07  0.060 bars    5.9e-07  0.152 bars
  grpo   every setting, combined          1.5e-06  0.750 bars  1.0e-06  0.273 bars    1.3e-06  0.688 bars
GRPO's gradients are the closest to the bar, on `one` as in tests/test_gpu_objectives.py (0.67 bars there): its head factor of 32 amplifies
the fp32 rounding of the logits; the settings add nothing to it (KL 0.1: 0.72, clip 0.7 / 1.3: 0.75, no KL: 0.63).  Every result is
at least 299 loss bars and 26 gradient bars (entropy 0.5 on RIFT; 77 elsewhere) from the restatement at the defaults.  Term sums: within
1.6e-6 per valid candidate, counts exact, identity with stats[0] to 1.3e-15 relative.  Bridge cross-check on `std`: 0.006 - 0.022 bars.
The defaults, the kind test and the fully masked batches are bit comparisons."""


@pytest.fixture(scope="module")
def engines():
    """get(mode, head factor) -> (engine, state dict): one engine per operand build and factor of O.spread_weights, made on demand."""
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    made = {}

    def get(mode, weights):
        key = ("fp16" if mode == "fp16" else "bf16", weights)
        if key not in made:
            sd = O.spread_weights(H.weights(), weights)
            eng = _ffi.Engine("cuda:0", operands=key[0])
            eng.load_state_dict({k: v.clone() for k, v in sd.items()})
            made[key] = (eng, sd)
        return made[key]

    yield get
    for eng, _ in made.values():
        eng.close()


def _forward(engines, name, mode, kind, variant=0):
    """One eval forward and the case built from the device's own logits: (engine, state dict, r_pad, q_final, case, info)."""
    eng, sd = engines(mode, O.head_scale(name, kind))
    b = O.batch(name)
    out = eng.forward(b["cur_pluto_feature_torch"], fp32=mode == "fp32")
    torch.cuda.synchronize()
    r_pad = O.line_padding(b)
    bs, R = r_pad.shape
    prob = out["probability"].cpu()
    assert prob.shape == (bs, R, O.M) and bool((prob[r_pad] == -1e6).all()) and bool(torch.isfinite(prob).all())
    c, info = P.build_case(name, kind, prob, r_pad, variant)
    info["ratios"] = O.realised_ratios(prob, r_pad, c["old_group_logits_torch"])
    return eng, sd, r_pad, eng.tap("q_final").view(bs, R, O.M, 128).cpu(), c, info


def _run(eng, sd, kind, c, objective=None, terms=False):
    """loss_backward (+ objective / terms) + loss_finalize under the profiler's launch record: (loss, grads, stats, flat, terms or None)."""
    eng.prof_enable(True)
    res = eng.loss_backward(kind, c, objective=objective, terms=terms)
    ran = eng.prof_report()
    eng.prof_enable(False)
    assert ran.get("loss_kernel", {}).get("count") == 1, sorted(ran)                      # exactly one objective launch
    assert ("loss_terms_kernel" in ran) == bool(terms), sorted(ran)
    stats, flat = res[0], res[1]
    grads = {k: torch.zeros_like(sd[O.PREFIX + k]).cuda() for k in losses.PI_KEYS}
    loss = float(eng.loss_finalize(stats, flat, grads).item())
    torch.cuda.synchronize()
    return loss, {k: g.cpu() for k, g in grads.items()}, stats.cpu(), flat.cpu(), (res[3].cpu() if terms else None)


def _errors(loss, grads, ref):
    """(|loss - ref|, worst gradient error in bars of its own tensor)."""
    return abs(loss - float(ref[0])), max(H.max_err(grads[k], ref[1][k]) / O.bar(ref[1][k]) for k in grads)


def _same_bits(a, b):
    return a[0] == b[0] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,mode", CASES)
def test_defaults_write_the_bits_of_the_compiled_in_entry(engines, name, mode, kind):
    """rift_loss_backward_ex with rift_objective_params_default(kind): stats, the 16 897 gradient sums and the finalized gradients are
    those of rift_loss_backward on the same forward, bit for bit, with and without `terms`; one objective launch each."""
    eng, sd, r_pad, qf, c, info = _forward(engines, name, mode, kind)
    old = _run(eng, sd, kind, c)
    assert old[3].numel() == 16897 and float(old[2][1]) == float(c["group_advantage_mask_torch"].sum()) > 0
    for terms in (False, True):
        new = _run(eng, sd, kind, c, objective={}, terms=terms)
        assert _same_bits(old, new), (terms, old[0], new[0])
    from rift_amd import _ffi
    explicit = _run(eng, sd, kind, c, objective=_ffi.objective_params(kind, **P.DEFAULTS[kind]))
    assert _same_bits(old, explicit)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,mode", CASES)
def test_every_setting_reaches_the_kernel(engines, name, mode, kind):
    """Each setting of objective_param_cases.SETTINGS and the combined case: loss and every gradient within the bars of the restatement at
    those settings, and farther than 10 bars from the restatement at the defaults."""
    eng, sd, r_pad, qf, c, info = _forward(engines, name, mode, kind)
    keep = c["group_advantage_mask_torch"].view(info["ratios"].shape).numpy()
    d = P.edge_distances(info["ratios"], keep)
    assert O.ratio_margin(info, info["ratios"])[0] < 1e-5 and all(d[e] >= m - 1e-5 for e, m in P.EDGES.items()), d
    base = P.reference(sd, qf, kind, c, r_pad, P.DEFAULTS[kind])
    for sname, (over, _, names) in P.SETTINGS[kind].items():
        if name not in names:
            continue
        s = P.settings(kind, sname)
        ref = P.reference(sd, qf, kind, c, r_pad, s)
        loss, grads, stats, _, _ = _run(eng, sd, kind, c, objective=over)
        lerr, gerr = _errors(loss, grads, ref)
        lfar, gfar = _errors(loss, grads, base)
        print(f"OBJEX {name} {kind} {mode} [{sname}]: loss {float(ref[0]):+.6f}, |loss - ref| {lerr:.2e}, gradients {gerr:.4f} bars; "
              f"from the defaults' reference: {lfar / O.LOSS_BAR:.0f} loss bars, {gfar:.0f} gradient bars")
        assert np.isfinite(loss) and lerr < O.LOSS_BAR, sname
        for k in grads:
            assert H.max_err(grads[k], ref[1][k]) < O.bar(ref[1][k]), (sname, k)
        assert lfar > 10 * O.LOSS_BAR and gfar > 10, sname
        assert float(stats[1]) == float(keep.sum())


@pytest.mark.parametrize("name,mode", CASES)
def test_kind_only_picks_the_defaults(engines, name, mode):
    """RIFT with kl_beta 0.2 and GRPO with dual_clip 3 on the same inputs are the same settings: the same bits.  GRPO with kl_beta 0 reads no
    reference logits: without them it gives the bits of the call that has them."""
    eng, sd, r_pad, qf, c, info = _forward(engines, name, mode, "rift")
    a = _run(eng, sd, "rift", c, objective={"kl_beta": 0.2}, terms=True)
    b = _run(eng, sd, "grpo", c, objective={"dual_clip": 3.0}, terms=True)
    assert _same_bits(a, b) and torch.equal(a[4], b[4])
    ref = P.reference(sd, qf, "rift", c, r_pad, dict(P.DEFAULTS["rift"], kl_beta=0.2))
    assert _errors(a[0], a[1], ref)[0] < O.LOSS_BAR and _errors(a[0], a[1], ref)[1] < 1.0
    bare = {k: v for k, v in c.items() if k != "ref_group_logits_torch"}
    with_ref = _run(eng, sd, "grpo", c, objective={"kl_beta": 0.0, "dual_clip": 3.0})
    without = _run(eng, sd, "grpo", bare, objective={"kl_beta": 0.0, "dual_clip": 3.0})
    rift_old = _run(eng, sd, "rift", bare)
    assert _same_bits(with_ref, without) and _same_bits(without, rift_old)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,mode", CASES)
def test_term_sums(engines, name, mode, kind):
    """`terms` at the defaults and at the combined settings: the counts are the restatement's (and follow from the placed classes), the three
    sums per valid candidate are within 1e-5 of it, stats[0] = terms[0] - kl_beta terms[1] + entropy_coef terms[2] to 1e-12 relative, two
    runs give the same bits, and asking for the terms changes nothing else."""
    eng, sd, r_pad, qf, c, info = _forward(engines, name, mode, kind)
    for sname, over in (("defaults", {}), ("combined", P.COMBINED)):
        s = dict(P.DEFAULTS[kind], **over)
        ref = P.reference(sd, qf, kind, c, r_pad, s)
        plain = _run(eng, sd, kind, c, objective=over)
        first = _run(eng, sd, kind, c, objective=over, terms=True)
        again = _run(eng, sd, kind, c, objective=over, terms=True)
        t, want = first[4], ref[2]
        assert _same_bits(plain, first) and _same_bits(first, again) and torch.equal(t, again[4])
        assert [float(v) for v in t[3:]] == [float(v) for v in want[3:]], (t.tolist(), want.tolist())
        assert (int(t[3]), int(t[4]), int(t[5])) == P.expected_counts(c, info, s) and float(t[5]) == float(first[2][1])
        n = float(t[5])
        err = [abs(float(t[k]) - float(want[k])) / n for k in range(3)]
        ident = abs(float(first[2][0]) - float(t[0] - s["kl_beta"] * t[1] + s["entropy_coef"] * t[2])) / abs(float(first[2][0]))
        print(f"TERMS {name} {kind} {mode} [{sname}]: counts {[int(v) for v in t[3:6]]}, |sum - ref| / count {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}, identity {ident:.1e}")
        assert max(err) < 1e-5 and ident < 1e-12
        assert (float(t[1]) != 0.0) == (s["kl_beta"] != 0.0) and (float(t[2]) != 0.0) == (s["entropy_coef"] != 0.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,mode", CASES)
def test_nothing_valid(engines, name, mode, kind):
    """The whole batch masked, every term switched on: loss exactly 0.0, count 0, every sum and every term exactly zero."""
    eng, sd, r_pad, qf, c, info = _forward(engines, name, mode, kind, variant=1)
    loss, grads, stats, flat, t = _run(eng, sd, kind, c, objective=P.COMBINED, terms=True)
    assert loss == 0.0 and float(stats[0]) == 0.0 and float(stats[1]) == 0.0
    assert not bool(flat.any()) and all(not bool(g.any()) for g in grads.values()) and not bool(t.any())


def test_refusals_launch_nothing(engines):
    """Every refusal of include/rift_hip.h: RIFT_ERR_ARG, a message in rift_last_error, no launch (the profiler's record stays empty) and
    the outputs as they were."""
    from rift_amd import _ffi
    eng, sd, r_pad, qf, c, info = _forward(engines, "one", "fp32", "rift")
    dev = eng.device
    keep = {k: c[k].to(dev) for k in ("old_group_logits_torch", "ref_group_logits_torch", "group_advantage_torch", "group_advantage_mask_torch")}
    keep["old_group_logits_torch"], keep["ref_group_logits_torch"] = keep["old_group_logits_torch"].float().contiguous(), keep["ref_group_logits_torch"].float().contiguous()

    def loss_in(ref=True):
        li = _ffi.RiftLossIn()
        li.old_group_logits, li.group_advantage = keep["old_group_logits_torch"].data_ptr(), keep["group_advantage_torch"].data_ptr()
        li.group_valid_mask = keep["group_advantage_mask_torch"].data_ptr()
        li.ref_group_logits = keep["ref_group_logits_torch"].data_ptr() if ref else None
        li.clip_epsilon, li.lambda_entropy = 0.2, 0.01
        return li

    stats = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    flat = torch.full((_ffi.PI_NPARAM,), -7.0, device=dev)
    terms = torch.full((8,), -7.0, dtype=torch.float64, device=dev)
    lo = _ffi.RiftLossOut()
    lo.stats, lo.flat_grad_sum = stats.data_ptr(), flat.data_ptr()
    nan, inf = float("nan"), float("inf")
    rift, grpo, ppo, reinforce, sft = (_ffi.LOSS_KINDS[k] for k in ("rift", "grpo", "ppo", "reinforce", "sft"))
    bad = [("params == NULL", rift, None, True, "NULL")]
    bad += [(f"kind {k}", k, {}, True, "kind") for k in (ppo, reinforce, sft, 7, -1)]
    bad += [(f"{f} = {v}", rift, {f: v}, True, "not finite") for f in P.KEYS for v in (nan, inf, -inf)]
    bad += [("clip_low = 0", rift, {"clip_low": 0.0}, True, "clip_low"), ("clip_low = -0.8", grpo, {"clip_low": -0.8}, True, "clip_low"),
            ("clip_low = 1.01", rift, {"clip_low": 1.01}, True, "clip_low"), ("clip_high = 0.99", rift, {"clip_high": 0.99}, True, "clip_high"),
            ("dual_clip = 1", rift, {"dual_clip": 1.0}, True, "dual_clip"), ("dual_clip = 0.5", grpo, {"dual_clip": 0.5}, True, "dual_clip"),
            ("dual_clip = -3", rift, {"dual_clip": -3.0}, True, "dual_clip"), ("kl_beta = -0.2", grpo, {"kl_beta": -0.2}, True, "kl_beta"),
            ("entropy_coef = -0.5", rift, {"entropy_coef": -0.5}, True, "entropy_coef"),
            ("kl_beta 0.2 without reference logits", rift, {"kl_beta": 0.2}, False, "ref_group_logits"),
            ("GRPO defaults without reference logits", grpo, {}, False, "ref_group_logits")]
    eng.prof_enable(True)
    for what, kind, over, has_ref, word in bad:
        p = None
        if over is not None:
            p = _ffi.RiftObjectiveParams()
            assert eng.lib.rift_objective_params_default(kind if kind in (rift, grpo) else rift, C.byref(p)) == 0
            for k, v in over.items():
                setattr(p, k, v)
        li = loss_in(has_ref)
        rc = eng.lib.rift_loss_backward_ex(eng.ctx, kind, C.byref(li), C.byref(p) if p is not None else None, C.byref(lo), terms.data_ptr(), None)
        msg = (eng.lib.rift_last_error(eng.ctx) or b"").decode()
        assert rc == -1 and "rift_loss_backward_ex" in msg and word in msg, (what, rc, msg)
    ran = eng.prof_report()
    eng.prof_enable(False)
    torch.cuda.synchronize()
    assert sum(int(v.get("count", 0)) for v in ran.values()) == 0, ran
    assert bool((stats == -7.0).all()) and bool((flat == -7.0).all()) and bool((terms == -7.0).all())
    # the binding turns a refusal into an exception that carries the library's reason
    with pytest.raises(RuntimeError, match=r"rift_loss_backward_ex failed \(-1\).*clip_high"):
        eng.loss_backward("rift", c, objective={"clip_high": 0.5})
    with pytest.raises(ValueError, match="terms"):
        eng.loss_backward("rift", c, terms=True)
    # ... and the edge values the refusals leave open are accepted: clip 1 / 1, the GRPO kind without KL and without reference logits
    ok = _run(eng, sd, "grpo", {k: v for k, v in c.items() if k != "ref_group_logits_torch"}, objective={"clip_low": 1.0, "clip_high": 1.0, "kl_beta": 0.0})
    ref = P.reference(sd, qf, "grpo", c, r_pad, dict(P.DEFAULTS["grpo"], clip_low=1.0, clip_high=1.0, kl_beta=0.0))
    assert _errors(ok[0], ok[1], ref)[0] < O.LOSS_BAR and _errors(ok[0], ok[1], ref)[1] < 1.0


def _combined_in_torch(prob, r_pad, c, dev, s):
    """The combined objective as a trainer would write it in PyTorch over the model's `probability` (fp32 on the device)."""
    bs = prob.shape[0]
    pad = r_pad.to(dev).unsqueeze(-1)
    lp = torch.log_softmax(prob.masked_fill(pad, -1e8).view(bs, -1), dim=1)
    lo = torch.log_softmax(c["old_group_logits_torch"].to(dev).masked_fill(pad, -1e8).view(bs, -1), dim=1)
    rp = torch.softmax(c["ref_group_logits_torch"].to(dev).masked_fill(pad, -1e8).view(bs, -1), dim=1)
    A = c["group_advantage_torch"].to(dev).view(bs, -1)
    ratio = (lp - lo).exp()
    obj = torch.min(A * ratio, A * ratio.clamp(s["clip_low"], s["clip_high"]))
    obj = torch.where(A < 0, torch.max(obj, A * s["dual_clip"]), obj)
    obj = obj - s["kl_beta"] * (torch.xlogy(rp, rp) - rp * lp) + s["entropy_coef"] * (-(lp.exp() * lp))
    return -obj[c["group_advantage_mask_torch"].to(dev).view(bs, -1)].mean()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_bridge_cross_check(precision, kind):
    """The combined objective written in PyTorch over `probability` of a differentiable_head model, loss.backward() through
    rift_head_backward: its gradients are within the bar of rift_loss_backward_ex + rift_loss_finalize on the same forward."""
    from rift_amd.planning.pluto.model.pluto_model import PlanningModel
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    sd = O.spread_weights(H.weights(), O.head_scale("std", kind))
    m = PlanningModel(radius=120, drop_path=0.0, dropout=0.0, state_dropout=0.0)
    m.load_state_dict(sd)
    m = m.to(dev)
    m.compute_precision, m.need_traj = precision, False
    m.train()
    for p in m.parameters():
        p.requires_grad_(False)
    head = dict(m.planning_decoder.pi_head.named_parameters())
    for p in head.values():
        p.requires_grad_(True)
    m.differentiable_head = True
    b = O.batch("std")
    r_pad = O.line_padding(b)
    prob = m(H.clone_tree(b["cur_pluto_feature_torch"]))["probability"]
    assert prob.grad_fn is not None
    c, info = P.build_case("std", kind, prob.detach().cpu(), r_pad)
    s = dict(P.DEFAULTS[kind], **P.COMBINED)
    loss_t = _combined_in_torch(prob, r_pad, c, dev, s)
    loss_t.backward()
    loss_t = float(loss_t.detach())
    eng = m.engine()
    stats, flat, _ = eng.loss_backward(kind, c, objective=P.COMBINED)
    grads = {k: torch.zeros_like(head[k]) for k in losses.PI_KEYS}
    loss = float(eng.loss_finalize(stats, flat, grads).item())
    torch.cuda.synchronize()
    worst = max(H.max_err(head[k].grad.cpu(), grads[k].cpu()) / O.bar(grads[k].cpu()) for k in grads)
    print(f"BRIDGE std {kind} {precision}: loss {loss:+.6f} (torch {loss_t:+.6f}), gradients within {worst:.4f} bars of the fixed-function route")
    assert abs(loss - loss_t) < O.LOSS_BAR
    for k in grads:
        assert float(grads[k].abs().max()) > 0 and H.max_err(head[k].grad.cpu(), grads[k].cpu()) < O.bar(grads[k].cpu()), k
    m.release_engine()


def _trainer_run(monkeypatch, env, objective, steps=3, validate=None):
    from rift_amd import synthetic as syn
    from rift_amd.planning.fine_tuner.rlft.trainer import RLFTTrainer
    from rift_amd.planning.pluto.model.pluto_model import PlanningModel
    from rift_amd.replay import DeviceReplay
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scenes = [syn.make_scene(4700 + i) for i in range(48)]
    g = torch.Generator().manual_seed(21)
    picks = [torch.randperm(48, generator=g)[:24].to(torch.int32).to(dev) for _ in range(steps)]
    torch.cuda.synchronize()
    replay = DeviceReplay(scenes, dev, rcap=6)
    model = PlanningModel(radius=120)
    model.load_state_dict({k: v.clone() for k, v in H.weights().items()})
    model = model.to(dev)
    model.need_traj = False
    model.train()
    tr = RLFTTrainer(model, kind="rift", seed=7, lr=1e-3, objective=objective)
    for ix in picks:
        fb, b = tr.gather(replay, ix)
        tr.training_step(fb, b)
    mean = tr.pop_mean_loss()
    out = {"mean": mean, "pipeline": bool(tr.pipeline),
           "terms": None if tr.last_terms is None else tr.last_terms.cpu().clone(),
           "pi": {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k.startswith(O.PREFIX)}}
    if validate is not None:
        out["validation"] = validate(tr, replay, model)
    torch.cuda.synchronize()
    tr.close()
    model.release_engine()
    return out


@pytest.mark.parametrize("path", ["pipelined", "serial"])
def test_trainer_takes_the_objective_on_every_path(monkeypatch, path):
    """Three steps of RLFTTrainer: objective=None and objective={} (the defaults through rift_loss_backward_ex) leave the same pi_head bit
    for bit, on the pipelined path (deferred tail on the update stream) and with RIFT_OVERLAP=0 RIFT_PIPELINE=0 (the serial step);
    {'dual_clip': 0} leaves another; the term sums are there when asked for."""
    env = {} if path == "pipelined" else {"RIFT_OVERLAP": "0", "RIFT_PIPELINE": "0"}
    none = _trainer_run(monkeypatch, env, None)
    same = _trainer_run(monkeypatch, env, {"terms": True})
    other = _trainer_run(monkeypatch, env, {"dual_clip": 0.0})
    assert none["pipeline"] == same["pipeline"] == (path == "pipelined")
    assert none["mean"] == same["mean"] and all(torch.equal(v, same["pi"][k]) for k, v in none["pi"].items())
    assert other["mean"] != none["mean"] and any(not torch.equal(v, other["pi"][k]) for k, v in none["pi"].items())
    assert none["terms"] is None and other["terms"] is None
    t = same["terms"]
    assert float(t[5]) > 0 and float(t[0]) != 0.0 and float(t[1]) == 0.0 and float(t[2]) == 0.0 and float(t[6]) == 0.0 and float(t[7]) == 0.0


def test_pipelined_validation_with_the_combined_objective(monkeypatch):
    """validation_step(out=...) on a gathered batch rides the step pipeline (head + objective on the update stream): its loss with the
    combined objective is within 1e-5 of the restatement on that forward's q_final and the parameters of the last update."""
    def validate(tr, replay, model):
        assert tr.pipelined_validation
        dev = tr.engine.device
        out = torch.zeros(1, dtype=torch.float64, device=dev)
        fb, b = tr.gather(replay, torch.arange(17, dtype=torch.int32, device=dev) + 5)
        tr.validation_step(fb, b, out=out)
        tr.wait_update()
        torch.cuda.synchronize()
        prob = tr._prob[:fb.bs].cpu()
        r_pad = prob[:, :, 0] == -1e6
        bs, R = r_pad.shape
        qf = tr.engine.tap("q_final").view(bs, R, O.M, 128).cpu()
        c = {"old_group_logits_torch": b["old_group_logits"].cpu(), "ref_group_logits_torch": b["ref_group_logits"].cpu(),
             "group_advantage_torch": b["group_advantage"].cpu(), "group_advantage_mask_torch": b["group_valid_mask"].cpu().bool()}
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith(O.PREFIX)}
        ref = P.reference(sd, qf, "rift", c, r_pad, dict(P.DEFAULTS["rift"], **P.COMBINED))
        base = P.reference(sd, qf, "rift", c, r_pad, P.DEFAULTS["rift"])
        return float(out.item()), float(ref[0]), float(base[0]), float(tr.last_terms[5].item()), float(c["group_advantage_mask_torch"].sum())

    run = _trainer_run(monkeypatch, {}, dict(P.COMBINED, terms=True), validate=validate)
    got, want, base, counted, valid = run["validation"]
    print(f"VALIDATION combined objective: loss {got:+.6f}, restatement {want:+.6f} (defaults {base:+.6f})")
    assert abs(got - want) < 1e-5 and abs(got - base) > 1e-4 and counted == valid > 0
