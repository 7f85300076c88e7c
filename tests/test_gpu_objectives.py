"""loss_kernel<MAXPL> (rift_amd/csrc/loss.h) and the host code that fills its arguments, at designed inputs: every branch of the five
objectives, holes in the valid mask, an underflowing reference probability, ties of the argmax, PPO actions beyond the first plane, a scene
and a batch with nothing valid, in every lane plane of loss_kernel<2>, <4> and <16>.  The cases and the fp64 references are in
tests/objective_cases.py; tests/test_objective_cases.py checks on the CPU that each decision is visible on them.  Every test runs one eval
forward, builds the case from the DEVICE's own logits (so the ratios sit where they were placed whatever the operand format), and
compares loss_backward + loss_finalize with the oracle evaluated in fp64 on the device's q_final.  Bars (test_losses_and_pi_head_grads):
|loss - ref| < 1e-5, max |g - ref| < 1e-5 + 1e-4 max |ref| per tensor, indices bit-exact.  Needs a real MI355X: `pytest -m gpu`.

Measured on MI355X: MEASURED below; profiles/NOTES_r13.md has every case."""
import numpy as np
import pytest
import torch

from oracle import losses
from tests import helpers as H
from tests import objective_cases as O

pytestmark = pytest.mark.gpu

# forward(fp32=True) | the default 16-bit operand build | Engine(operands="fp16"): loss.h is compiled once per build namespace
MODES = {"one": ("fp32", "bf16", "fp16"), "std": ("fp32", "bf16", "fp16"), "dense": ("fp32", "bf16"), "wide": ("fp32",), "lead": ("fp32", "bf16")}
CASES = [(n, m) for n in O.BATCHES for m in MODES[n]]
TIE_CASES = CASES + [("lead", m) for m in MODES["lead"]]

MEASURED = """The per-kind summary of the table in profiles/NOTES_r13.md, which has every (batch, kind, mode): worst |loss - fp64 oracle| and
worst gradient error in bars of its own tensor (1e-5 + 1e-4 max |ref|), over every batch and mode of a kind; next to it the distance between the fp32 oracle and its fp64 evaluation on the CPU forward of the same batches:
  kind        loss error   (of 1e-5)   gradient error   oracle fp32 vs fp64: loss / gradients
  rift        4.2e-07      0.042       0.063 bars       4.2e-07 / 1.7e-06
  grpo        1.3e-06      0.128       0.67 bars        4.2e-07 / 5.5e-06
  ppo         3.4e-07      0.034       0.070 bars       6.0e-07 / 1.2e-06
  reinforce   3.7e-07      0.037       0.092 bars       2.2e-07 / 8.2e-07   (ties)
  sft         3.4e-07      0.034       0.113 bars       2.2e-07 / 8.2e-07   (ties)
Above a tenth of a bar: GRPO on `one` in every mode (loss 0.11 .. 0.13, gradients 0.23 .. 0.67 of the bar) -- its head factor of 32
(objective_cases.head_scale) amplifies the fp32 rounding of the logits together with the 0.5 % by which the twelve rows of q_final differ,
the price of a visible KL weight on a one-line scene; GRPO on `dense` in fp32 (gradients 0.12); SFT on `one` in the default build, 1.27e-6 on
mlp.3.weight against a bar of 1.13e-5 (with the tie weights only the last Linear has a gradient, so the bar is its absolute part).  Every
other case is below a tenth of both bars; the fully masked batches are exactly zero."""


@pytest.fixture(scope="module")
def engines():
    """get(mode, weights) -> (engine, state dict): one engine per operand build and state dict ("model" = H.weights() for PPO, "tie", or the
    factor of O.spread_weights for RIFT / GRPO), made on demand."""
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    made = {}

    def get(mode, weights):
        key = ("fp16" if mode == "fp16" else "bf16", weights)
        if key not in made:
            sd = H.weights() if weights == "model" else (O.tie_weights(H.weights()) if weights == "tie" else O.spread_weights(H.weights(), weights))
            eng = _ffi.Engine("cuda:0", operands=key[0])
            eng.load_state_dict({k: v.clone() for k, v in sd.items()})
            made[key] = (eng, sd)
        return made[key]

    yield get
    for eng, _ in made.values():
        eng.close()


def _forward(engines, name, mode, weights="model"):
    eng, sd = engines(mode, weights)
    b = O.batch(name)
    out = eng.forward(b["cur_pluto_feature_torch"], fp32=mode == "fp32")
    torch.cuda.synchronize()
    r_pad = O.line_padding(b)
    bs, R = r_pad.shape
    prob = out["probability"].cpu()
    assert prob.shape == (bs, R, O.M) and bool((prob[r_pad] == -1e6).all()) and bool(torch.isfinite(prob).all())
    return eng, sd, r_pad, prob, eng.tap("q_final").view(bs, R, O.M, 128).cpu()


def _loss(eng, sd, kind, c, prefill=0.0, **kw):
    """loss_backward + loss_finalize under the profiler's launch record: (loss, grads, chosen, stats, flat)."""
    eng.prof_enable(True)
    stats, flat, chosen = eng.loss_backward(kind, c, **kw)
    ran = eng.prof_report()
    eng.prof_enable(False)
    assert ran.get("loss_kernel", {}).get("count") == 1, sorted(ran)
    grads = {k: torch.full_like(sd[O.PREFIX + k], prefill).cuda() for k in losses.PI_KEYS}
    loss = float(eng.loss_finalize(stats, flat, grads).item())
    torch.cuda.synchronize()
    return loss, grads, chosen, stats.cpu(), flat.cpu()


def _compare(tag, loss, grads, ref):
    """Print, then assert, the two bars against ref = (loss, {parameter: gradient}, ...)."""
    lerr = abs(loss - float(ref[0]))
    gerr = {k: H.max_err(grads[k].cpu(), ref[1][k]) for k in grads}
    worst = max(gerr[k] / O.bar(ref[1][k]) for k in gerr)
    note = "  (above a tenth of a bar)" if lerr > 0.1 * O.LOSS_BAR or worst > 0.1 else ""
    print(f"OBJ {tag}: loss {float(ref[0]):+.6f}, |loss - ref| {lerr:.2e}, gradients {max(gerr.values()):.2e} = {worst:.4f} bars{note}")
    assert np.isfinite(loss) and lerr < O.LOSS_BAR
    for k in grads:
        assert gerr[k] < O.bar(ref[1][k]), k


@pytest.mark.parametrize("kind", ["rift", "grpo"])
@pytest.mark.parametrize("name,mode", CASES)
def test_group_objectives_on_placed_ratios(engines, name, mode, kind):
    eng, sd, r_pad, prob, qf = _forward(engines, name, mode, O.head_scale(name, kind))
    c, info = O.build_case(name, kind, prob, r_pad)
    off, margin = O.ratio_margin(info, O.realised_ratios(prob, r_pad, c["old_group_logits_torch"]))
    assert off < 1e-5 and margin >= O.MARGIN and all(O.FILLER_RANGE[0] <= s <= O.FILLER_RANGE[1] for s in info["filler"])
    loss, grads, _, stats, _ = _loss(eng, sd, kind, c)
    assert float(stats[1]) == float(c["group_advantage_mask_torch"].sum())
    _compare(f"{name} {kind} {mode}", loss, grads, O.objective_ref64(sd, qf, kind, c, r_pad))


@pytest.mark.parametrize("kind", ["rift", "grpo"])
@pytest.mark.parametrize("name,mode", CASES)
def test_group_objectives_with_nothing_valid(engines, name, mode, kind):
    """The whole batch masked: loss exactly 0.0, count 0, gradient sums exactly zero, and gradient tensors that held zeros still do."""
    eng, sd, r_pad, prob, qf = _forward(engines, name, mode, O.head_scale(name, kind))
    c, _ = O.build_case(name, kind, prob, r_pad, variant=1)
    loss, grads, _, stats, flat = _loss(eng, sd, kind, c)
    assert loss == 0.0 and float(stats[1]) == 0.0 and float(stats[0]) == 0.0
    assert not bool(flat.any()) and all(not bool(g.any()) for g in grads.values())


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name,mode", CASES)
def test_ppo_actions_in_every_plane(engines, name, mode, variant):
    eng, sd, r_pad, prob, qf = _forward(engines, name, mode)
    c, info = O.build_case(name, "ppo", prob, r_pad, variant)
    clip, ent = O.PPO_SETTINGS[variant]
    lp = torch.log_softmax(prob.double().masked_fill(r_pad.unsqueeze(-1), -1e8).view(prob.shape[0], -1), dim=1)
    ratio = (lp[torch.arange(prob.shape[0]), info["flat"]] - c["old_log_prob_torch"].double()).exp()
    assert float((ratio - info["ratio"]).abs().max()) < 1e-5
    loss, grads, _, _, _ = _loss(eng, sd, "ppo", c, clip_epsilon=clip, lambda_entropy=ent)
    _compare(f"{name} ppo{variant} {mode}", loss, grads, O.objective_ref64(sd, qf, "ppo", c, r_pad, clip, ent))


@pytest.mark.parametrize("kind", ["reinforce", "sft"])
@pytest.mark.parametrize("name,mode", TIE_CASES)
def test_tied_logits_take_the_first_valid_candidate(engines, name, mode, kind):
    """pi_head's last Linear at weight 0, bias 0.25: every valid logit is 0.25 exactly.  REINFORCE chooses (first valid line, 0) and its loss
    is mean(ret_b log(12 valid lines_b)); SFT keeps the first valid line with the teacher's mode.  `lead`: the leading 1 / 6 / 0 lines are
    invalid, the winners are the flat indices 12, 72 (second plane) and 0."""
    eng, sd, r_pad, prob, qf = _forward(engines, name, mode, "tie")
    assert bool((prob[~r_pad] == 0.25).all())
    c, info = O.build_case(name, kind, prob, r_pad)
    if kind == "sft":
        c["action_mode_torch"] = eng.sft_teacher_mode(c["trajectory_torch"], c["teacher_infos_torch"], O.TEACHER_FR).cpu()
        assert torch.equal(c["action_mode_torch"][:, 1], info["teacher_m"])
    loss, grads, chosen, _, _ = _loss(eng, sd, kind, c)
    chosen = chosen.cpu()
    want_m = torch.zeros_like(info["first"]) if kind == "reinforce" else info["teacher_m"]
    assert torch.equal(chosen[:, 0], info["first"] // O.M) and torch.equal(chosen[:, 1], want_m), chosen.tolist()
    if name == "lead":
        assert info["first"].tolist() == [12, 72, 0]
    if kind == "reinforce":
        assert abs(loss - info["closed_form"]) < O.LOSS_BAR
    _compare(f"{name} {kind} {mode}", loss, grads, O.objective_ref64(sd, qf, kind, c, r_pad))
