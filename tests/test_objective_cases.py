"""The input conditions of tests/test_gpu_objectives.py, checked on the references alone (no GPU), with logits from the CPU oracle's forward
on the same batches: every ratio sits on its chosen side of 0.8 / 1.2 / 3.0 with a margin, every class is live in every lane plane that
can hold it, every decision of loss_kernel is VISIBLE -- changing it moves the fp64 reference by more than 100 bars -- and the fp32 oracle
and its fp64 evaluation agree far inside the bar.  These are conditions on the case design: a case that fails one is redesigned."""
import numpy as np
import pytest
import torch

from oracle import losses, pluto_ref
from tests import helpers as H
from tests import objective_cases as O

NAMES = tuple(O.BATCHES)


@pytest.fixture(scope="module")
def forwards():
    """{(batch, weights): (r_pad, logits, q_final, state dict)} from oracle.pluto_ref.planning_model_forward, computed once; weights: "model" =
    H.weights() (PPO), "tie", or the factor of O.spread_weights (RIFT, GRPO)."""
    out = {}
    for name in NAMES + ("lead",):
        for w in ("model", "tie") + tuple(sorted({O.head_scale(name, kind) for kind in ("rift", "grpo")})):
            if name == "lead" and w != "tie":
                continue
            sd = H.weights() if w == "model" else (O.tie_weights(H.weights()) if w == "tie" else O.spread_weights(H.weights(), w))
            b = O.batch(name)
            ref, _, taps = pluto_ref.planning_model_forward(sd, b["cur_pluto_feature_torch"], need_traj=False, want_taps=True)
            out[name, w] = (O.line_padding(b), ref["probability"], taps["q_final"], sd)
    return out


def _moved(ref, mut):
    """(|loss shift|, the largest gradient shift of a tensor in bars of that tensor)."""
    return abs(float(ref[0]) - float(mut[0])), max(float((ref[1][k] - mut[1][k]).abs().max()) / O.bar(ref[1][k]) for k in ref[1])


def _agree(a, b):
    return abs(float(a[0]) - float(b[0])), max(float((a[1][k].double() - b[1][k].double()).abs().max()) for k in a[1])


def test_batches_have_the_shapes_the_kernel_dispatches_on(forwards):
    want = {"one": (1, 12, 2), "std": (5, 72, 2), "dense": (3, 192, 4), "wide": (2, 264, 16)}
    for name in NAMES:
        r_pad, prob, _, _ = forwards[name, "model"]
        bs, R, M = prob.shape
        maxpl = 2 if R * M <= 128 else (4 if R * M <= 256 else 16)              # shared.hip rift_loss_backward
        assert (bs, R * M, maxpl) == want[name]
        assert tuple((~r_pad).sum(1).tolist()) == O.BATCHES[name]
        assert bool((prob[r_pad] == -1e6).all()) and bool(torch.isfinite(prob).all())
    r_pad = forwards["lead", "tie"][0]
    assert r_pad.shape == (3, 7) and [int(v) for v in (~r_pad).float().argmax(1)] == [1, 6, 0]


@pytest.mark.parametrize("kind", ["rift", "grpo"])
@pytest.mark.parametrize("name", NAMES)
def test_ratios_sit_where_they_were_placed(forwards, name, kind):
    r_pad, prob, _, _ = forwards[name, O.head_scale(name, kind)]
    c, info = O.build_case(name, kind, prob, r_pad)
    classes = O.CLASSES[kind]
    ratios = O.realised_ratios(prob, r_pad, c["old_group_logits_torch"])
    off, margin = O.ratio_margin(info, ratios)
    print(f"{name} {kind}: fillers {np.round(info['filler'], 3).tolist()}, |realised - target| {off:.2e}, margin {margin:.3f}")
    assert off < 1e-5 and margin >= O.MARGIN
    assert all(O.FILLER_RANGE[0] <= s <= O.FILLER_RANGE[1] for s in info["filler"])
    # advantages: fp64, 0.4 .. 1.0, the sign of the class; exactly 0.0 on the zero class
    A = c["group_advantage_torch"].view(ratios.shape).numpy()
    assert c["group_advantage_torch"].dtype == torch.float64
    for k, (_, sign) in enumerate(classes):
        a = A[info["cls"] == k]
        assert (a.size or name == "one") and (np.all(a == 0.0) if sign == 0 else np.all((np.sign(a) == sign) & (np.abs(a) >= 0.4) & (np.abs(a) <= 1.0)))
    # the mask: never True on a padded line; holes inside valid lines
    mask = c["group_advantage_mask_torch"].view(ratios.shape).numpy()
    live = (~r_pad).repeat_interleave(O.M, dim=1).numpy()
    assert not mask[~live].any() and int((live & ~mask).sum()) >= 2
    if name in O.LINE_HOLES:
        s, ln = O.LINE_HOLES[name]
        assert live[s, ln * O.M] and not mask[s, ln * O.M:(ln + 1) * O.M].any()
    if name in O.SCENE_HOLES:
        assert not mask[O.SCENE_HOLES[name]].any() and live[O.SCENE_HOLES[name]].any()
    # every class live in every plane that has room for the classes; a scarcer plane holds as many distinct classes as it has candidates, in
    # priority order; the single 12-candidate scene of `one` holds its balanced subset (O.SMALL_DEALS, the module's docstring has the algebra)
    present, room = O.classes_by_plane(dict(c, **info), classes), O.plane_capacity(r_pad)
    for q, n in room.items():
        if name == "one":
            assert present[q] == set(O.SMALL_DEALS[kind][0])
        elif n >= len(classes):
            assert present[q] == set(classes), (q, set(classes) - present[q])
        else:
            assert present[q] == set(classes[:n]), (q, present[q])
    if kind == "grpo":
        rp32 = torch.softmax(c["ref_group_logits_torch"].masked_fill(r_pad.unsqueeze(-1), -1e8).view(ratios.shape[0], -1), dim=1)
        rp64 = torch.softmax(c["ref_group_logits_torch"].double().masked_fill(r_pad.unsqueeze(-1), -1e8).view(ratios.shape[0], -1), dim=1)
        for b, j in enumerate(info["underflow"]):
            assert float(rp32[b, j]) == 0.0 and 0.0 < float(rp64[b, j]) < 1e-80 and (mask[b, j] or not mask[b].any())
            assert int((rp32[b][torch.from_numpy(live[b])] == 0).sum()) == 1


def test_small_deals_cover_the_classes_between_them():
    for kind, classes in O.CLASSES.items():
        a, b = O.SMALL_DEALS[kind]
        assert set(a) | set(b) == set(classes)
        for deal in (a, b):
            assert abs(sum(1.0 / t - 1.0 for t, _ in deal)) <= 0.5


@pytest.mark.parametrize("kind", ["rift", "grpo"])
@pytest.mark.parametrize("name", NAMES)
def test_group_objective_decisions_are_visible(forwards, name, kind):
    """The fp32 oracle, its fp64 evaluation and the restatement agree, and every mutant moves the fp64 loss by 100 loss bars and at least
    one gradient tensor by 100 of that tensor's bars -- on every batch."""
    r_pad, prob, qf, sd = forwards[name, O.head_scale(name, kind)]
    c, info = O.build_case(name, kind, prob, r_pad)
    r64 = O.objective_ref64(sd, qf, kind, c, r_pad)
    r32 = O.objective_ref32(sd, qf, kind, c, r_pad)
    dl, dg = _agree(r32, r64)
    rl, rg = _agree(O.restated(sd, qf, kind, c, r_pad), r64)
    print(f"{name} {kind}: loss {float(r64[0]):+.6f}; fp32 oracle vs fp64: loss {dl:.2e}, gradients {dg:.2e}; restatement vs fp64 oracle {rl:.1e} / {rg:.1e}")
    assert dl < 1e-6 and rl < 1e-12 and rg < 1e-12
    for mname, fn in O.mutants(kind).items():
        ml, mg = _moved(r64, fn(sd, qf, b=c, r_pad=r_pad))
        print(f"    {mname}: loss moves by {ml:.3e}, gradients by {mg:.0f} bars")
        assert ml >= 100 * O.LOSS_BAR and mg >= 100, mname


@pytest.mark.parametrize("kind", ["rift", "grpo"])
@pytest.mark.parametrize("name", NAMES)
def test_fully_masked_batch_is_zero_in_the_oracle(forwards, name, kind):
    r_pad, prob, qf, sd = forwards[name, O.head_scale(name, kind)]
    c, _ = O.build_case(name, kind, prob, r_pad, variant=1)
    assert not bool(c["group_advantage_mask_torch"].any())
    for ref in (O.objective_ref32, O.objective_ref64, O.restated):
        loss, grads, _ = ref(sd, qf, kind, c, r_pad)
        assert float(loss) == 0.0 and all(not bool(g.any()) for g in grads.values())


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_ppo_actions_reach_beyond_the_first_line_and_plane(forwards, name, variant):
    r_pad, prob, qf, sd = forwards[name, "model"]
    c, info = O.build_case(name, "ppo", prob, r_pad, variant)
    clip, ent = O.PPO_SETTINGS[variant]
    bs = prob.shape[0]
    lp = torch.log_softmax(prob.double().masked_fill(r_pad.unsqueeze(-1), -1e8).view(bs, -1), dim=1)
    ratio = (lp[torch.arange(bs), info["flat"]] - c["old_log_prob_torch"].double()).exp()
    assert float((ratio - info["ratio"]).abs().max()) < 1e-5
    for edge in (0.6, 0.8, 1.2, 1.4):
        assert float((ratio - edge).abs().min()) > 0.09
    assert not bool(r_pad[torch.arange(bs), c["action_mode_torch"][:, 0]].any())
    r64 = O.objective_ref64(sd, qf, "ppo", c, r_pad, clip, ent)
    dl, dg = _agree(O.objective_ref32(sd, qf, "ppo", c, r_pad, clip, ent), r64)
    rl, rg = _agree(O.restated(sd, qf, "ppo", c, r_pad, clip, ent), r64)
    print(f"{name} ppo {variant}: chosen {info['flat'].tolist()}, ratios {info['ratio'].tolist()}; fp32 oracle vs fp64 {dl:.2e} / {dg:.2e}")
    assert dl < 1e-6 and rl < 1e-12 and rg < 1e-12
    if int(info["flat"].max()) >= 64:
        ml, mg = _moved(r64, O.mutants("ppo")["chosen index modulo 64"](sd, qf, b=c, r_pad=r_pad, clip_epsilon=clip, lambda_entropy=ent))
        print(f"    chosen index modulo 64: loss moves by {ml:.3e}, gradients by {mg:.0f} bars")
        assert ml >= 1e-3 and mg >= 100


def test_ppo_places_cover_the_indices_the_issue_names():
    for name in ("std", "dense"):
        r_pad = O.line_padding(O.batch(name))
        last = set(((~r_pad).sum(1) * O.M - 1).tolist())
        flat = set()
        for variant in (0, 1):
            places = O.PPO_PLACES[name][variant]
            flat |= {int((~r_pad[b]).sum()) * O.M - 1 if j == "last" else j for b, j in enumerate(places)}
        assert {0, 63, 64} <= flat and flat & last
    # wide: the last candidate of the 22-line scene, 263, lies in the fifth plane (loss_kernel<16>)
    assert O.PPO_PLACES["wide"][0][0] == "last" and O.PPO_PLACES["wide"][1][0] == 64
    r_pad = O.line_padding(O.batch("wide"))
    assert int((~r_pad[0]).sum()) * O.M - 1 == 263


@pytest.mark.parametrize("kind", ["reinforce", "sft"])
@pytest.mark.parametrize("name", NAMES + ("lead",))
def test_tied_logits_choose_the_first_valid_candidate(forwards, name, kind):
    """Every valid logit is 0.25: (r, m) = (first valid line, 0) for REINFORCE and the loss is mean(ret_b log(12 valid lines_b)); SFT keeps
    the first valid line with the teacher's mode.  The last-index rule gives the same loss (every log-probability of a scene is equal) --
    it shows in the indices and in the gradient, which is what the GPU test compares."""
    r_pad, prob, qf, sd = forwards[name, "tie"]
    assert bool((prob[~r_pad] == 0.25).all())
    c, info = O.build_case(name, kind, prob, r_pad)
    r64 = O.objective_ref64(sd, qf, kind, c, r_pad)
    dl, dg = _agree(O.objective_ref32(sd, qf, kind, c, r_pad), r64)
    loss, grads, (r, m) = O.restated(sd, qf, kind, c, r_pad)
    rl, rg = _agree((loss, grads), r64)
    assert dl < 1e-6 and rl < 1e-12 and rg < 1e-12
    first = info["first"]
    if kind == "reinforce":
        _, ro, mo = losses.reinforce_loss(prob, r_pad, c["return_torch"])
        assert torch.equal(ro, first // O.M) and not bool(mo.any()) and torch.equal(r, ro) and torch.equal(m, mo)
        assert abs(float(loss) - info["closed_form"]) < 1e-12
    else:
        _, ro, mo = losses.sft_loss(prob, r_pad, c["trajectory_torch"], c["teacher_infos_torch"])
        assert torch.equal(ro, first // O.M) and torch.equal(mo, info["teacher_m"]) and torch.equal(r, ro) and torch.equal(m, mo)
        assert len(set(mo.tolist())) == len(mo) or len(mo) > 12
    if name == "lead":
        assert first.tolist() == [12, 72, 0]
    mut = O.mutants(kind)["last-index tie rule"](sd, qf, b=c, r_pad=r_pad)
    ml, mg = _moved(r64, mut)
    rows = (~r_pad).sum(1) > 1 if kind == "sft" else torch.ones(len(first), dtype=torch.bool)
    assert bool((mut[2][0][rows] != r[rows]).all()) if kind == "sft" else bool(((mut[2][0] * O.M + mut[2][1]) == info["last"]).all())
    print(f"{name} {kind} ties: fp32 oracle vs fp64 {dl:.2e} / {dg:.2e}; last-index rule moves the loss by {ml:.1e} and the gradients by {mg:.0f} bars")
    if bool(rows.any()):
        assert mg >= 100
