"""The settings of the group objective at run time (RiftObjectiveParams, rift_loss_backward_ex): the plain fp64 restatement with the five
settings as parameters, the settings the tests use and the counts that follow from the placed classes.  The inputs are those of
tests/objective_cases.py -- ratios placed on both sides of 0.7 / 0.8 / 1.2 / 1.26 / 1.3 / 2.5 / 3 / 4 for either sign of the advantage --
on which the changes that were mutants of the compiled-in kernel are settings this entry has to honour.  Shared by
tests/test_objective_param_cases.py (CPU: every setting is visible on the restatement alone) and tests/test_gpu_objective_params.py (the
kernel against the restatement).  Nothing here calls the library."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses
from oracle.pluto_ref import SD, mlp_layer
from tests import objective_cases as O

KEYS = ("clip_low", "clip_high", "dual_clip", "kl_beta", "entropy_coef")          # the order of RiftObjectiveParams
DEFAULTS = {"rift": dict(clip_low=0.8, clip_high=1.2, dual_clip=3.0, kl_beta=0.0, entropy_coef=0.0),
            "grpo": dict(clip_low=0.8, clip_high=1.2, dual_clip=0.0, kl_beta=0.2, entropy_coef=0.0)}
COMBINED = dict(clip_low=0.7, clip_high=1.3, dual_clip=2.0, kl_beta=0.05, entropy_coef=0.5)
# {kind: {name: (settings on top of the kind's defaults, least gradient shift in bars, batches)}}.  The entropy term is linear in its
# coefficient and moves the gradients by 12 - 65 bars at 0.2: the tests use 0.5 and ask for 25 bars.  The asymmetric range (0.8, 1.28) shows
# on the class (1.26, +1) alone, which the one-line scene of `one` does not hold.  dual_clip 3 on GRPO's classes would move nothing (no ratio
# above 1.5): 1.35 puts the class (1.5, -1) on the floor.
ALL, LARGER = ("one", "std", "dense", "wide"), ("std", "dense", "wide")
SETTINGS = {
    "rift": {"clip 0.7/1.3": (dict(clip_low=0.7, clip_high=1.3), 50, ALL), "clip 0.8/1.28": (dict(clip_high=1.28), 50, LARGER),
             "dual clip 2": (dict(dual_clip=2.0), 50, ALL), "no dual clip": (dict(dual_clip=0.0), 50, ALL),
             "KL 0.2": (dict(kl_beta=0.2), 50, ALL), "entropy 0.5": (dict(entropy_coef=0.5), 25, ALL), "combined": (COMBINED, 50, ALL)},
    "grpo": {"clip 0.7/1.3": (dict(clip_low=0.7, clip_high=1.3), 50, ALL), "clip 0.8/1.28": (dict(clip_high=1.28), 50, LARGER),
             "dual clip 1.35": (dict(dual_clip=1.35), 50, ALL), "KL 0.1": (dict(kl_beta=0.1), 50, ALL), "no KL": (dict(kl_beta=0.0), 50, ALL),
             "entropy 0.5": (dict(entropy_coef=0.5), 25, ALL), "combined": (COMBINED, 50, ALL)},
}
CASES = [(kind, sname, name) for kind in SETTINGS for sname, (_, _, names) in SETTINGS[kind].items() for name in names]
# Every edge a setting puts into the clamp, the pass condition or the floor.  The placement lands the ratios within 1e-5 of their targets
# (asserted), and fp32 moves a ratio of 4 by 1e-6; the guard classes 1.26 / 0.74 lie 0.02 from 1.28 and 0.04 from 1.3 / 0.7 by design, so
# the edges of objective_cases keep its margin and the added ones take 0.015: 1500 placement errors.
EDGES = {0.8: O.MARGIN, 1.2: O.MARGIN, 3.0: O.MARGIN, 2.0: O.MARGIN, 1.35: O.MARGIN, 0.7: 0.015, 1.28: 0.015, 1.3: 0.015}


def settings(kind, sname):
    """The five settings of (kind, setting name): the kind's defaults with the setting's on top."""
    return dict(DEFAULTS[kind], **SETTINGS[kind][sname][0])


def build_case(name, kind, probability, r_pad, variant=0):
    """objective_cases.build_case; RIFT cases also get reference logits (objective_cases.ref_logits_case), for kl_beta > 0."""
    c, info = O.build_case(name, kind, probability, r_pad, variant)
    if kind == "rift":
        c["ref_group_logits_torch"], info["underflow"] = O.ref_logits_case(dict(c, **info), probability)
    return c, info


def restated_ex(sd, q_final, kind, b, r_pad, clip=(0.8, 1.2), dual_clip=None, kl_beta=None, entropy_coef=0.0):
    """The objective family of rift_loss_backward_ex in plain fp64 with autograd: `kind` only picks the defaults of dual_clip / kl_beta
    (None).  At a kind's defaults the operations are those of objective_cases.restated, in its order.  Returns (loss, {parameter:
    gradient}, terms (8,) f64: the sums of include/rift_hip.h)."""
    dual_clip = DEFAULTS[kind]["dual_clip"] if dual_clip is None else dual_clip
    kl_beta = DEFAULTS[kind]["kl_beta"] if kl_beta is None else kl_beta
    params = {k: sd[O.PREFIX + k].double().clone().requires_grad_(True) for k in losses.PI_KEYS}
    pi = mlp_layer(q_final.double(), SD({O.PREFIX + k: v for k, v in params.items()}, O.PREFIX)).squeeze(-1)
    bs = pi.shape[0]
    fill = r_pad.unsqueeze(-1)
    lp = F.log_softmax(pi.masked_fill(fill, -1e6).masked_fill(fill, -1e8).view(bs, -1), dim=1)
    lo = F.log_softmax(b["old_group_logits_torch"].double().masked_fill(fill, -1e8).view(bs, -1), dim=1)
    A = b["group_advantage_torch"].double().view(bs, -1)
    ratio = (lp - lo).exp()
    u, c = A * ratio, A * ratio.clamp(clip[0], clip[1])
    obj = torch.min(u, c)
    passes = ((ratio >= clip[0]) & (ratio <= clip[1])) | (u < c)
    floored = torch.zeros_like(passes)
    if dual_clip != 0:
        floored = (A < 0) & (obj < A * dual_clip)
        obj = torch.where(A < 0, torch.max(obj, A * dual_clip), obj)
    sur = obj
    kl = ent = torch.zeros_like(obj)
    if kl_beta != 0:
        rp = F.softmax(b["ref_group_logits_torch"].double().masked_fill(fill, -1e8).view(bs, -1), dim=1)
        kl = torch.xlogy(rp, rp) - rp * lp
        obj = obj - kl_beta * kl
    if entropy_coef != 0:
        ent = -(lp.exp() * lp)
        obj = obj + entropy_coef * ent
    keep = b["group_advantage_mask_torch"].view(bs, -1)
    loss = -obj[keep].mean() if bool(keep.any()) else torch.zeros((), dtype=torch.float64)
    if loss.requires_grad:
        loss.backward()
    terms = torch.zeros(8, dtype=torch.float64)
    terms[0], terms[1], terms[2] = sur.detach()[keep].sum(), kl.detach()[keep].sum(), ent.detach()[keep].sum()
    terms[3], terms[4], terms[5] = float((~passes & ~floored)[keep].sum()), float(floored[keep].sum()), float(keep.sum())
    return loss.detach(), {k: (v.grad.detach().clone() if v.grad is not None else torch.zeros_like(v)) for k, v in params.items()}, terms


def reference(sd, q_final, kind, b, r_pad, s):
    """restated_ex at the settings dict `s` (KEYS)."""
    return restated_ex(sd, q_final, kind, b, r_pad, (s["clip_low"], s["clip_high"]), s["dual_clip"], s["kl_beta"], s["entropy_coef"])


def expected_counts(c, info, s):
    """(clamped without gradient, on the floor, valid) from the PLACED ratios and the advantages' signs alone: outside the clip range the
    clamped side of min(u, c) is the active one for A > 0 above it, for A < 0 below it, and for A = 0 (u = c = 0, no u < c) on either side;
    A < 0 above the range keeps u = A ratio, which lies under the floor A dual_clip when ratio > dual_clip."""
    t = info["target"]
    A = c["group_advantage_torch"].view(t.shape).numpy()
    keep = c["group_advantage_mask_torch"].view(t.shape).numpy()
    low, high = t < s["clip_low"], t > s["clip_high"]
    clamped = (high & (A > 0)) | (low & (A < 0)) | ((low | high) & (A == 0))
    floored = high & (A < 0) & (t > s["dual_clip"]) if s["dual_clip"] else np.zeros_like(keep)
    return int((clamped & keep).sum()), int((floored & keep).sum()), int(keep.sum())


def edge_distances(ratios, keep):
    """{edge: the smallest distance of a valid candidate's realised ratio from it}."""
    r = ratios[keep]
    return {e: (float(np.min(np.abs(r - e))) if r.size else np.inf) for e in EDGES}


def moved(ref, other):
    """(|loss shift|, the largest gradient shift of a tensor in bars of that tensor of `ref`)."""
    return abs(float(ref[0]) - float(other[0])), max(float((ref[1][k] - other[1][k]).abs().max()) / O.bar(ref[1][k]) for k in ref[1])
