"""Designed inputs and plain fp64 restatements for the objective kernel (loss_kernel<MAXPL>, rift_amd/csrc/loss.h): RIFT dual clip, GRPO,
PPO actor, REINFORCE and SFT at inputs where every data-dependent decision of the kernel is taken on purpose -- the side of min(u, c) for
either sign of the advantage, the dual-clip floor, the rp > 0 guard of the KL term, holes in the valid mask inside valid lines, a scene
with nothing valid, the first-index tie rule of the argmax across lanes and lane planes, a PPO action beyond the first plane -- and in
every lane plane the group has (one wave per scene, candidate j lives in lane j % 64 of plane j // 64).  Shared by
tests/test_objective_cases.py (CPU: the conditions the inputs must satisfy, on the references alone) and tests/test_gpu_objectives.py (the
kernel against the references).  Nothing here calls the library.

The classes.  A design candidate j of a scene gets a target ratio t_j: old_logit_j = logit_j - log t_j.  The old policy's softmax then
is q_j = (p_j / t_j) / Z with Z = sum_j p_j / t_j, and the realised ratio p_j / q_j = t_j Z.  Every other valid candidate of the scene
(the fillers, which hold most of the probability) takes the one ratio s = P_filler / (1 - sum_design p_j / t_j) that makes Z = 1, so the
design ratios land on the grid exactly.  s must lie in [0.85, 1.15]: inside the clip range with the same 0.05 margin as the design ratios.

How many design candidates a scene can hold follows from that bound.  With e_j = 1 / t_j - 1 the condition reads
sum_design p_j e_j = -P_filler (1 / s - 1); e is +1 at t = 0.5 and -0.75 at t = 4, so a scene of 12 candidates that held the eleven RIFT
classes of the plan would leave one filler of p ~ 1/12 to absorb sum e ~ -0.2 .. -0.5: s ~ 0.75 .. 0.85.  Therefore
  * a plane of a scene with at least three candidates per class holds every class twice, on its candidates of smallest p, a plane with
    more candidates than classes every class once;
  * a trailing plane with fewer candidates than classes (the 8 candidates of line 5 beyond lane 63, ...) is all design, the classes dealt
    in priority order and continued from scene to scene of the batch, the fillers of that scene being in its other planes;
  * a scene of one line (12 candidates) holds one of two balanced subsets of the classes (SMALL_DEALS: sum e within +-0.5), six or seven
    design candidates and five or six fillers.
The same bound limits the mask holes.  "One member of every class masked" needs a second, live member of the class in the scene, which
only the planes that hold every class twice have: there the second member of every class is a hole.  The other scenes (`one`, the
one-line scenes of `std` and `wide`, for RIFT's fourteen classes also the three-line scene of `std`) mask two fillers instead and no design candidate; the masked line of
std / dense / wide and the masked scene of std take design candidates and fillers alike."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses
from oracle.pluto_ref import SD, mlp_layer
from rift_amd import synthetic as syn
from tests import small_kernel_cases as K

M = 12
PREFIX = "planning_decoder.pi_head."
SEED0 = 9100
# valid reference lines per scene.  one: bs 1, G 12, a single plane with 52 idle lanes.  std: bs 5 -- the second 4-wave workgroup holds one live
# wave -- G 72 (loss_kernel<2>), line 5 straddles lanes 63 / 64.  dense: G 192, loss_kernel<4>, three planes.  wide: G 264, loss_kernel<16>.
BATCHES = {"one": (1,), "std": (1, 5, 6, 6, 3), "dense": (11, 9, 16), "wide": (22, 1)}
# ties only: R = 7, the leading 1 / 6 / 0 lines of the three scenes invalid: the first valid candidate is 12, 72 (second plane), 0
LEAD_LINES, LEAD_CLEARED = (7, 7, 4), (1, 6, 0)
EDGES = (0.8, 1.2, 3.0)
MARGIN = 0.05
FILLER_RANGE = (0.85, 1.15)

# (target ratio, sign of A) in priority order: the decisions a scarce plane must hold come first
# The last three are guards.  With 0.5 / 1.5 alone a clip range of 0.7 / 1.3 changes the loss but no gradient (the clamped side is constant
# under either range, and the kernel spells the range twice: in the clamp and in the gradient's pass condition): 1.26 with A > 0 and 0.74
# with A < 0 are clamped, gradient-free, under 0.8 / 1.2 and pass a gradient under 0.7 / 1.3.  Likewise 4.0 with A < 0 sits on the floor
# whether it is 3 A or 2 A: 2.5 with A < 0 is above 3 A (gradient) and below 2 A (none).
RIFT_CLASSES = ((4.0, -1), (1.5, +1), (0.5, -1), (0.5, +1), (1.5, -1), (4.0, +1), (0.9, 0), (0.9, +1), (1.1, -1), (0.9, -1), (1.1, +1),
                (1.26, +1), (0.74, -1), (2.5, -1))
# GRPO: no ratio above 1.5 (a ratio of 4 carries a gradient of 4 A there, next to which the KL term's does not show: the row "r > 3, GRPO"
# of DESIGN.md's branch table is not covered)
GRPO_CLASSES = tuple((1.5, 0) if c == (0.9, 0) else c for c in RIFT_CLASSES if c[0] not in (4.0, 2.5))
CLASSES = {"rift": RIFT_CLASSES, "grpo": GRPO_CLASSES}
# one-line scenes: balanced subsets (sum of 1 / t - 1: rift -0.07 / -0.40, grpo +0.27 / +0.25); `one` takes the first, the one-line
# scene of a larger batch the second
SMALL_DEALS = {
    "rift": (((0.5, +1), (4.0, -1), (1.1, -1), (0.9, 0), (0.74, -1), (2.5, -1), (1.1, +1)),
             ((0.5, -1), (4.0, +1), (1.5, -1), (0.9, +1), (0.9, -1), (1.26, +1), (1.5, +1))),
    "grpo": (((0.5, +1), (1.5, +1), (1.5, -1), (1.1, -1), (1.5, 0), (0.74, -1)),
             ((0.5, -1), (0.9, +1), (0.9, -1), (1.1, +1), (1.5, +1), (1.5, -1), (1.26, +1))),
}
# (batch: (scene, line)) one whole valid line masked; std's scene 1 is masked entirely
LINE_HOLES = {"std": (2, 3), "dense": (1, 4), "wide": (0, 7)}
SCENE_HOLES = {"std": 1}


# ---- batches -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch(name):
    if name == "lead":
        b = syn.collate_scenes([syn.make_scene(SEED0 + 50 + i, num_agents=12, num_polygons=8, r_min=r, r_max=r) for i, r in enumerate(LEAD_LINES)])
        for s, n in enumerate(LEAD_CLEARED):
            b["cur_pluto_feature_torch"]["reference_line"]["valid_mask"][s, :n] = False
        return b
    return syn.collate_scenes([syn.make_scene(SEED0 + i, num_agents=12, num_polygons=8, r_min=r, r_max=r) for i, r in enumerate(BATCHES[name])])


def batch(name):
    """A fresh copy of the collated batch `name` (BATCHES, or "lead")."""
    from tests import helpers as H
    return H.clone_tree(_batch(name))


def line_padding(b):
    """(bs, R) bool, True on a reference line without a valid point (pluto_model.py:143)."""
    return ~b["cur_pluto_feature_torch"]["reference_line"]["valid_mask"].any(-1)


def tie_weights(sd):
    """The state dict with pi_head's last Linear at weight 0, bias 0.25: every valid candidate's logit is 0.25 exactly, in any arithmetic."""
    sd = {k: v.clone() for k, v in sd.items()}
    sd[PREFIX + "mlp.3.weight"] = torch.zeros_like(sd[PREFIX + "mlp.3.weight"])
    sd[PREFIX + "mlp.3.bias"] = torch.full_like(sd[PREFIX + "mlp.3.bias"], 0.25)
    return sd


HEAD_SCALE = {"rift": 12.0, "grpo": 20.0}


def head_scale(name, kind):
    """The factor on pi_head's last Linear for the RIFT / GRPO cases of batch `name`.  With the fixture weights the candidates of a scene differ
    by 0.005 .. 0.4 in their logits and the gradients of a mean over up to 250 candidates are of the order of 1e-2: the absolute part of
    the gradient bar (1e-5) then hides every decision that moves a few per cent of the gradient.  12 spreads the logits of a scene by 3 .. 5
    and scales the gradients of the layers below with it; GRPO takes 20 for its KL weight, and 32 on `one`, whose single one-line scene
    spreads its logits by 0.005 (0.06 at 12): there the 12 rows of q_final differ by 0.5 % of their norm, which no head can change.
    More is not available.  The logits grow with the factor and their fp32 rounding with them, so both the distance between the fp32
    oracle and its fp64 evaluation (RIFT on `one`, with its ratios of 4: 6e-7 at 12, 3e-6 at 50, against the 1e-6 asked of it) and the
    device's distance from the fp64 reference grow in step with the visibility of the KL weight: on `one` 100 bars of visibility cost
    about 0.6 of the gradient bar in fp32 mode (measured: 169 bars against 0.995 at a factor of 50)."""
    return 32.0 if (name, kind) == ("one", "grpo") else HEAD_SCALE[kind]


def spread_weights(sd, k):
    """The state dict with pi_head's last Linear weight multiplied by k."""
    sd = {n: v.clone() for n, v in sd.items()}
    sd[PREFIX + "mlp.3.weight"] = sd[PREFIX + "mlp.3.weight"] * k
    return sd


def plane_count(G):
    return -(-G // 64)


# ---- ratio placement (RIFT, GRPO) ----------------------------------------------------------------------------------------------------------
def _filler_ratio(p, idx, t):
    """s for the design candidates idx with targets t; None when the design alone exceeds the old policy's mass."""
    den = 1.0 - float(np.sum(p[idx] / t))
    mask = np.ones(p.shape[0], dtype=bool)
    mask[idx] = False
    return float(p[mask].sum()) / den if den > 0 else None


def _plane_slots(p, v, G, classes, deal_small, next_cls, scene):
    """Which candidates of a scene are design candidates and which classes they take, plane by plane (the rules of the module docstring):
    [(candidate indices in ascending p, class indices to deal among them, whether the plane's second members are mask holes)]."""
    ncls = len(classes)
    planes = [v[v // 64 == q] for q in range(plane_count(G)) if (v // 64 == q).any()]
    doubled = [q for q, c in enumerate(planes) if c.size >= 3 * ncls]
    slots = []
    for q, c in enumerate(planes):
        order = c[np.argsort(p[c], kind="stable")]
        if c.size >= 3 * ncls:                                       # every class twice; one doubled plane of the scene carries the holes
            slots.append((order[:2 * ncls], list(range(ncls)) * 2, q == doubled[scene % len(doubled)]))
        elif c.size == M and len(planes) == 1:                       # a one-line scene: a balanced subset
            slots.append((order[:len(deal_small)], [classes.index(d) for d in deal_small], False))
        elif c.size > ncls:                                          # every class once
            slots.append((order[:ncls], list(range(ncls)), False))
        else:                                                        # a short trailing plane: all design, the priority list continued
            assert len(planes) > 1, "a small plane on its own: the deals are written down for 12 candidates"
            k0 = next_cls.get(int(c[0]) // 64, 0)
            slots.append((order, [(k0 + i) % ncls for i in range(c.size)], False))
            next_cls[int(c[0]) // 64] = (k0 + c.size) % ncls
    return slots


def _deal(p, slots, classes, rng):
    """Assign the classes of every slot to its candidates so that the filler ratio lands in [0.9, 1.1]: the identity deal first, then up to 63
    seeded permutations, the best one kept.  Returns (filler ratio, design indices, their class indices, which of them are mask holes)."""
    best = None
    for attempt in range(64):
        idx, kk, hole = [], [], []
        for cand, ks, holed in slots:
            perm = rng.permutation(len(ks)) if attempt else np.arange(len(ks))
            idx += list(cand[perm])
            kk += ks
            hole += [holed and i >= len(ks) // 2 for i in range(len(ks))]          # the second member of every class
        idx, kk = np.asarray(idx), np.asarray(kk)
        s = _filler_ratio(p, idx, np.array([classes[k][0] for k in kk]))
        if s is not None and (best is None or abs(s - 1) < abs(best[0] - 1)):
            best = (s, idx, kk, np.asarray(hole))
        if best is not None and abs(best[0] - 1) <= 0.10:
            break
    return best


def place_ratios(probability, r_pad, classes, name="", seed=515, masked=False):
    """The RIFT / GRPO inputs for the policy's own logits `probability` (bs, R, M), see the module docstring.  Returns the batch entries
    old_group_logits_torch (fp32), group_advantage_torch (fp64, |A| in [0.4, 1.0], sign by class, 0.0 for the zero class),
    group_advantage_mask_torch and the bookkeeping: cls (bs, G) = index into `classes` (-1 filler, -2 padded line), target (bs, G) ratio,
    filler (bs,) = s.  `name` selects the line / scene holes; masked: the variant with nothing valid in the whole batch."""
    bs, R, _ = probability.shape
    G = R * M
    rng = np.random.default_rng(seed + 7 * len(classes) + sum(ord(c) for c in name))
    logit = probability.detach().double().view(bs, G).numpy()
    live = (~r_pad).repeat_interleave(M, dim=1).numpy()
    small = SMALL_DEALS["rift" if classes is RIFT_CLASSES else "grpo"]
    cls = np.full((bs, G), -2, dtype=np.int64)
    target = np.ones((bs, G))
    filler = np.ones(bs)
    mask = live.copy()
    old = rng.standard_normal((bs, G))                               # (padded lines keep a draw: both sides mask them)
    adv = rng.standard_normal((bs, G))
    next_cls = {}                                                    # per plane: where the priority list continues in the next scene
    for b in range(bs):
        v = np.nonzero(live[b])[0]
        if v.size == 0:
            continue
        z = logit[b, v] - logit[b, v].max()
        p = np.zeros(G)
        p[v] = np.exp(z) / np.exp(z).sum()
        # ---- the deal: `one` takes the first balanced subset, the one-line scene of a larger batch the second
        s, idx, kk, hole = _deal(p, _plane_slots(p, v, G, classes, small[bs > 1], next_cls, b), classes, rng)
        assert FILLER_RANGE[0] <= s <= FILLER_RANGE[1], (name, b, s)
        # ---- the placement: old logits, advantages, holes
        cls[b, v], filler[b] = -1, s
        cls[b, idx] = kk
        target[b, v] = s
        target[b, idx] = [classes[k][0] for k in kk]
        old[b, v] = logit[b, v] - np.log(target[b, v])
        sign = np.where(rng.random(G) < 0.5, -1.0, 1.0)
        sign[idx] = [classes[k][1] for k in kk]
        adv[b] = rng.uniform(0.4, 1.0, G) * sign
        mask[b, idx[hole]] = False
        if not hole.any():                                           # a scene without a doubled class: two fillers are the holes
            mask[b, v[cls[b, v] == -1][:2]] = False
    if name in LINE_HOLES:
        s_, ln = LINE_HOLES[name]
        assert live[s_, ln * M]
        mask[s_, ln * M:(ln + 1) * M] = False
    # the fillers among the holes carry A > 0 (objective ~ +0.7 each against a batch mean near 0): a kernel that counted them moves the loss
    lost = live & ~mask & (cls == -1)
    adv[lost] = np.abs(adv[lost])
    if name in SCENE_HOLES:
        mask[SCENE_HOLES[name]] = False
    if masked:
        mask[:] = False
    return {"old_group_logits_torch": torch.from_numpy(old).float().view(bs, R, M), "group_advantage_torch": torch.from_numpy(adv).view(bs, R, M),
            "group_advantage_mask_torch": torch.from_numpy(mask).view(bs, R, M), "old_group_logits_mask_torch": torch.from_numpy(live).view(bs, R, M),
            "cls": cls, "target": target, "filler": filler}


PEAK = 8.0


def ref_logits_case(case, probability, seed=616):
    """GRPO's frozen-policy logits: 2 randn, with two placed candidates per scene.  One live filler lies 200 below the row's maximum: its
    fp32 softmax is exactly 0 (the xlogy(0, .) = 0 branch; about 1e-87 in fp64).  The live candidate whose policy logit lies farthest from
    the scene's p-weighted mean lies PEAK above the maximum and takes most of the frozen policy's mass: d kl / d logit = rp - p sum(rp)
    sums to zero over a scene, so only a reference policy concentrated where the head's activations differ from the scene's mean gives the
    KL term a visible gradient.  Returns (ref logits (bs, R, M) fp32, flat index of the underflowing candidate per scene)."""
    cls = case["cls"]
    bs, G = cls.shape
    g = torch.Generator().manual_seed(seed + G)
    ref = 2.0 * torch.randn(bs, G, generator=g)
    mask = case["group_advantage_mask_torch"].view(bs, G)
    z = probability.detach().double().view(bs, G)
    where = []
    for b in range(bs):
        valid = torch.from_numpy(cls[b] >= -1)
        fill = torch.from_numpy(cls[b] == -1) & mask[b]
        j = int(torch.nonzero(fill)[-1]) if fill.any() else int(torch.nonzero(valid)[-1])
        top = float(ref[b][valid].max())
        ref[b, j] = top - 200.0
        where.append(j)
        if mask[b].any():
            pw = torch.softmax(z[b].masked_fill(~valid, -1e8), 0)
            far = (z[b] - (pw * z[b]).sum()).abs().masked_fill(~mask[b], -1.0)
            far[j] = -1.0
            ref[b, int(far.argmax())] = top + PEAK
    return ref.view(bs, -1, M).contiguous(), where


def realised_ratios(probability, r_pad, old_logits):
    """pi / pi_old per candidate in fp64 (bs, G)."""
    bs = probability.shape[0]
    fill = r_pad.unsqueeze(-1)
    lp = F.log_softmax(probability.detach().double().masked_fill(fill, -1e8).view(bs, -1), dim=1)
    lo = F.log_softmax(old_logits.double().masked_fill(fill, -1e8).view(bs, -1), dim=1)
    return (lp - lo).exp().numpy()


def ratio_margin(case, ratios):
    """(largest |realised - target| over the valid candidates, smallest distance of a design ratio from 0.8 / 1.2 / 3.0)."""
    design, valid = case["cls"] >= 0, case["cls"] >= -1
    off = float(np.max(np.abs(ratios - case["target"])[valid])) if valid.any() else 0.0
    return off, min(float(np.min(np.abs(ratios[design] - e))) for e in EDGES)


def classes_by_plane(case, classes):
    """{plane: set of the classes with a live (valid-mask True) member in that plane, over the scenes of the batch}."""
    cls, live = case["cls"], case["group_advantage_mask_torch"].view(case["cls"].shape).numpy()
    out = {}
    for q in range(plane_count(cls.shape[1])):
        part = cls[:, q * 64:(q + 1) * 64][live[:, q * 64:(q + 1) * 64]]
        out[q] = {classes[k] for k in part[part >= 0]}
    return out


def plane_capacity(r_pad):
    """{plane: valid candidates of the batch in that plane}."""
    live = (~r_pad).repeat_interleave(M, dim=1).numpy()
    return {q: int(live[:, q * 64:(q + 1) * 64].sum()) for q in range(plane_count(live.shape[1]))}


# ---- PPO -----------------------------------------------------------------------------------------------------------------------------
# chosen flat index per scene ("last" = the scene's last valid candidate), two variants: run at (clip 0.2, entropy 0.01) and (0.4, 0.2)
PPO_PLACES = {"one": ((0,), ("last",)), "std": ((0, "last", 63, 64, "last"), ("last", 0, 64, 63, 0)),
              "dense": ((0, 63, 64), (63, 64, "last")), "wide": (("last", 0), (64, "last"))}
PPO_FIRST = {"one": 3, "std": 3, "dense": 5, "wide": 2}       # scene 0's entry of K.PPO_RATIOS / K.PPO_ADV (wide: 263 and 64 take an unclipped one)
PPO_SETTINGS = ((0.2, 0.01), (K.PPO_CLIP, K.PPO_ENT))


def ppo_place(probability, r_pad, name, variant):
    """PPO inputs on the policy's own logits: the chosen candidate at PPO_PLACES, old_log_prob putting the ratio on K.PPO_RATIOS (each at
    least 0.1 from a boundary of either clip range), advantages of both signs from K.PPO_ADV."""
    bs, R, _ = probability.shape
    lp = F.log_softmax(probability.detach().double().masked_fill(r_pad.unsqueeze(-1), -1e8).view(bs, -1), dim=1)
    nvalid = (~r_pad).sum(1) * M
    assert bool((~r_pad[:, 0]).all())
    flat = torch.tensor([int(nvalid[b]) - 1 if j == "last" else j for b, j in enumerate(PPO_PLACES[name][variant])])
    assert bool((flat < nvalid).all())
    pick = (torch.arange(bs) * 2 + 3 * variant + PPO_FIRST[name]) % len(K.PPO_RATIOS)
    ratio = torch.tensor(K.PPO_RATIOS, dtype=torch.float64)[pick]
    return {"action_mode_torch": torch.stack([flat // M, flat % M], 1), "advantage_torch": torch.tensor(K.PPO_ADV)[pick],
            "old_log_prob_torch": (lp[torch.arange(bs), flat] - ratio.log()).float(), "ratio": ratio, "flat": flat}


# ---- ties (REINFORCE, SFT) -------------------------------------------------------------------------------------------------------------
TEACHER_T, TEACHER_FR = 25, 10


def teacher_case(bs, R):
    """tests/small_kernel_cases.py sft_case at any (bs, R): integer grid, the candidate (7 + 29 b) % G of scene b -- on a padded line in
    some scenes, as the reference allows -- is the only one 1 from the teacher's speed; every other is at least 2 away."""
    G, T = R * M, TEACHER_T
    traj = torch.zeros(bs, G, T, 6)
    k = torch.clamp((torch.arange(T) + 1) // TEACHER_FR, min=1)
    tgt = [(7 + 29 * b) % G for b in range(bs)]
    for b in range(bs):
        for gi in range(G):
            d = 9 if gi == tgt[b] else (12 + (gi * 7 + b) % 8 if gi % 2 else 8 - (gi + b) % 7)
            traj[b, gi, :, 0] = 100.0 + b + d * k
            traj[b, gi, :, 1] = -40.0 + b
    teacher = torch.tensor([[10.0, 100.0 + b, -40.0 + b, 0.0, 6.0] for b in range(bs)])
    return traj.view(bs, R, M, T, 6).contiguous(), teacher, torch.tensor(tgt) % M


def tie_inputs(r_pad, seed=717):
    """return_torch (fp32, away from 0), the teacher's trajectories / infos and mode, the first valid flat index per scene and the closed
    form of the REINFORCE loss when every valid logit is equal: mean(ret_b log(12 valid lines_b))."""
    bs, R = r_pad.shape
    g = torch.Generator().manual_seed(seed + R)
    ret = (0.5 + torch.rand(bs, generator=g)) * torch.where(torch.arange(bs) % 2 == 0, 1.0, -1.0)
    traj, teacher, m = teacher_case(bs, R)
    first = (~r_pad).float().argmax(1) * M
    lines = (~r_pad).sum(1).double()
    return {"return_torch": ret, "trajectory_torch": traj, "teacher_infos_torch": teacher, "teacher_m": m, "first": first,
            "last": ((R - 1 - (~r_pad).flip(1).float().argmax(1)) * M + M - 1),
            "closed_form": float((ret.double() * torch.log(M * lines)).mean())}


# ---- references ----------------------------------------------------------------------------------------------------------------------
FLOAT_KEYS = ("old_group_logits_torch", "ref_group_logits_torch", "group_advantage_torch", "advantage_torch", "old_log_prob_torch",
              "return_torch", "trajectory_torch", "teacher_infos_torch")
ORACLE_KEYS = FLOAT_KEYS + ("group_advantage_mask_torch", "action_mode_torch")


def _oracle(sd, q_final, kind, b, r_pad, clip_epsilon, lambda_entropy):
    if kind in ("rift", "grpo") and not bool(b["group_advantage_mask_torch"].any()):
        # nothing valid: the reference returns the constant 0.0, which has no graph to differentiate
        prob = mlp_layer(q_final, SD({k: v for k, v in sd.items() if k.startswith(PREFIX)}, PREFIX)).squeeze(-1).masked_fill(r_pad.unsqueeze(-1), -1e6)
        args = (prob, r_pad, b["old_group_logits_torch"]) + ((b["ref_group_logits_torch"],) if kind == "grpo" else ())
        loss = (losses.rift_loss if kind == "rift" else losses.grpo_loss)(*args, b["group_advantage_torch"], b["group_advantage_mask_torch"])
        assert not loss.requires_grad
        return loss.double(), {k: torch.zeros_like(sd[PREFIX + k]) for k in losses.PI_KEYS}, prob
    return losses.pi_head_loss_and_grads(sd, q_final, kind, b, r_pad, clip_epsilon, lambda_entropy)


def objective_ref32(sd, q_final, kind, b, r_pad, clip_epsilon=0.2, lambda_entropy=0.01):
    """oracle.losses.pi_head_loss_and_grads as it stands: (loss, {parameter: gradient}, logits)."""
    return _oracle(sd, q_final.float(), kind, {k: b[k] for k in ORACLE_KEYS if k in b}, r_pad, clip_epsilon, lambda_entropy)


def objective_ref64(sd, q_final, kind, b, r_pad, clip_epsilon=0.2, lambda_entropy=0.01):
    """The same oracle with every float input, the pi_head parameters and q_final cast to fp64."""
    sd64 = {PREFIX + k: sd[PREFIX + k].double() for k in losses.PI_KEYS}
    b64 = {k: (b[k].double() if k in FLOAT_KEYS else b[k]) for k in ORACLE_KEYS if k in b}
    return _oracle(sd64, q_final.double(), kind, b64, r_pad, clip_epsilon, lambda_entropy)


def restated(sd, q_final, kind, b, r_pad, clip_epsilon=0.2, lambda_entropy=0.01, clip=(0.8, 1.2), floor=3.0, dual="neg", kl_weight=0.2,
             valid="mask", tie="first", ppo_modulo=None):
    """The five objectives in plain fp64 with every decision of the kernel as a parameter; at the defaults it is objective_ref64 (asserted
    in tests/test_objective_cases.py).  Returns (loss, {parameter: gradient}, (r, m) chosen per scene or None)."""
    params = {k: sd[PREFIX + k].double().clone().requires_grad_(True) for k in losses.PI_KEYS}
    pi = mlp_layer(q_final.double(), SD({PREFIX + k: v for k, v in params.items()}, PREFIX)).squeeze(-1)
    bs, R, _ = pi.shape
    fill = r_pad.unsqueeze(-1)
    masked = pi.masked_fill(fill, -1e6).masked_fill(fill, -1e8).view(bs, -1)
    lp = F.log_softmax(masked, dim=1)
    rows = torch.arange(bs)
    chosen = None

    def argmax(x):
        return x.argmax(1) if tie == "first" else x.shape[1] - 1 - x.flip(1).argmax(1)

    if kind in ("rift", "grpo"):
        lo = F.log_softmax(b["old_group_logits_torch"].double().masked_fill(fill, -1e8).view(bs, -1), dim=1)
        A = b["group_advantage_torch"].double().view(bs, -1)
        ratio = (lp - lo).exp()
        obj = torch.min(A * ratio, A * ratio.clamp(clip[0], clip[1]))
        if kind == "rift":
            side = {"neg": A < 0, "pos": A > 0, "none": torch.zeros_like(A, dtype=torch.bool)}[dual]
            obj = torch.where(side, torch.max(obj, A * floor), obj)
        else:
            rp = F.softmax(b["ref_group_logits_torch"].double().masked_fill(fill, -1e8).view(bs, -1), dim=1)
            obj = obj - kl_weight * (torch.xlogy(rp, rp) - rp * lp)
        keep = b["group_advantage_mask_torch"].view(bs, -1) if valid == "mask" else (~r_pad).repeat_interleave(M, dim=1)
        loss = -obj[keep].mean() if bool(keep.any()) else torch.zeros((), dtype=torch.float64)
    elif kind == "ppo":
        flat = b["action_mode_torch"][:, 0] * M + b["action_mode_torch"][:, 1]
        if ppo_modulo:
            flat = flat % ppo_modulo
        ratio = (lp[rows, flat] - b["old_log_prob_torch"].double()).exp()
        A = b["advantage_torch"].double()
        ent = -(lp.exp() * lp).sum(1)
        loss = -(torch.min(A * ratio, A * ratio.clamp(1 - clip_epsilon, 1 + clip_epsilon)).mean() + ent.mean() * lambda_entropy)
    elif kind == "reinforce":
        flat = argmax(masked)
        chosen = (flat // M, flat % M)
        loss = -(lp[rows, flat] * b["return_torch"].double()).mean()
    elif kind == "sft":
        _, m = losses.sft_teacher_mode(b["trajectory_torch"], b["teacher_infos_torch"])
        best_r = argmax(masked) // M
        chosen = (best_r, m)
        loss = -lp[rows, best_r * M + m].mean()
    else:
        raise ValueError(kind)
    if loss.requires_grad:
        loss.backward()
    return loss.detach(), {k: (v.grad.detach().clone() if v.grad is not None else torch.zeros_like(v)) for k, v in params.items()}, chosen


MUTANTS = {
    "rift": {"clip 0.7/1.3": dict(clip=(0.7, 1.3)), "dual-clip floor 2 A": dict(floor=2.0), "no dual clip": dict(dual="none"),
             "dual clip on A > 0": dict(dual="pos"), "valid = ~r_pad": dict(valid="lines")},
    "grpo": {"clip 0.7/1.3": dict(clip=(0.7, 1.3)), "KL weight 0.1": dict(kl_weight=0.1), "valid = ~r_pad": dict(valid="lines")},
    "ppo": {"chosen index modulo 64": dict(ppo_modulo=64)},
    "reinforce": {"last-index tie rule": dict(tie="last")},
    "sft": {"last-index tie rule": dict(tie="last")},
}


def mutants(kind):
    """{name: the fp64 reference with one decision changed}: each a function of (sd, q_final, batch, r_pad, ...) like `restated`."""
    return {name: functools.partial(restated, kind=kind, **kw) for name, kw in MUTANTS[kind].items()}


def bar(ref):
    """The project's gradient bar of one tensor (tests/test_gpu_parity.py test_losses_and_pi_head_grads)."""
    return 1e-5 + 1e-4 * float(ref.abs().max())


LOSS_BAR = 1e-5


# ---- one case = the batch entries of one (batch, kind, variant) on given logits ---------------------------------------------------------------
def build_case(name, kind, probability, r_pad, variant=0):
    """The loss inputs of (batch `name`, kind) for the logits `probability`; variant: RIFT / GRPO 1 = the fully masked batch, PPO = index
    into PPO_SETTINGS.  Returns (batch entries, bookkeeping dict)."""
    if kind in ("rift", "grpo"):
        c = place_ratios(probability, r_pad, CLASSES[kind], name, masked=bool(variant))
        info = {k: c.pop(k) for k in ("cls", "target", "filler")}
        if kind == "grpo":
            c["ref_group_logits_torch"], info["underflow"] = ref_logits_case(dict(c, **info), probability)
        return c, info
    if kind == "ppo":
        c = ppo_place(probability, r_pad, name, variant)
        info = {k: c.pop(k) for k in ("ratio", "flat")}
        return c, info
    c = tie_inputs(r_pad)
    info = {k: c.pop(k) for k in ("teacher_m", "first", "last", "closed_form")}
    return c, info
