"""Case tables and the plain fp64 restatement of the arena advantage (include/rift_advantage.h states the rule): the group advantage of
every candidate of a replay arena from its stored returns, under a baseline, a scale and a clip.  Shared by
tests/test_advantage_param_cases.py (CPU: the restatement against the oracle's z-score and the conditions the inputs must satisfy) and
tests/test_gpu_advantage_params.py (the kernels against the restatement).  Nothing here calls the library."""
import functools
import itertools

import numpy as np

BASELINES = ("mean", "leave_one_out", "none")
SCALES = ("group_std", "batch_rms", "none")
CLIPS = (0.0, 1.5)
EPSS = (1e-5, 0.0)
NS = (1, 3, 4, 5, 9)                      # scenes: four per workgroup, so a ragged last workgroup but for 4
RCAPS = (1, 5, 6, 11, 17)                 # 12 .. 204 candidates: below, at and above one, two and three wave widths
BIG = (2051, 1)                           # the fixed-order reduction: past its 1024 threads, ragged
MASKS = ("none", "holes", "scene_masked", "one_valid", "two_valid")
DISTS = ("normal", "shifted", "constant")  # N(0, 1) | -300 + 0.5 z (tests/small_kernel_cases.py) | normal with two scenes of one constant value
CONSTANTS = (2.5, -300.5)                 # few mantissa bits: any sum of up to 204 of them is exact, so the group's sd is exactly 0
CLIP_MARGIN = 1e-6
SHAPES = tuple(itertools.product(NS, RCAPS)) + (BIG,)


def case_ids():
    return [f"n{n}_R{r}" for n, r in SHAPES]


@functools.lru_cache(maxsize=None)
def case(k, seed=20261):
    """Inputs of shape k of SHAPES: returns (n, Rcap, 12) f64 (every element drawn, valid or not), r_count (n) i32 or None, mask
    (n, Rcap, 12) u8 or None, and the kind of mask and distribution it was built with.  The kinds rotate with k so that every pair of them
    occurs (tests/test_advantage_param_cases.py holds that)."""
    n, Rcap = SHAPES[k]
    mask_kind, dist = MASKS[(k // 5 + k % 5) % 5], DISTS[k % 3]
    rng = np.random.default_rng(seed + 7 * k)
    z = rng.standard_normal((n, Rcap, 12))
    ret = -300.0 + 0.5 * z if dist == "shifted" else z.copy()
    const_scenes = ()
    if dist == "constant":
        const_scenes = (0, n - 1) if n > 1 else (0,)
        for j, i in enumerate(const_scenes):
            ret[i] = CONSTANTS[j]
    r_count = rng.integers(1, Rcap + 1, size=n).astype(np.int32)
    r_count[0] = Rcap
    if n >= 3:
        r_count[1] = 0
    if k % 4 == 0:
        r_count = None                      # every scene has Rcap lines
    mask = None
    if mask_kind != "none":
        mask = (rng.random((n, Rcap, 12)) > 0.25).astype(np.uint8) * rng.integers(1, 256, size=(n, Rcap, 12)).astype(np.uint8)    # any non-zero byte is valid
        if mask_kind == "scene_masked":
            mask[n - 1] = 0
        elif mask_kind in ("one_valid", "two_valid"):
            mask[0] = 0
            mask[0].reshape(-1)[rng.choice(Rcap * 12, size=1 if mask_kind == "one_valid" else 2, replace=False)] = 1
    return {"n": n, "Rcap": Rcap, "returns": ret, "r_count": r_count, "mask": mask, "mask_kind": mask_kind, "dist": dist,
            "const_scenes": const_scenes}


def settings(k):
    """The (baseline, scale, clip, eps) every shape is run under: all of them, but for BIG (every baseline x scale pair at clip 1.5)."""
    if SHAPES[k] == BIG:
        return [(b, s, 1.5, 1e-5) for b in BASELINES for s in SCALES]
    return list(itertools.product(BASELINES, SCALES, CLIPS, EPSS))


def valid_of(c):
    n, Rcap = c["n"], c["Rcap"]
    valid = np.zeros((n, Rcap, 12), dtype=np.bool_)
    for i in range(n):
        valid[i, :Rcap if c["r_count"] is None else int(c["r_count"][i])] = True
    if c["mask"] is not None:
        valid &= c["mask"] != 0
    return valid


def restate(c, baseline, scale, clip, eps):
    """The rule, scene by scene in fp64 numpy.  -> advantage (n, Rcap, 12), the value before the clamp, stats [8]."""
    ret, valid = c["returns"], valid_of(c)
    n = c["n"]
    cen = np.zeros_like(ret)
    sd = np.zeros(n)
    G = np.zeros(n, dtype=np.int64)
    for i in range(n):
        x = ret[i][valid[i]]
        G[i] = x.size
        if x.size == 0:
            continue
        mean = np.mean(x)
        sd[i] = np.sqrt(np.mean((x - mean) ** 2))
        if baseline == "mean":
            ci = x - mean
        elif baseline == "leave_one_out":
            ci = (x - mean) * (x.size / (x.size - 1)) if x.size > 1 else np.zeros_like(x)
        else:
            ci = x
        cen[i][valid[i]] = ci
    N = int(G.sum())
    rms = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        if scale == "group_std":
            raw = np.where(valid, cen / (sd + eps)[:, None, None], 0.0)
        elif scale == "batch_rms":
            rms = float(np.sqrt(np.sum(cen[valid] ** 2) / N)) if N else 0.0
            raw = np.where(valid, cen / (rms + eps), 0.0)
        else:
            raw = cen
    adv = np.clip(raw, -clip, clip) if clip > 0 else raw
    clamped = int(np.sum(np.abs(raw[valid]) > clip)) if clip > 0 else 0
    stats = np.array([N, int(np.sum(G > 0)), int(np.sum((G > 0) & (sd == 0.0))), rms, clamped, 0, 0, 0], dtype=np.float64)
    return adv, raw, stats


def is_case(c, baseline, scale, clip, eps):
    """With eps = 0 a denominator can be exactly 0 (a constant group or a single candidate under GROUP_STD, an arena whose centred values
    are all 0 under BATCH_RMS): 0 / 0 is not a case."""
    _, raw, _ = restate(c, baseline, scale, clip, eps)
    return bool(np.isfinite(raw).all())


def loo_literal(c):
    """LEAVE_ONE_OUT as it is said: x_j minus the mean of the OTHER valid candidates of its scene (0 where there is none)."""
    ret, valid = c["returns"], valid_of(c)
    out = np.zeros_like(ret)
    for i in range(c["n"]):
        idx = np.argwhere(valid[i])
        for r, m in idx:
            others = [ret[i, r2, m2] for r2, m2 in idx if (r2, m2) != (r, m)]
            out[i, r, m] = ret[i, r, m] - np.mean(others) if others else 0.0
    return out
