"""Cases of the sampled candidate choice (include/rift_select.h): seeded logits at the shapes that reach every path of control_tick_kernel's
SAMPLE stage, and for each case the uniform numbers u it is asked with -- constructed from the host's own distribution
(rift_amd.planning.pluto.inference.candidate_distribution), not drawn.  tests/test_select_cases.py holds the cases to the properties claimed
here on the CPU; tests/test_gpu_select.py runs them on the device.

The u of a case: for every kept candidate with a positive weight, whose interval of the CDF is [lo, hi) = [c_(j-1) / W, c_j / W) and whose
probability is p = hi - lo: the midpoint, and both ends moved inwards; then u = 0 and u = 1 - 2^-53.  The ends move inwards by 1e-3 * p where
that keeps them EDGE_MARGIN = 1e-4 from the edge (p > 0.1), and by EDGE_MARGIN (and a hair) otherwise: every u is then at least 1e-4 * W from every edge
between two candidates' intervals on the host's weights, which is the precondition under which the device (expf a few ulp from numpy's, the
prefix sums added in another order) must make the same choice.  0 and W are not edges between two choices: u * W < c of the first drawable
candidate holds for u = 0 whatever the rounding, and a u * W that reaches W falls to the rule's last drawable candidate.
"""
import numpy as np

from rift_amd.planning.pluto.inference import candidate_distribution

EDGE_MARGIN = 1e-4          # distance of every constructed u from every interior CDF edge, in units of W
P_MIN = 1e-3                # main cases: the smallest probability of a kept candidate with a positive weight
PAD = np.float32(-1e6)      # the logit of a padded reference line, as the model emits it

# name -> (Rb, topk ('G' = every candidate), temperature, logits recipe, main)
CASES = {
    "rb1_k10": (1, 10, 1.0, "spread3", True),                # G = 12: one partial plane
    "rb1_kG": (1, "G", 1.0, "spread3", True),
    "rb1_k1": (1, 1, 1.0, "spread3", False),                 # topk = 1: the greedy candidate for every u
    "rb11_k10_carry": (11, 10, 1.0, "high_planes", True),    # G = 132, <4> with a partial third plane; every kept candidate in plane 1 or 2
    "rb11_kG_T100": (11, "G", 100.0, "spread1.5", True),     # every plane contributes, close to uniform
    "rb11_kG_dead": (11, "G", 1.0, "dead", False),           # ten padded lines and one -inf logit inside the kept set: 11 drawable of 132 kept
    "rb16_k10_tie": (16, 10, 1.0, "tie", True),              # G = 192: three full planes; two equal logits inside the kept set
    "rb16_k10_T005": (16, 10, 0.05, "gap6", False),          # T = 0.05 with the top 6 ahead: every other weight underflows, greedy for every u
    "rb22_k10": (22, 10, 1.0, "spread3", True),              # G = 264: <16>
    "rb22_kG_T100": (22, "G", 100.0, "spread1.5", True),     # <16>, five planes carried
}
GREEDY_FOR_EVERY_U = ("rb1_k1", "rb16_k10_T005")


def _logits(name, Rb, recipe):
    G = Rb * 12
    g = np.random.default_rng(sum(name.encode()) * 7919 + G)
    if recipe.startswith("spread"):
        z = g.uniform(0.0, float(recipe[6:]), G)
    elif recipe == "high_planes":                            # the ten largest at flat indices >= 64, three of them in the partial plane [128, 132)
        z = g.uniform(-6.0, -4.0, G)
        at = np.concatenate([g.choice(np.arange(64, 128), 7, replace=False), [128, 130, 131]])
        z[at] = g.uniform(0.0, 3.0, 10)
    elif recipe == "tie":                                    # the top ten spread over the three planes, two of them equal (and neither the top)
        z = g.uniform(-6.0, -4.0, G)
        at = np.sort(np.concatenate([g.choice(np.arange(0, 64), 3, replace=False), g.choice(np.arange(64, 128), 3, replace=False),
                                     g.choice(np.arange(128, 192), 4, replace=False)]))
        z[at] = g.uniform(0.0, 2.5, 10)
        z[at[7]] = z[at[2]]
        z[at[5]] = 3.0
    elif recipe == "gap6":
        z = g.uniform(0.0, 3.0, G)
        z[101] = 9.5
    elif recipe == "dead":                                   # line 4 is the live one; every other line is padded; one of its modes is -inf
        z = np.full(G, PAD, dtype=np.float64)
        z[48:60] = g.uniform(0.0, 3.0, 12)
        z[53] = -np.inf
    else:
        raise KeyError(recipe)
    return z.astype(np.float32).reshape(Rb, 12)


def case(name):
    Rb, topk, temperature, recipe, main = CASES[name]
    return {"name": name, "Rb": Rb, "G": Rb * 12, "topk": Rb * 12 if topk == "G" else topk, "temperature": temperature,
            "logits": _logits(name, Rb, recipe), "main": main}


def intervals(c):
    """[(flat index, lo, hi)] of every kept candidate with a positive weight, in ascending flat index: its interval of the CDF, in units of W."""
    _, kept, w, cum = candidate_distribution(c["logits"], c["topk"], c["temperature"])
    W = cum[-1]
    out, lo = [], 0.0
    for j, wj, cj in zip(kept, w, cum):
        if wj > 0:
            out.append((int(j), lo, float(cj / W)))
            lo = float(cj / W)
    return out


def draws(c):
    """The constructed u of a case (module docstring), float64."""
    us = []
    for _, lo, hi in intervals(c):
        move = max(1e-3 * (hi - lo), 1.001 * EDGE_MARGIN)          # (a hair above the margin: the distance is measured through a rounded product)
        us += [0.5 * (lo + hi), lo + move, hi - move]
    us += [0.0, 1.0 - 2.0 ** -53]
    return np.array(us, dtype=np.float64)


def edge_distance(logits, topk, temperature, u):
    """min over the edges between two drawable candidates' intervals of |u * W - c_j| / W (inf when there is one interval only)."""
    _, _, w, cum = candidate_distribution(logits, topk, temperature)
    edges = cum[w > 0][:-1]
    return float(np.min(np.abs(float(u) * cum[-1] - edges)) / cum[-1]) if edges.size else float("inf")


# ---- many CBVs on one batch row: 256 CBVs, u_k = (k + 0.5) / 256, sixteen chunked launches ----------------------------------------------------
MANY_K, MANY_RB, MANY_TOPK, MANY_T, MANY_SEED = 256, 4, 10, 1.0, 0


def many_case():
    g = np.random.default_rng(MANY_SEED)
    return {"Rb": MANY_RB, "G": MANY_RB * 12, "topk": MANY_TOPK, "temperature": MANY_T,
            "logits": g.uniform(0.0, 3.0, (MANY_RB, 12)).astype(np.float32), "u": (np.arange(MANY_K) + 0.5) / MANY_K}


# ---- the chunk seam: 17 CBVs, distinct u, one per sixteenth of [0, 1) and one more -----------------------------------------------------------
SEAM_K = 17


def seam_case():
    c = case("rb1_k10")
    return dict(c, u=(np.arange(SEAM_K) + 0.37) / SEAM_K)
