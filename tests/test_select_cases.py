"""The cases of tests/select_cases.py have the properties claimed for them, and sample_candidate -- the host statement of
include/rift_select.h -- draws from the distribution it reports.  No GPU."""
import numpy as np
import pytest

from rift_amd.planning.pluto import inference as inf
from tests import select_cases as S


def _cases():
    return [S.case(n) for n in S.CASES]


def test_case_table_reaches_every_kernel_path():
    cases = _cases()
    assert {c["Rb"] for c in cases} == {1, 11, 16, 22}                         # one partial plane | <4> with a partial third | three full | <16>
    assert {c["topk"] for c in cases} >= {1, 10, 12, 132, 264} and {c["temperature"] for c in cases} == {0.05, 1.0, 100.0}
    for c in cases:
        assert c["logits"].dtype == np.float32 and c["logits"].shape == (c["Rb"], 12) and 1 <= c["topk"] <= c["G"]
    # the carry matters: every drawable candidate of this case lies in plane 1 or above, some in the partial third plane
    flat = [j for j, _, _ in S.intervals(S.case("rb11_k10_carry"))]
    assert min(flat) >= 64 and max(flat) >= 128 and len(flat) == 10
    # <16>: drawable candidates in five planes
    assert {j >> 6 for j, _, _ in S.intervals(S.case("rb22_kG_T100"))} == {0, 1, 2, 3, 4}
    # two equal logits inside the kept set, both drawable, neither the top
    c = S.case("rb16_k10_tie")
    order, _, w, _ = inf.candidate_distribution(c["logits"], c["topk"], c["temperature"])
    z = c["logits"].reshape(-1)[order]
    dup = [k for k in range(1, len(z)) if z[k] == z[k - 1]]
    assert len(dup) == 1 and dup[0] >= 2 and order[dup[0] - 1] < order[dup[0]] and (w > 0).all()
    # a padded line and a -inf logit inside the kept set: topk above the number of live candidates
    c = S.case("rb11_kG_dead")
    order, kept, w, _ = inf.candidate_distribution(c["logits"], c["topk"], c["temperature"])
    z = c["logits"].reshape(-1)
    assert np.isneginf(z[kept]).sum() == 1 and (z[kept] == S.PAD).sum() == 120 and (w > 0).sum() == 11 and c["topk"] > 11
    assert (w[~np.isfinite(z[kept]) | (z[kept] == S.PAD)] == 0).all() and (z[36:48] == S.PAD).all()


def test_main_cases_keep_every_probability_above_the_floor():
    seen = 0
    for c in _cases():
        p = np.array([hi - lo for _, lo, hi in S.intervals(c)])
        print(f"{c['name']}: {p.size} drawable, p in [{p.min():.3e}, {p.max():.3e}]")
        assert abs(p.sum() - 1.0) < 1e-12
        if c["main"]:
            seen += 1
            assert p.min() >= S.P_MIN, c["name"]
    assert seen >= 6


def test_every_constructed_u_keeps_its_distance_from_every_edge():
    """A precondition on the inputs, not a tolerance: no case is skipped."""
    closest = np.inf
    for c in _cases():
        us = S.draws(c)
        assert us.dtype == np.float64 and (us >= 0).all() and (us < 1).all() and us[-2] == 0.0 and us[-1] == 1.0 - 2.0 ** -53
        assert us.size == 3 * len(S.intervals(c)) + 2
        d = min(S.edge_distance(c["logits"], c["topk"], c["temperature"], u) for u in us)
        closest = min(closest, d)
        assert d >= S.EDGE_MARGIN, (c["name"], d)
    many = S.many_case()
    d_many = min(S.edge_distance(many["logits"], many["topk"], many["temperature"], u) for u in many["u"])
    seam = S.seam_case()
    d_seam = min(S.edge_distance(seam["logits"], seam["topk"], seam["temperature"], u) for u in seam["u"])
    print(f"closest constructed u to an edge: {closest:.3e} W; 256 CBVs on a row: {d_many:.3e} W; seam: {d_seam:.3e} W")
    assert d_many >= S.EDGE_MARGIN and d_seam >= S.EDGE_MARGIN
    assert len(set(seam["u"].tolist())) == S.SEAM_K == 17 and many["u"].size == 256


def test_every_drawable_candidate_is_chosen_by_some_u():
    for c in _cases():
        iv = S.intervals(c)
        got = [inf.sample_candidate(c["logits"], c["topk"], c["temperature"], u) for u in S.draws(c)]
        assert {g[0] for g in got} == {j for j, _, _ in iv}, c["name"]
        # the three u of an interval choose its candidate, with its probability and its position by descending logit
        order = inf.candidate_distribution(c["logits"], c["topk"], c["temperature"])[0]
        for k, (j, lo, hi) in enumerate(iv):
            for flat, pos, p in got[3 * k:3 * k + 3]:
                assert flat == j and order[pos] == j and abs(p - (hi - lo)) < 1e-12
        assert got[-2][0] == iv[0][0] and got[-1][0] == iv[-1][0]               # u = 0: the first drawable; u = 1 - 2^-53: the last
    many = S.many_case()
    assert len({inf.sample_candidate(many["logits"], many["topk"], many["temperature"], u)[0] for u in many["u"]}) == many["topk"]


def test_low_temperature_and_topk_one_are_greedy_for_every_u():
    for name in S.GREEDY_FOR_EVERY_U:
        c = S.case(name)
        assert c["topk"] == 1 or c["temperature"] == 0.05
        top = int(np.argmax(c["logits"].reshape(-1)))
        us = np.concatenate([S.draws(c), np.linspace(0.0, 1.0, 101, endpoint=False)])
        for u in us:
            assert inf.sample_candidate(c["logits"], c["topk"], c["temperature"], u) == (top, 0, 1.0), (name, u)


def test_ties_are_ordered_by_flat_index_whatever_numpy_sorts_by_default():
    """sample_candidate's order is stable; with topk cutting through equal logits the LOWER flat indices are kept."""
    z = np.zeros(24, dtype=np.float32)
    z[[20, 3, 11]] = 1.0
    order, kept, w, _ = inf.candidate_distribution(z, 5, 1.0)
    assert order.tolist() == [3, 11, 20, 0, 1] and kept.tolist() == [0, 1, 3, 11, 20]
    flat, pos, p = inf.sample_candidate(z, 5, 1.0, 0.999)
    assert (flat, pos) == (20, 2) and abs(p - 1.0 / (3.0 + 2.0 * np.exp(np.float32(-1.0)))) < 1e-7
    assert inf.sample_candidate(z, 5, 1.0, 0.0)[:2] == (0, 3)


def test_twenty_thousand_seeded_draws_match_the_probabilities():
    """Frequencies against p within 4 standard errors per candidate."""
    c = S.case("rb16_k10_tie")
    iv = S.intervals(c)
    n = 20000
    g = np.random.default_rng(20260)
    count = {j: 0 for j, _, _ in iv}
    for u in g.random(n):
        count[inf.sample_candidate(c["logits"], c["topk"], c["temperature"], u)[0]] += 1
    for j, lo, hi in iv:
        p = hi - lo
        se = np.sqrt(p * (1 - p) / n)
        print(f"candidate {j}: p {p:.4f} frequency {count[j] / n:.4f} ({(count[j] / n - p) / se:+.2f} se)")
        assert abs(count[j] / n - p) <= 4 * se, (j, p, count[j] / n)
