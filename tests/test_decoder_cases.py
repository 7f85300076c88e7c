"""The conditions tests/test_gpu_planning_decoder.py rests on, checked on the CPU alone: the fp64 reference of tests/decoder_cases.py IS the
oracle's planning decoder, the designed batches hold the key counts, line paddings and quirk rows they claim, and every wrong restatement
(mutant) of the reference moves at least one compared tap of one case by three device bars -- so a kernel that computed the mutant instead
would miss its bar three times over.  These are conditions on the case design: a case that fails one is redesigned."""
import pytest
import torch

from tests import decoder_cases as DC
from tests import helpers as H

# Mutants that stay under 3 K["bf16"] E_emu[.., bf16] at every compared tap of every case, with the ratio shift / E_emu they reach (at most
# three may stand here; every one of them must clear one bar in bf16 and three in fp16).  None: under decoder_cases.SCALES every mutant
# clears three bf16 bars (profiles/NOTES_r17.md).
BF16_EXCEPTIONS = {}


@pytest.fixture(scope="module")
def shifts():
    """{mutant: {(case, tap): max shift of the fp64 reference over all rows}}"""
    out = {}
    for m in DC.MUTANTS:
        out[m] = {}
        for name in DC.ONLY.get(m, DC.CASES):
            r_emb, enc_out, kpm, r_kpm, _ = DC.oracle_inputs(name)
            mut = DC.reference64(DC.case_weights(), r_emb, enc_out, kpm, r_kpm, mut=m)
            for tap, d in DC.max_shift(mut, DC.case_reference(name), taps=DC.TAPS).items():
                out[m][name, tap] = d
    return out


def _best(shifts, m, fmt):
    """(bars, shift / E_emu, (case, tap)) of the compared tap a mutant moves by the most device bars (K E_emu)."""
    best = (0.0, 0.0, None)
    for (name, tap), d in shifts[m].items():
        e = DC.case_emu_error(name)[tap, fmt]
        if d / (DC.K[fmt] * e) > best[0]:
            best = (d / (DC.K[fmt] * e), d / e, (name, tap))
    return best


@pytest.mark.parametrize("name", ["small", "full"])
def test_reference_is_the_oracle_on_the_suite_fixtures(name):
    """q0, dec0..dec3 and q_final of every row (padded lines included) under the suite's weights as they are, from the oracle's own r_emb /
    enc_out: within 1e-5 of oracle.pluto_ref's taps (the oracle run on double tensors: in fp32 its own rounding alone is 1.1e-5 on `small`)."""
    r_emb, enc_out, kpm, r_kpm, taps = DC.oracle_inputs(name, scaled=False)
    ref = DC.reference64(H.weights(), r_emb, enc_out, kpm, r_kpm)
    for t in DC.ALL_TAPS:
        d = float((ref[t] - taps[t].double()).abs().max())
        print(f"    {name} {t}: |fp64 - oracle| {d:.2e}")
        assert d < 1e-5, (name, t, d)


@pytest.mark.parametrize("name", DC.CASES)
def test_reference_is_the_oracle_on_the_designed_cases(name):
    """... and under the rescaled weights on the designed batches (holes, padded ego, quirk rows that expose padded lines): 1e-5."""
    taps = DC.oracle_inputs(name)[4]
    for t in DC.ALL_TAPS:
        d = float((DC.case_reference(name)[t] - taps[t].double()).abs().max())
        assert d < 1e-5, (name, t, d)


def test_cases_hold_the_keys_lines_and_quirk_rows_they_claim():
    for name, (_, A, Mp, R, keys, lines) in DC.SPEC.items():
        kpm, r_kpm = DC.paddings(DC.case(name))
        assert kpm.shape == (len(keys), A + Mp) and r_kpm.shape == (len(keys), R), name
        assert (~kpm).sum(1).tolist() == [abs(k) for k in keys], name
        assert [bool(kpm[b, 0]) for b in range(len(keys))] == [k < 0 for k in keys], name          # the ego slot is padded only where asked
        want = [set(range(ln)) if isinstance(ln, int) else set(ln) for ln in lines]
        assert [set(torch.nonzero(~r_kpm[b]).flatten().tolist()) for b in range(len(keys))] == want, name
        assert all(len(w) >= 1 for w in want) and all(abs(k) >= 1 for k in keys), name                # no softmax row is fully masked
        for t in DC.ALL_TAPS:
            assert torch.isfinite(DC.case_reference(name)[t]).all(), (name, t)
        for b in range(len(keys)):                                                                   # scattered: the valid keys are no prefix
            if 2 < abs(keys[b]) < A + Mp - 2:
                assert bool(kpm[b, :abs(keys[b])].any()), (name, b)
    # key tiles of sixteen: the batch's tile count, and scenes on both sides of a per-scene tile edge
    assert [DC.SPEC[n][1] + DC.SPEC[n][2] for n in DC.CASES] == [80, 96, 112, 128, 40, 192]
    for name, edge in (("std80", 64), ("std80", 16), ("std96", 80), ("mid112", 96), ("mid128", 112), ("dense_192", 176)):
        keys = [abs(k) for k in DC.SPEC[name][4]]
        assert edge in keys and edge + 1 in keys, (name, edge)
    assert DC.SPEC["dense_r9"][3] == 9 and DC.SPEC["dense_192"][3] == 16
    # std80: bs = 9 does not divide 12, so the twelve modes of a scene draw their quirk rows from several scenes
    kpm, r_kpm = DC.paddings(DC.case("std80"))
    bs = r_kpm.shape[0]
    quirk = DC.quirk_rows(r_kpm).view(bs, DC.M, -1)
    assert torch.equal(quirk[3, 5], r_kpm[(12 * 3 + 5) % bs])
    own = r_kpm[:, None, :].expand_as(quirk)
    exposes = (~quirk & own).any(-1)                       # a padded line of the scene is a key
    masks = (quirk & ~own).any(-1)                         # a valid line of the scene is masked
    only_padded = (quirk | own).all(-1)                    # every valid line masked: what is left are padded lines only
    assert bool(exposes.any()) and bool(masks.any()) and bool(only_padded.any())
    assert bool((~quirk).any(-1).all())                    # ... and every row keeps a key
    assert all(len({(12 * b + m) % bs for m in range(12)}) > 1 for b in range(bs))


def test_emulation_errors_are_those_of_operand_rounding():
    """E_emu: fp16's below bf16's (three more mantissa bits) and small against the tap: a bf16 operand carries 2^-9 of relative error, some
    forty contractions deep that is a few per cent of the largest value at the most."""
    for name in DC.CASES:
        E = DC.case_emu_error(name)
        for tap in DC.ALL_TAPS:
            top = float(DC.case_reference(name)[tap].abs().max())
            assert 0.0 < E[tap, "fp16"] < E[tap, "bf16"] < 0.02 * top, (name, tap, E[tap, "fp16"], E[tap, "bf16"], top)


def test_bar_factor_is_within_the_limit():
    assert all(1 <= DC.K[f] <= 6 for f in DC.FMT)


@pytest.mark.parametrize("mutant", DC.MUTANTS)
def test_mutant_moves_a_tap_by_three_bars(shifts, mutant):
    b16, r16, where16 = _best(shifts, mutant, "fp16")
    bbf, rbf, wherebf = _best(shifts, mutant, "bf16")
    print(f"{mutant}: fp16 {r16:.1f} x E_emu = {b16:.1f} bars at {where16}, bf16 {rbf:.1f} x E_emu = {bbf:.1f} bars at {wherebf}")
    assert b16 >= 3.0, (mutant, b16, where16)
    if mutant in BF16_EXCEPTIONS:
        assert 1.0 <= bbf < 3.0, f"{mutant}: {bbf:.1f} bf16 bars -- off the list above three, a missing case or scale under one"
        assert abs(rbf - BF16_EXCEPTIONS[mutant]) < 0.1 * BF16_EXCEPTIONS[mutant], (mutant, rbf)
    else:
        assert bbf >= 3.0, (mutant, bbf, wherebf)


def test_exception_list_is_short():
    assert len(BF16_EXCEPTIONS) <= 3 and set(BF16_EXCEPTIONS) <= set(DC.MUTANTS)
