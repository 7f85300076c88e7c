"""The conditions tests/test_gpu_history_encoder.py rests on, checked on the CPU alone: the fp64 reference of tests/history_cases.py IS the
oracle's history encoder, the designed cases hold the tiles, holes and neighbours they claim, and every wrong restatement (mutant) of the
reference moves at least one compared tap of one case by three device bars -- so a kernel that computed the mutant instead would miss its
bar three times over.  These are conditions on the case design: a case that fails one is redesigned."""
import pytest

from oracle import pluto_ref
from tests import helpers as H
from tests import history_cases as HC

NAMES = tuple(HC.CASES)

# Mutants that stay under 3 K["bf16"] E_emu[.., bf16] at every tap of every case, with the ratio shift / E_emu they reach (at most three may
# stand here; every one of them clears 3 K["fp16"] E_emu[.., fp16] like all the others).  Level 2's truncated left edge changes queries 0 and 1
# only, which oc2 (steps 2..4) sees as two of the five keys of the second block: 8.2 E_emu in bf16 (2.7 bars), 66.6 in fp16 (22 bars).
BF16_EXCEPTIONS = {"window_left_l2": 8.2}


@pytest.fixture(scope="module")
def shifts():
    """{mutant: {(case, tap): max shift of the fp64 reference over the history sequences}}"""
    out = {}
    for m in HC.MUTANTS:
        out[m] = {}
        for name in NAMES:
            data = HC.case(name)
            hist = HC.ranking(data)[0]
            for tap, d in HC.max_shift(HC.reference(data, HC.case_weights(), None, m), HC.reference64(name), hist).items():
                out[m][name, tap] = d
    return out


def _best(shifts, m, fmt):
    """(bars, shift / E_emu, (case, tap)) of the compared tap a mutant moves by the most device bars (HC.bar: K E_emu; f9: its absolute bar)."""
    best = (0.0, 0.0, None)
    for (name, tap), d in shifts[m].items():
        bars = d / HC.bar(name, tap, fmt)
        if bars > best[0]:
            best = (bars, d / (HC.F9_BAR if tap == "f9" else HC.emu_error(name)[tap, fmt]), (name, tap))
    return best


def test_reference_is_the_oracle_on_the_full_fixture():
    """F9 rows and the encoder's output of the 115 history sequences of `full` (reference weights, rpb as generated) against
    oracle.pluto_ref's fp32 agent_features / nat_sequence_encoder: 1e-5; and the reference's level-2 tap against the oracle's."""
    data, sd = HC.case("full"), H.weights()
    ref = HC.reference(data, sd)
    valid = data["agent"]["valid_mask"][:, :, :21].any(-1).flatten()
    feat = pluto_ref.agent_features(data).reshape(-1, 20, 9)
    assert float((ref["f9"] - feat.double()).abs().max()) < 1e-5
    taps = {}
    out = pluto_ref.nat_sequence_encoder(feat[valid].permute(0, 2, 1).contiguous(), pluto_ref.SD(sd, HC.HE), taps)
    assert int(valid.sum()) == 117 and int(HC.ranking(data)[0].sum()) == 115
    assert float((ref["out"][valid] - out.double()).abs().max()) < 1e-5
    assert float((ref["level2"][valid] - taps["nat_level2"].double()).abs().max()) < 1e-5


def test_cases_hold_the_tiles_and_histories_they_claim():
    hist, aidx, cnt = HC.ranking(HC.case("edges"))
    assert hist.numel() == 24 and int(hist.sum()) == 19 and cnt == [6, 7, 6] and aidx.numel() == 21
    assert int((aidx[16:20] >= 0).sum()) == 3 and int((aidx[18:21] >= 0).sum()) == 1
    v = HC.case("edges")["agent"]["valid_mask"]
    assert v.shape[2] > 21 and bool(v[0, 5, 21:].all()) and not bool(v[0, 5, :21].any()) and not bool(hist[5])
    pair = v[:, :, 1:21] & v[:, :, :20]
    assert bool(hist[6]) and int(v[0, 6, :21].sum()) == 1 and not bool(pair[0, 6].any())
    assert not bool(v[0, 1, 0]) and not bool(v[0, 2, 20]) and not bool(v[0, 3, 7]) and bool(v[0, 3, 6]) and bool(v[0, 3, 8])
    f9 = HC.reference64("edges")["f9"].abs().amax(dim=(1, 2))
    for s in (8, 13):                                 # a quiet history sequence between two loud rows
        assert bool(hist[s]) and float(f9[s - 1]) > 20 * float(f9[s]) and float(f9[s + 1]) > 20 * float(f9[s])
    hist, aidx, cnt = HC.ranking(HC.case("one"))
    assert int(hist.sum()) == 1 and cnt == [0, 1, 0]
    hist, aidx, cnt = HC.ranking(HC.case("rounds"))
    assert hist.numel() == 72 and 64 <= int(hist.sum()) <= 70 and cnt == [21, 23, 22]
    assert 64 < aidx.numel() <= 96                    # three groups of eight four-agent tiles
    assert 22 <= aidx.numel() // 3 <= 24              # three rounds of eight three-agent tiles, the last partial


def test_emulation_errors_are_those_of_operand_rounding():
    """E_emu: zero where no contraction stands in front, fp16's below bf16's (three more mantissa bits), and small against the tap: a
    bf16 operand carries 2^-9 of relative error, some twenty contractions deep that is a few per cent of the largest value at the most."""
    for name in NAMES:
        E = HC.emu_error(name)
        hist = HC.ranking(HC.case(name))[0]
        for tap in HC.TAPS + ("level2",):
            if tap == "f9":
                assert E[tap, "bf16"] == 0.0 and E[tap, "fp16"] == 0.0
            else:
                top = float(HC.reference64(name)[tap][hist].abs().max())
                assert 0.0 < E[tap, "fp16"] < E[tap, "bf16"] < 0.05 * top, (name, tap, E[tap, "fp16"], E[tap, "bf16"], top)


def test_bar_factor_is_within_the_limit():
    assert all(1 <= HC.K[f] <= 6 for f in HC.FMT)


@pytest.mark.parametrize("mutant", HC.MUTANTS)
def test_mutant_moves_a_tap_by_three_bars(shifts, mutant):
    b16, r16, where16 = _best(shifts, mutant, "fp16")
    bbf, rbf, wherebf = _best(shifts, mutant, "bf16")
    print(f"{mutant}: fp16 {r16:.1f} x E_emu = {b16:.1f} bars at {where16}, bf16 {rbf:.1f} x E_emu = {bbf:.1f} bars at {wherebf}")
    assert b16 >= 3.0, (mutant, b16, where16)
    if mutant in BF16_EXCEPTIONS:
        assert bbf < 3.0, f"{mutant} clears three bf16 bars: take it off the list"
        assert abs(rbf - BF16_EXCEPTIONS[mutant]) < 0.1 * BF16_EXCEPTIONS[mutant], (mutant, rbf)
    else:
        assert bbf >= 3.0, (mutant, bbf, wherebf)


def test_exception_list_is_short():
    assert len(BF16_EXCEPTIONS) <= 3 and set(BF16_EXCEPTIONS) <= set(HC.MUTANTS)
