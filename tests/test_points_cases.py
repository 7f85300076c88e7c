"""The conditions tests/test_gpu_points_encoder.py rests on, checked on the CPU alone: the fp64 reference of tests/points_cases.py IS the
oracle's PointsEncoder, the designed cases hold the masks, tile ends and packed rounds they claim, the shifted biases give both max-pools
channels of all three sign kinds, the train-mode statistics are well defined, every wrong restatement (mutant) moves a compared tap by three
device bars, and the packed-round table's bound holds where the two-line bound it replaced did not.  These are conditions on the case
design: a case that fails one is redesigned."""
import pytest
import torch

from oracle import pluto_ref
from tests import points_cases as PC

NAMES = tuple(PC.CASES)
MODES = (False, True)


def test_reference_is_the_oracle():
    """`ends`, both encoders, eval and train: out and the new running statistics against oracle.pluto_ref.points_encoder (fp32): 1e-4."""
    data, sd = PC.case("ends"), PC.case_weights()
    for train in MODES:
        ref = PC.reference64("ends", train)
        for e, (x, mask) in PC.features(data).items():
            new = {}
            out = pluto_ref.points_encoder(x.float(), mask, pluto_ref.SD(sd, PC.PE[e]), train, new)
            assert float((ref[e]["out"] - out.double()).abs().max()) < 1e-4, (e, train)
            if train:
                for i, bn in ((1, "first_mlp.1"), (2, "second_mlp.1")):
                    assert float((ref[e][f"rm{i}"] - new[PC.PE[e] + bn + ".running_mean"].double()).abs().max()) < 1e-4
                    assert float((ref[e][f"rv{i}"] - new[PC.PE[e] + bn + ".running_var"].double()).abs().max()) < 1e-4
                    assert ref[e][f"nbt{i}"] == int(new[PC.PE[e] + bn + ".num_batches_tracked"]) == 4
            else:
                assert not new


def test_cases_hold_the_masks_tiles_and_rounds_they_claim():
    fa, fb = PC.features(PC.case("ends"))["a"], PC.features(PC.case("ends"))["b"]
    pv, lv = fa[1], fb[1]
    assert pv.shape == (21, 20) and lv.shape == (15, 120)
    assert bool(pv[0].all()) and not bool(pv[1].any()) and pv[2].nonzero().flatten().tolist() == [0] and pv[3].nonzero().flatten().tolist() == [19]
    assert pv[4].nonzero().flatten().tolist() == list(range(4, 16)) and pv[5].nonzero().flatten().tolist() == list(range(0, 20, 2))
    assert bool(pv[20, 19])
    assert PC.tiles_per_line(lv) == [8, 1, 2, 7, 8, 8, 1, 0, 4, 8, 8, 3, 5, 7, 8]
    assert bool(lv[0].all()) and bool(lv[14].all()) and int(lv[5].sum()) == 1 and int(lv[6].sum()) == 1 and int(lv[9].sum()) == 16
    assert not bool(lv[8, 7]) and not bool(lv[8, 32:48].any()) and int(lv[8].sum()) == 60 - 17 and bool(lv[8, 59])
    assert PC.live_rounds(pv, "a") == [0, 1]
    pv, lv = PC.features(PC.case("rounds"))["a"][1], PC.features(PC.case("rounds"))["b"][1]
    assert pv.shape == (40, 20) and lv.shape == (8, 120)
    assert PC.live_rounds(pv, "a") == [0, 2, 3] and PC.live_rounds(lv, "b") == [0, 1, 2, 3]
    assert not bool(pv[24:30].any()) and bool(pv[30:36].any(-1).all())      # a dead 120-row tile inside live round 2
    assert not bool(lv[5].any()) and bool(lv[4].any())                      # a half-dead line round
    for name, long in (("segments_long", True), ("segments_mixed", False)):
        lv = PC.features(PC.case(name))["b"][1]
        t = PC.tiles_per_line(lv)
        assert len(t) == 99 and PC.pack_nseg(99) == 3 and PC.pack_per(99) == 33
        if long:
            assert set(t) == {7, 8} and int(lv.all(-1).sum()) >= 1
        else:
            assert set(t) == set(range(9)) and [l for l in range(99) if t[l] == 0] == [32, 33, 65, 66, 98]


@pytest.mark.parametrize("train", MODES)
def test_both_max_pools_have_channels_of_all_three_sign_kinds(train):
    """The designated fully valid line, partially valid line and partially valid polygon of `ends`: at least 16 channels negative on every
    valid point (a zero row would win the max), at least 16 with a positive maximum (a zero row changes nothing) -- at both maxima."""
    data = PC.case("ends")
    ref = PC.reference64("ends", train, keep_stats=True)
    feats = PC.features(data)
    for e, grp in (("b", PC.ENDS_FULL_LINE), ("b", PC.ENDS_PART_LINE), ("a", PC.ENDS_PART_POLY)):
        mask = feats[e][1][grp]
        full = bool(mask.all())
        assert full == (grp == PC.ENDS_FULL_LINE) and int(mask.sum()) >= 12
        f = ref[e]["_f"][grp][mask]                                  # (valid points, 256): what the first max sees of the valid rows
        assert int((f.max(0)[0] < 0).sum()) >= 16 and int((f.max(0)[0] > 0).sum()) >= 16, (e, grp, "first max")
        o = ref[e]["_o"][grp][mask]                                  # (valid points, 128): the same for the second max
        neg, pos = int((o.max(0)[0] < 0).sum()), int((o.max(0)[0] > 0).sum())
        assert neg >= 16 and pos >= 16, (e, grp, neg, pos)
        out = ref[e]["out"][grp]
        assert int((out == 0).sum()) == (0 if full else neg), "a partially valid polyline's all-negative channels come out 0"
        assert int((out < 0).sum()) == (neg if full else 0)


def test_train_mode_statistics_are_well_defined():
    """At least 64 valid points per encoder in the train-mode runs of every case, and batch variances that are no rounding noise: the
    smallest channel variance is far above BatchNorm's eps = 1e-5."""
    for name in NAMES:
        ref = PC.reference64(name, True, keep_stats=True)
        for e, (_, mask) in PC.features(PC.case(name)).items():
            n = int(mask.sum())
            assert n >= 64, (name, e, n)
            for i in (1, 2):
                vmin = float(ref[e][f"_var{i}"].min())
                assert vmin > 1e-3, (name, e, i, vmin)
    assert int(PC.features(PC.case("rounds"))["a"][1].sum()) == 66 and int(PC.features(PC.case("rounds"))["b"][1].sum()) == 78


def test_eval_and_train_statistics_differ_visibly():
    for e in PC.PE:
        ev, tr = PC.reference64("ends", False)[e], PC.reference64("ends", True)[e]
        for k in ("s1", "t1", "s2", "t2"):
            assert float((ev[k] - tr[k]).abs().max()) > 0.05, (e, k)


def test_emulation_errors_are_those_of_operand_rounding():
    """E_emu: zero for eval-mode s*, t* (running statistics: no contraction in front), fp16's below bf16's elsewhere, small against the tap."""
    for name in NAMES:
        for train in MODES:
            E = PC.emu_error(name, train)
            ref = PC.compared(PC.reference64(name, train), PC.case(name))
            for tap in ref:
                if not train and tap[:2] in ("s1", "t1", "s2", "t2"):
                    assert E[tap, "bf16"] == 0.0 and E[tap, "fp16"] == 0.0 and PC.bar(name, train, tap, "bf16") > 0.0
                else:
                    top = float(ref[tap].abs().max())
                    assert 0.0 < E[tap, "fp16"] < E[tap, "bf16"] < 0.05 * max(top, 1.0), (name, train, tap, E[tap, "fp16"], E[tap, "bf16"], top)


def test_bar_factor_is_within_the_limit():
    assert all(1 <= PC.K[f] <= 6 for f in PC.FMT)


@pytest.fixture(scope="module")
def shifts():
    """{mutant: {(case, train, tap): max shift of the fp64 reference over the compared part of the tap}}"""
    out = {}
    for m in PC.MUTANTS:
        out[m] = {}
        for name in ("ends", "rounds"):
            for train in MODES:
                if m in PC.TRAIN_ONLY and not train:
                    continue
                data = PC.case(name)
                mut = PC.reference(data, PC.case_weights(), train, None, m)
                for tap, d in PC.max_shift(mut, PC.reference64(name, train), data).items():
                    out[m][name, train, tap] = d
    return out


def _best(shifts, m, fmt):
    best = (0.0, 0.0, None)
    for (name, train, tap), d in shifts[m].items():
        b = PC.bar(name, train, tap, fmt)
        if d / b > best[0]:
            E = PC.emu_error(name, train)[tap, fmt]
            best = (d / b, d / E if E > 0 else float("inf"), (name, "train" if train else "eval", tap))
    return best


@pytest.mark.parametrize("mutant", PC.MUTANTS)
def test_mutant_moves_a_tap_by_three_bars(shifts, mutant):
    b16, r16, where16 = _best(shifts, mutant, "fp16")
    bbf, rbf, wherebf = _best(shifts, mutant, "bf16")
    print(f"{mutant}: fp16 {r16:.1f} x E_emu = {b16:.1f} bars at {where16}, bf16 {rbf:.1f} x E_emu = {bbf:.1f} bars at {wherebf}")
    assert b16 >= 3.0, (mutant, b16, where16)
    assert bbf >= 3.0, (mutant, bbf, wherebf)


def test_segments_long_needs_one_record_more_than_two_line_rounds():
    """99 lines of 7 or 8 tiles: three segments of 33 lines, 17 rounds each = 51 records where ceil(99 / 2) = 50 were allocated; the
    table's bound (pe_fused.h: pe_pack_max_rounds) holds them."""
    t = PC.tiles_per_line(PC.features(PC.case("segments_long"))["b"][1])
    assert PC.pack_rounds(t) == 51 and (99 + 1) // 2 == 50 and PC.pack_max_rounds(99) == 51
    assert PC.pack_rounds([6] * 66) == 34 and (66 + 1) // 2 == 33          # (one record beyond the old table)
    t = PC.tiles_per_line(PC.features(PC.case("segments_mixed"))["b"][1])
    assert PC.pack_rounds(t) <= PC.pack_max_rounds(99)


def test_table_bound_holds_for_every_line_count():
    """nL = 1 .. 200 at all-8 and all-6 tile counts (two lines per round: the worst case), and at a mixed pattern: the round count stays
    within pe_pack_max_rounds, which stays within ceil(nL / 2) + nseg; the two-line bound it replaces is broken at some nL."""
    broken = []
    for nl in range(1, 201):
        bound = PC.pack_max_rounds(nl)
        assert (nl + 1) // 2 <= bound <= (nl + 1) // 2 + PC.pack_nseg(nl), (nl, bound)
        for tiles in ([8] * nl, [6] * nl, [1 + (5 * l) % 8 for l in range(nl)]):
            n = PC.pack_rounds(tiles)
            assert n <= bound, (nl, n, bound)
            if n > (nl + 1) // 2:
                broken.append(nl)
    assert 66 in broken and 99 in broken and min(broken) >= 64


def test_check_pack_table_sees_a_wrong_table():
    """The invariants on a hand-made table of three lines (tiles 8, 0, 3) -- and on the same table with one word wrong at a time."""
    tiles = [8, 0, 3]
    tab = [-1] * 16 + [0] * 16
    for l, (first, slot) in ((0, (0, 0)), (2, (8, 1))):
        t = tiles[l]
        for k in range(t):
            tab[first + k] = ((l * 120 + 16 * k) << 8) | (k << 4) | slot
        tab[16 + slot] = first | ((first + t - 1) << 8) | ((1 if t < 8 else 0) << 16) | (1 << 17)
    assert PC.check_pack_table(tiles, [1, 0, 0, 0], tab) == 1
    for i, v in ((3, -1), (9, tab[9] ^ (1 << 4)), (17, 0), (17, tab[17] ^ (1 << 16)), (12, 5), (20, 1 << 17)):
        bad = list(tab)
        bad[i] = v
        with pytest.raises(AssertionError):
            PC.check_pack_table(tiles, [1, 0, 0, 0], bad)
    with pytest.raises(AssertionError):
        PC.check_pack_table(tiles, [2, 0, 0, 0], tab + [-1] * 16 + [0] * 16)      # a record that holds no line
