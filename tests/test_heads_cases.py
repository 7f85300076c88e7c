"""The conditions tests/test_gpu_heads.py rests on, checked on the CPU alone: the fp64 reference of tests/heads_cases.py IS the oracle's
trajectory / prediction / hidden / ref-free heads, the designed batches reach the tile and group boundaries they claim, and every wrong
restatement (mutant) of the reference moves at least one compared tap of one case by three device bars -- so a kernel that computed the
mutant instead would miss its bar three times over.  These are conditions on the case design: a case that fails one is redesigned."""
import pytest
import torch

from oracle import pluto_ref
from tests import heads_cases as HC

# Mutants that stay under three bars at every compared tap of every case, with the ratio shift / E_emu they reach and the reason.  None:
# every mutant clears three bars in both formats.
EXCEPTIONS = {}


@pytest.fixture(scope="module")
def shifts():
    """{mutant: {(case, tap): max shift of the fp64 reference over the compared part}}"""
    out = {}
    for m in HC.MUTANTS:
        out[m] = {}
        for name in HC.CASES:
            enc_out, q_final, _ = HC.oracle_inputs(name)
            mut = HC.reference64(HC.case_weights(), enc_out, q_final, HC.SPEC[name][2], mut=m)
            for tap, d in HC.max_shift(mut, HC.case_reference(name), HC.case(name)).items():
                out[m][name, tap] = d
    return out


def _best(shifts, m, fmt):
    """(bars, shift / E_emu, (case, tap)) of the compared tap a mutant moves by the most device bars (K E_emu)."""
    best = (0.0, 0.0, None)
    for (name, tap), d in shifts[m].items():
        e = HC.case_emu_error(name)[tap, fmt]
        if d / (HC.K[fmt] * e) > best[0]:
            best = (d / (HC.K[fmt] * e), d / e, (name, tap))
    return best


@pytest.mark.parametrize("name", HC.CASES)
def test_reference_is_the_oracle(name):
    """All four outputs of every row (padded lines and agents included) from the oracle's own enc_out / q_final: within 1e-9 of
    oracle.pluto_ref's outputs (the oracle run on double tensors)."""
    out = HC.oracle_inputs(name)[2]
    ref = HC.case_reference(name)
    for t in HC.TAPS:
        assert ref[t].shape == out[t].shape, (name, t)
        d = float((ref[t] - out[t].double()).abs().max())
        print(f"    {name} {t}: |fp64 - oracle| {d:.2e}")
        assert d < 1e-9, (name, t, d)


def test_cases_reach_the_boundaries_they_claim():
    """From the shapes alone: every tile, group and ego-workgroup boundary named below is hit by at least one case."""
    S = {n: HC.shapes(n) for n in HC.CASES}
    plan = {n: s["plan_rows"] for n, s in S.items()}
    pred = {n: s["pred_rows"] for n, s in S.items()}
    # planning rows: under one tile; a multiple of 128 (bs R = 32); a multiple plus 12; more than 1024: nine tiles, group 1 holds one
    assert any(p < HC.TILE for p in plan.values())
    assert any(p % HC.TILE == 0 and s["bs"] * s["R"] == 32 for p, s in zip(plan.values(), S.values()))
    assert any(p > HC.TILE and p % HC.TILE == 12 for p in plan.values())
    assert (S["plan1056"]["bs"], S["plan1056"]["R"], plan["plan1056"]) == (11, 8, 1056)
    assert -(-plan["plan1056"] // HC.TILE) == 9 and plan["plan1056"] > HC.GROUP_ROWS
    # prediction rows: A = 2; A - 1 not dividing 128 with N > A and more than a tile of rows (tiles straddle scenes); exactly 128 rows
    # (bs = 2, A = 65); more than 1024 (bs = 24, A = 45)
    assert any(s["A"] == 2 and s["bs"] > 1 for s in S.values()) and any(s["A"] == 2 and s["bs"] == 1 for s in S.values())
    assert any(HC.TILE % s["per"] != 0 and s["N"] > s["A"] and r > HC.TILE for r, s in zip(pred.values(), S.values()))
    assert (S["p128"]["bs"], S["p128"]["A"], pred["p128"]) == (2, 65, 128)
    assert (S["pred1056"]["bs"], S["pred1056"]["A"], pred["pred1056"]) == (24, 45, 1056) and pred["pred1056"] > HC.GROUP_ROWS
    assert all(s["N"] > s["A"] for s in S.values())                        # polygons behind the agents: stride N is not stride A
    # ego rows: around the 16 rows of an ego_heads_kernel workgroup
    assert {1, 15, 16, 17, 33} <= {s["bs"] for s in S.values()}
    for name in HC.CASES:
        data = HC.case(name)
        rv, av = HC.masks(data)
        s = S[name]
        assert rv.shape == (s["bs"], s["R"]) and av.shape == (s["bs"], s["per"]), name
        assert bool(rv[:, 0].all()), name                                   # every scene keeps a line: no softmax row is fully masked
        assert bool(av.any()), name
        if s["bs"] > 1:
            assert not bool(av.all()), name                                 # a padded agent whose prediction is not compared
        if s["R"] > 1 and s["bs"] > 1:
            assert not bool(rv.all()), name
        for t in HC.TAPS:
            assert torch.isfinite(HC.case_reference(name)[t]).all(), (name, t)


def test_rows_beside_the_gathered_ones_differ_visibly():
    """What a wrong gather would read -- the ego row (offset 0), the first polygon (one past the last agent) and the next scene's ego row --
    differs from the gathered agent rows by far more than an operand rounding of the encoder output."""
    for name in HC.CASES:
        enc = HC.oracle_inputs(name)[0]
        s = HC.shapes(name)
        A = s["A"]
        top = float(enc.abs().max())
        d = [float((enc[:, 0] - enc[:, 1]).abs().max(-1)[0].min()), float((enc[:, A] - enc[:, A - 1]).abs().max(-1)[0].min())]
        if s["bs"] > 1:
            d.append(float((enc[1:, 0] - enc[:-1, A - 1]).abs().max(-1)[0].min()))
        assert min(d) > 0.05 * top, (name, d, top)


def test_emulation_errors_are_those_of_operand_rounding():
    """E_emu: fp16's below bf16's (three more mantissa bits) and small against the tap: two contractions deep, a bf16 operand carries 2^-9
    of relative error."""
    for name in HC.CASES:
        E = HC.case_emu_error(name)
        ref = HC.compared(HC.case_reference(name), HC.case(name))
        for tap in HC.TAPS:
            top = float(ref[tap].abs().max())
            assert 0.0 < E[tap, "fp16"] < E[tap, "bf16"] < 0.02 * top, (name, tap, E[tap, "fp16"], E[tap, "bf16"], top)


def test_bar_factor_is_within_the_limit():
    assert all(1 <= HC.K[f] <= 6 for f in HC.FMT)


@pytest.mark.parametrize("name", HC.CASES)
def test_oracle_in_fp32_stays_within_the_device_bars(name):
    """oracle.pluto_ref's own fp32 evaluation of the heads on the same inputs: within the exact path's bar of the fp64 reference, which is
    below every 16-bit bar -- the bars leave room for a correct fp32 implementation."""
    enc_out, q_final, _ = HC.oracle_inputs(name)
    sd = pluto_ref.SD(HC.case_weights())
    x, q = enc_out.float(), q_final.float()
    bs, R = q.shape[:2]
    A = HC.SPEC[name][2]
    F = torch.nn.functional
    loc, yaw, vel = (pluto_ref.mlp_layer(q, sd.sub(f"planning_decoder.{h}_head")).view(bs, R, 12, 80, 2) for h in HC.HEADS)
    got = {"trajectory": torch.cat([loc, yaw, vel], -1), "prediction": pluto_ref.agent_predictor(x[:, 1:A], sd.sub("agent_predictor")),
           "hidden": pluto_ref.linear(F.relu(pluto_ref.linear(x[:, 0], sd, "hidden_proj.0")), sd, "hidden_proj.2"),
           "ref_free_trajectory": pluto_ref.mlp_layer(x[:, 0], sd.sub("ref_free_decoder")).reshape(bs, 80, 4)}
    E = HC.case_emu_error(name)
    for tap, d in HC.max_shift(got, HC.case_reference(name), HC.case(name)).items():
        print(f"    {name} {tap}: |oracle fp32 - fp64| {d:.2e} (fp32 bar {HC.FP32_BAR:.0e}, fp16 bar {HC.K['fp16'] * E[tap, 'fp16']:.2e})")
        assert d <= HC.FP32_BAR < HC.K["fp16"] * E[tap, "fp16"] < HC.K["bf16"] * E[tap, "bf16"], (name, tap, d)


@pytest.mark.parametrize("mutant", HC.MUTANTS)
def test_mutant_moves_a_tap_by_three_bars(shifts, mutant):
    b16, r16, where16 = _best(shifts, mutant, "fp16")
    bbf, rbf, wherebf = _best(shifts, mutant, "bf16")
    print(f"{mutant}: fp16 {r16:.1f} x E_emu = {b16:.1f} bars at {where16}, bf16 {rbf:.1f} x E_emu = {bbf:.1f} bars at {wherebf}")
    if mutant in EXCEPTIONS:
        assert 1.0 <= bbf < 3.0 and abs(rbf - EXCEPTIONS[mutant][0]) < 0.1 * EXCEPTIONS[mutant][0], (mutant, bbf, rbf)
        return
    assert b16 >= 3.0, (mutant, b16, where16)
    assert bbf >= 3.0, (mutant, bbf, wherebf)


# the outputs a mutant must show on: heads3_fused_kernel writes two of them, ego_heads_kernel the other two
BOTH, EGO_BOTH = ("trajectory", "prediction"), ("hidden", "ref_free_trajectory")
SHOWS_ON = {"heads_reordered": BOTH, "pair_swapped": BOTH, "step_column_mapping": BOTH, "row_of_neighbour_tile": BOTH, "ntiles_9_10_dropped": BOTH,
            "ln_over_128_columns": BOTH + ("ref_free_trajectory",), "gather_offset_0": ("prediction",), "gather_stride_A": ("prediction",),
            "hidden_relu_missing": ("hidden",), "ego_stride_A": EGO_BOTH, "ego_row_of_neighbour_tile": EGO_BOTH}


@pytest.mark.parametrize("mutant", HC.MUTANTS)
def test_mutant_shows_on_every_output_its_kernel_writes(shifts, mutant):
    """... and not on one output alone: three bars in both formats on each output of SHOWS_ON, in some case."""
    for tap in SHOWS_ON[mutant]:
        for fmt in HC.FMT:
            bars = max(d / (HC.K[fmt] * HC.case_emu_error(name)[t, fmt]) for (name, t), d in shifts[mutant].items() if t == tap)
            assert bars >= 3.0, (mutant, tap, fmt, bars)


def test_exception_list_is_short():
    assert len(EXCEPTIONS) <= 3 and set(EXCEPTIONS) <= set(HC.MUTANTS)
