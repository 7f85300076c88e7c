"""The agent-history chain -- prep_kernel's F9 rows, nat_l0w / nat_l1w / nat_l2w_kernel, fpn_tail_kernel -- against the fp64 reference of
tests/history_cases.py at every level boundary the engine taps (nat_f9, nat_x1, nat_x2, nat_oc0..2, nat_level2, nat_out), on the designed
cases `edges`, `one` and `rounds`, eval forward only (DropPath: tests/test_gpu_dropstats.py).  tests/test_history_cases.py proves on the
CPU that a wrong window, rpb index, conv tap, downsample phase, upsample rule or tile neighbour moves one of these taps by three bars.

Bars.  16-bit builds: K[fmt] * E_emu[case, tap, fmt] -- E_emu = what rounding both operands of every contraction to the format costs the
fp64 reference, K one factor per build for all taps and cases (history_cases.K; measured ratios in profiles/NOTES_r14.md).  fp32: 1e-4.
nat_f9: differences, shape and validity bit-exact, cos / sin within 2e-6.  The fused path's rows are in compacted order and are mapped
through nat_aidx / nat_cnt; only history sequences are compared (the other ranks of a tile are holes nobody reads).
Needs a real MI355X: `pytest -m gpu`."""
import os

import pytest
import torch

from tests import history_cases as HC

pytestmark = pytest.mark.gpu

NAMES = tuple(HC.CASES)
CH = {"x1": (10, 64), "x2": (5, 128), "oc0": (3, 32), "oc1": (3, 64), "oc2": (3, 128), "level2": (5, 128), "out": (128,), "f9": (20, 9)}
# build -> (operand format, environment of the context, fp32 forward, cases)
BUILDS = {
    "bf16": ("bf16", {}, False, NAMES), "fp16": ("fp16", {}, False, NAMES),
    "bf16-layerwise": ("bf16", {"RIFT_NAT_UNFUSED": "1"}, False, NAMES), "fp16-layerwise": ("fp16", {"RIFT_NAT_UNFUSED": "1"}, False, NAMES),
    "fp32": ("bf16", {}, True, NAMES),
    "bf16-grid1": ("bf16", {"RIFT_NAT_GRID": "1"}, False, ("rounds",)), "fp16-grid1": ("fp16", {"RIFT_NAT_GRID": "1"}, False, ("rounds",)),
    "bf16-grid2": ("bf16", {"RIFT_NAT_GRID": "2"}, False, ("rounds",)), "fp16-grid2": ("fp16", {"RIFT_NAT_GRID": "2"}, False, ("rounds",)),
    "bf16-poison": ("bf16", {"RIFT_POISON_ARENA": "255"}, False, ("edges",)), "fp16-poison": ("fp16", {"RIFT_POISON_ARENA": "255"}, False, ("edges",)),
}
WORD = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def ffi():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    _ffi.load_library()
    return _ffi


@pytest.fixture(scope="module")
def runs(ffi):
    """build -> {case: {tap: CPU tensor in SLOT order, rows of slots that are no history sequence zero}}: one engine per build, made on
    first use with the build's switches in the environment (the context reads them when it is created)."""
    cache, prob = {}, {}

    def get(build):
        """(taps of every case of the build, {(build, case): the forward's `probability`})"""
        return taps_of(build), prob

    def taps_of(build):
        if build in cache:
            return cache[build]
        fmt, env, fp32, names = BUILDS[build]
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            eng = ffi.Engine("cuda:0", operands=fmt)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        eng.load_state_dict({k: v.clone() for k, v in HC.case_weights().items()})
        cache[build] = {}
        for name in names:
            data = HC.case(name)
            hist, aidx, cnt = HC.ranking(data)
            nA = hist.numel()
            keep = lambda x: torch.where(hist.view(-1, *[1] * (x.dim() - 1)), x, torch.zeros(()))
            out = eng.forward(data, fp32=fp32)
            torch.cuda.synchronize()
            prob[build, name] = out["probability"].cpu().clone()
            fused = not fp32 and "RIFT_NAT_UNFUSED" not in env
            raw = {t: eng.tap("nat_" + t).cpu() for t in (HC.TAPS if fused else ("f9", "oc0", "oc1", "oc2", "level2", "out"))}
            got = {"f9": raw["f9"].view(nA, 20, 9), "out": keep(raw["out"].view(nA, 128))}
            if fused:
                d_aidx, d_cnt = eng.tap("nat_aidx").cpu().view(torch.int32), eng.tap("nat_cnt").cpu().view(torch.int32)
                assert d_cnt.tolist() == cnt, (build, name, d_cnt.tolist(), cnt)
                live = aidx >= 0
                assert torch.equal(d_aidx[:aidx.numel()][live].long(), aidx[live]), (build, name)
                for t in ("x1", "x2", "oc0", "oc1", "oc2"):
                    rows = raw[t].view(WORD[fmt]).float() if t.startswith("oc") else raw[t]      # (oc*: the 16-bit words the FPN tail receives)
                    rows = rows.view(nA, *CH[t])[:aidx.numel()]
                    full = torch.zeros(nA, *CH[t])
                    full[aidx[live]] = rows[live]
                    got[t] = full
            else:
                for t in ("oc0", "oc1", "oc2", "level2"):
                    got[t] = keep(raw[t].view(nA, *CH[t]))
            cache[build][name] = got
        eng.close()
        return cache[build]

    return get


def _f9(got, ref):
    """Differences, shape and validity: the fp32 value of the exact difference.  cos / sin: 2e-6."""
    exact = [0, 1, 2, 3, 6, 7, 8]
    assert torch.equal(got[..., exact], ref[..., exact].float()), "F9 difference / shape / validity columns"
    e = float((got[..., 4:6].double() - ref[..., 4:6]).abs().max())
    print(f"    f9 cos / sin: {e:.2e} (bar {HC.F9_BAR:.0e})")
    assert e <= HC.F9_BAR


@pytest.mark.parametrize("build", ["bf16", "fp16", "bf16-layerwise", "fp16-layerwise"])
def test_sixteen_bit_taps_within_k_operand_rounding_errors(runs, build):
    """Every tap the path offers, every case, history sequences only: |device - fp64| <= K[fmt] * E_emu[case, tap, fmt].
    Measured on MI355X, worst device error / E_emu over all taps and cases: bf16 fused 1.26 (rounds, oc0), fp16 fused 1.29 (one, oc2),
    bf16 layer-wise 1.25, fp16 layer-wise 1.20 -- K = 3 for both builds; every figure in profiles/NOTES_r14.md."""
    fmt = BUILDS[build][0]
    got = runs(build)[0]
    worst, late = (0.0, None), []
    for name in NAMES:
        ref, hist, E = HC.reference64(name), HC.ranking(HC.case(name))[0], HC.emu_error(name)
        _f9(got[name]["f9"], ref["f9"])
        for t, g in got[name].items():
            if t == "f9":
                continue
            assert torch.isfinite(g).all(), (build, name, t)
            err = float((g.double()[hist] - ref[t][hist]).abs().max())
            ratio = err / E[t, fmt]
            print(f"    {build} {name} {t}: |device - fp64| {err:.3e}, E_emu {E[t, fmt]:.3e}, ratio {ratio:.2f} (K {HC.K[fmt]})")
            worst = max(worst, (ratio, (name, t)))
            if err > HC.bar(name, t, fmt):
                late.append((name, t, err, HC.bar(name, t, fmt)))
    print(f"  {build}: worst device error / E_emu = {worst[0]:.2f} at {worst[1]}")
    assert not late, late


def test_fp32_taps(runs):
    """The exact-fp32 layer-wise path: every tap within 1e-4 of the fp64 reference (measured: 8.4e-6 at the worst, level2 of `rounds`)."""
    got = runs("fp32")[0]
    late = []
    for name in NAMES:
        ref, hist = HC.reference64(name), HC.ranking(HC.case(name))[0]
        _f9(got[name]["f9"], ref["f9"])
        for t, g in got[name].items():
            if t == "f9":
                continue
            err = float((g.double()[hist] - ref[t][hist]).abs().max())
            print(f"    fp32 {name} {t}: |device - fp64| {err:.3e}")
            if not err <= 1e-4:
                late.append((name, t, err))
    assert not late, late


def _identical(a, b, what):
    assert a.keys() == b.keys()
    for t in a:
        assert torch.equal(a[t], b[t]), f"{what}: tap {t} differs in {int((a[t] != b[t]).sum())} words"


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("grid", ["1", "2"])
def test_persistent_loops_and_round_major_dealing_are_bit_identical(runs, fmt, grid):
    """`rounds` with RIFT_NAT_GRID = 1 (levels 0 and 1: three iterations of one workgroup's persistent loop, level 1 re-loading layer 0's
    weights for each tile group; level 2: round-major dealing, rounds of 8, 8 and 7 tiles) and = 2 (the two workgroups run two rounds and
    one) against the default grid (one iteration, wave-major dealing): every history tap bit for bit."""
    _identical(runs(f"{fmt}-grid{grid}")[0]["rounds"], runs(fmt)[0]["rounds"], f"{fmt} RIFT_NAT_GRID={grid}")
    # the switch also sizes the points encoder's persistent launch (never under two workgroups: one per side): the rest of the forward
    # has no reduction across workgroups in eval mode (BatchNorm on running statistics, max pooling), so its output does not move either
    p = runs(fmt)[1]
    d = float((p[f"{fmt}-grid{grid}", "rounds"] - p[fmt, "rounds"]).abs().max())
    print(f"    {fmt} RIFT_NAT_GRID={grid}: |probability - default grid's| = {d:.3e}")
    assert torch.equal(p[f"{fmt}-grid{grid}", "rounds"], p[fmt, "rounds"])


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_taps_do_not_depend_on_what_the_arena_held(runs, fmt):
    """`edges` with the arena filled with 0xFF ahead of the forward (RIFT_POISON_ARENA=255: every word a NaN) against the plain run: every
    tap bit for bit -- no kernel of the chain reads a row nobody wrote (holes of a tile, padding rows, the tokenizer's window ends)."""
    a = runs(f"{fmt}-poison")[0]["edges"]
    assert all(torch.isfinite(v).all() for v in a.values())
    _identical(a, runs(fmt)[0]["edges"], f"{fmt} RIFT_POISON_ARENA=255")
