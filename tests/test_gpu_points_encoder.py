"""The two PointsEncoders -- pass A (pe_stats1_kernel), the reference-line packing (pe_pack_body), the live-round list (pe_live_body), pass B
(pe_w_kernel / pe_mid_kernel), the fp16 hand-over of g, pass C (pe_out_kernel) and the layer-wise path -- against the fp64 reference of
tests/points_cases.py at what the passes hand to one another: pe_s1 / t1 / s2 / t2 (the folded BatchNorms), pe_gp (pe_mid_kernel only:
pe_w_kernel keeps it in registers; the layer-wise path's is without its bias), pe_g (fp16 words; fp32 layer-wise), poly_pe / r_pe (out),
and the running statistics after a train forward; on the designed cases `ends`, `rounds`, `segments_long` and `segments_mixed`, eval and
train mode.  tests/test_points_cases.py proves on the CPU that a missing or invented zero row, a dropped tile, a leaking neighbour, a
neighbour's gp, wrong statistics rows, swapped variances, the wrong mode or a swapped concat moves one of these taps by three bars.

Bars.  16-bit builds: K[fmt] * E_emu[case, mode, tap, fmt] (+ 8 ulp of fp32 for what an fp32 finalize writes: points_cases.FP32_ULPS).
fp32: 1e-4.  out is compared on ALL groups (a group without a valid point: exactly 0), g on the valid rows, gp on the groups with a valid
point.  r_pe shares its buffer with r_emb; the case weights zero the position embedding that is added into it (points_cases.case_weights).
Needs a real MI355X: `pytest -m gpu`."""
import os

import pytest
import torch

from tests import points_cases as PC

pytestmark = pytest.mark.gpu

NAMES = tuple(PC.CASES)
MODES = (False, True)
# variant -> (environment of the context, modes, taps offered besides out)
CORE = ("s1", "t1", "s2", "t2", "g")
VARIANTS = {
    "default": ({}, MODES, CORE),
    "nopack": ({"RIFT_PE_PACK": "0"}, MODES, CORE),
    "nolive": ({"RIFT_PE_LIVE": "0"}, (True,), CORE),
    "mid": ({"RIFT_PE_W": "0"}, MODES, CORE + ("gp",)),
    "layerwise": ({"RIFT_PE_UNFUSED": "1"}, MODES, CORE),
    "grid1": ({"RIFT_NAT_GRID": "1"}, MODES, CORE),
    "grid2": ({"RIFT_NAT_GRID": "2"}, MODES, CORE),
    "poison-arena": ({"RIFT_POISON_ARENA": "255"}, MODES, CORE),
    "poison-lds": ({"RIFT_POISON_LDS": "255"}, MODES, CORE),
}
FMTS = ("bf16", "fp16")
BN = {1: "first_mlp.1", 2: "second_mlp.1"}
STAT_KEYS = [PC.PE[e] + BN[i] + s for e in PC.PE for i in BN for s in (".running_mean", ".running_var", ".num_batches_tracked")]
ENV_KEYS = sorted({k for env, _, _ in VARIANTS.values() for k in env})


@pytest.fixture(scope="module")
def ffi():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    _ffi.load_library()
    return _ffi


@pytest.fixture(scope="module")
def runs(ffi):
    """(variant, fmt | "fp32", case, train) -> {tap_e: CPU tensor as points_cases.compared lays it out, "pack_hdr" / "pack_tab" /
    "live_hdr" / "live_a" / "live_b": ints where the build has them, "kernels": the launches of a second, profiled forward, "stats": the
    BatchNorm buffers after the forward}.  One engine per build, made on first use with the build's switches in the environment (the
    context reads them when it is created) and kept to the end of the module; the BatchNorm buffers are put back after every forward, so
    every forward starts from a fresh copy of the weights' statistics."""
    engines, cache = {}, {}

    def engine(variant, fmt):
        if (variant, fmt) not in engines:
            env = {} if fmt == "fp32" else VARIANTS[variant][0]
            old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
            os.environ.update(env)
            try:
                eng = ffi.Engine("cuda:0", operands="bf16" if fmt == "fp32" else fmt)
            finally:
                for k in ENV_KEYS:
                    os.environ.pop(k, None)
                    if old[k] is not None:
                        os.environ[k] = old[k]
            params = eng.load_state_dict({k: v.clone() for k, v in PC.case_weights().items()})
            engines[variant, fmt] = (eng, params)
        return engines[variant, fmt]

    def get(variant, fmt, name, train):
        key = (variant, fmt, name, bool(train))
        if key in cache:
            return cache[key]
        eng, params = engine(variant, fmt)
        sd, data = PC.case_weights(), PC.case(name)
        fp32 = fmt == "fp32"
        fused16 = not fp32 and variant != "layerwise"
        offered = CORE if fp32 else VARIANTS[variant][2]
        feats = PC.features(data)
        eng.forward(data, train=train, no_drop=True, bn_update=True, fp32=fp32)
        eng.check_finite()
        torch.cuda.synchronize()
        raw = {}
        for e, (x, mask) in feats.items():
            G, n = mask.shape
            raw[e] = {}
            for t in offered:
                v = eng.tap(f"pe_{t}_{e}").cpu()
                if t == "g":
                    v = (v.view(torch.float16).float() if fused16 else v).view(G, n, 256)
                elif t == "gp":
                    v = v.view(G, 256)
                raw[e][t] = v
            raw[e]["out"] = eng.tap("poly_pe" if e == "a" else "r_pe").cpu().view(G, 128)
        got = {k: v.clone() for k, v in PC.compared(raw, data).items()}
        ints = lambda nm: eng.tap(nm).cpu().view(torch.int32).tolist()
        if fused16 and variant not in ("mid", "nopack"):          # the table exists where pass B is pe_w_kernel on packed rounds
            got["pack_hdr"], got["pack_tab"] = ints("pe_pack_hdr"), ints("pe_pack_tab")
        if fused16 and variant != "mid" and (variant != "nopack" or train):       # the header: packed rounds or a live list
            got["live_hdr"] = ints("pe_live_hdr")
            if train and variant != "nolive":
                got["live_a"] = ints("pe_live_a")
                if variant == "nopack":
                    got["live_b"] = ints("pe_live_b")
        got["stats"] = {k: params[k].cpu().clone() for k in STAT_KEYS}
        for k in STAT_KEYS:                                # a fresh copy of the statistics for the next forward
            params[k].copy_(sd[k])
        eng.prof_enable(True)
        eng.forward(data, train=train, no_drop=True, bn_update=False, fp32=fp32)
        torch.cuda.synchronize()
        got["kernels"] = set(eng.prof_report())
        eng.prof_enable(False)
        cache[key] = got
        return got

    yield get
    for eng, _ in engines.values():
        eng.close()


def _ratios(got, name, train, fmt, what):
    """[(ratio to the bar's E_emu part, err, bar, tap)] of every compared tap; prints each."""
    ref = PC.compared(PC.reference64(name, train), PC.case(name))
    E = PC.emu_error(name, train)
    rows = []
    for tap, r in ref.items():
        if tap not in got:
            continue
        assert torch.isfinite(got[tap]).all(), (what, name, train, tap)
        err = float((got[tap].double() - r).abs().max())
        fl = PC.fp32_floor(name, train, tap)
        e = E[tap, fmt]
        ratio = max(err - fl, 0.0) / e if e > 0 else 0.0
        print(f"    {what} {name} {'train' if train else 'eval'} {tap}: |device - fp64| {err:.3e}, E_emu {e:.3e}, fp32 floor {fl:.1e}, ratio {ratio:.2f} "
              f"(K {PC.K[fmt]})")
        rows.append((ratio, err, PC.bar(name, train, tap, fmt), tap))
    return rows


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("variant", tuple(VARIANTS))
def test_sixteen_bit_taps_within_k_operand_rounding_errors(runs, variant, fmt, name):
    """Every tap the build offers, eval and train mode: |device - fp64| <= K[fmt] * E_emu[case, mode, tap, fmt]; the running statistics
    after the train forward within the same bar, num_batches_tracked exact; after the eval forward all of them bit-unchanged.
    Measured on MI355X, worst device error / E_emu over all taps, cases and modes: bf16 1.13 and fp16 1.79 (RIFT_NAT_GRID=1, segments_long,
    train, t2_b: one workgroup adds the statistics of all 51 rounds in fp32); every other build bf16 1.08 at the most (1.07: rounds, eval,
    out_a) and fp16 1.49 (segments_long, train, g_a: the fp16 hand-over of g rounds once more at the operand's own precision); layer-wise
    1.01 / 1.02 -- K = 3 (bf16) and 4 (fp16); every figure in profiles/NOTES_r20.md."""
    sd = PC.case_weights()
    late, worst = [], (0.0, None)
    for train in VARIANTS[variant][1]:
        got = runs(variant, fmt, name, train)
        rows = _ratios(got, name, train, fmt, f"{variant} {fmt}")
        ref = PC.reference64(name, train)
        E = PC.emu_error(name, train)
        for e in PC.PE:
            for i in BN:
                p = PC.PE[e] + BN[i]
                st = got["stats"]
                if not train:
                    assert all(torch.equal(st[p + s], sd[p + s]) for s in (".running_mean", ".running_var", ".num_batches_tracked")), (p, "eval")
                    continue
                assert int(st[p + ".num_batches_tracked"]) == ref[e][f"nbt{i}"] == int(sd[p + ".num_batches_tracked"]) + 1
                for s, tap in ((".running_mean", f"rm{i}_{e}"), (".running_var", f"rv{i}_{e}")):
                    err = float((st[p + s].double() - ref[e][tap[:3]]).abs().max())
                    fl = PC.fp32_floor(name, train, tap)
                    ratio = max(err - fl, 0.0) / E[tap, fmt]
                    print(f"    {variant} {fmt} {name} train {tap}: |device - fp64| {err:.3e}, E_emu {E[tap, fmt]:.3e}, ratio {ratio:.2f}")
                    rows.append((ratio, err, PC.bar(name, train, tap, fmt), tap))
        for ratio, err, bar, tap in rows:
            worst = max(worst, (ratio, (name, train, tap)), key=lambda w: w[0])
            if not err <= bar:
                late.append((name, train, tap, err, bar))
    print(f"  {variant} {fmt} {name}: worst device error / E_emu = {worst[0]:.2f} at {worst[1]}")
    assert not late, late


@pytest.mark.parametrize("name", NAMES)
def test_fp32_taps(runs, name):
    """The exact-fp32 layer-wise path: every offered tap and the new running statistics within 1e-4 of the fp64 reference (measured:
    6.8e-5 at the worst, t2_b of `rounds` in train mode)."""
    late = []
    for train in MODES:
        got = runs("default", "fp32", name, train)
        ref = PC.compared(PC.reference64(name, train), PC.case(name))
        for tap, r in ref.items():
            if tap in got:
                v = got[tap]
            elif tap[:2] in ("rm", "rv"):
                e, i = tap[-1], int(tap[2])
                v = got["stats"][PC.PE[e] + BN[i] + (".running_mean" if tap[:2] == "rm" else ".running_var")]
            else:
                continue
            err = float((v.double() - r).abs().max())
            print(f"    fp32 {name} {'train' if train else 'eval'} {tap}: |device - fp64| {err:.3e}")
            if not err <= 1e-4:
                late.append((name, train, tap, err))
    assert not late, late


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", FMTS)
def test_pack_table_and_live_lists(runs, fmt, name):
    """The packed-round table of both modes (eval: pe_pack_lines_kernel, train: the extra block of pass A) holds points_cases'
    invariants, within its allocation; the live list of the polygons (and of the lines without packing) is the rounds that hold a valid
    point; the header's workgroup split sums to the grid."""
    feats = PC.features(PC.case(name))
    tiles = PC.tiles_per_line(feats["b"][1])
    la, lb = PC.live_rounds(feats["a"][1], "a"), PC.live_rounds(feats["b"][1], "b")
    ra, rb = (feats["a"][1].shape[0] + 11) // 12, (feats["b"][1].shape[0] + 1) // 2
    for train in MODES:
        got = runs("default", fmt, name, train)
        assert len(got["pack_tab"]) == 32 * PC.pack_max_rounds(len(tiles))
        n = PC.check_pack_table(tiles, got["pack_hdr"], got["pack_tab"])
        print(f"    {fmt} {name} {'train' if train else 'eval'}: {n} packed rounds (table: {PC.pack_max_rounds(len(tiles))}, two-line rounds: {rb}), "
              f"live header {got['live_hdr']}")
        hdr = got["live_hdr"]
        assert hdr[1] == n and hdr[2] + hdr[3] == min(256, ra + rb) and hdr[2] >= 1 and hdr[3] >= 1
        if train:
            assert hdr[0] == len(la) and got["live_a"][:len(la)] == la
        else:
            assert hdr[0] == ra
    for variant, grid in (("grid1", 2), ("grid2", 2)):
        hdr = runs(variant, fmt, name, True)["live_hdr"]
        assert hdr[2] + hdr[3] == grid and hdr[0] == len(la)
    got = runs("nopack", fmt, name, True)
    assert got["live_hdr"][:2] == [len(la), len(lb)] and got["live_a"][:len(la)] == la and got["live_b"][:len(lb)] == lb
    if name == "rounds":
        assert la == [0, 2, 3]


def _identical(a, b, what, taps=None):
    for t in (taps or [k for k in a if k.endswith(("_a", "_b")) and not k.startswith("live")]):
        assert t in b, (what, t)
        assert torch.equal(a[t], b[t]), f"{what}: tap {t} differs in {int((a[t] != b[t]).sum())} words"


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", FMTS)
def test_eval_output_does_not_depend_on_the_round_a_row_sits_in(runs, fmt, name):
    """Eval mode: packed or two-line rounds, one, two or all workgroups -- poly_pe, r_pe and every other tap bit for bit (a row's
    arithmetic does not depend on its tile or round, a max has no order)."""
    base = runs("default", fmt, name, False)
    for variant in ("nopack", "grid1", "grid2"):
        _identical(runs(variant, fmt, name, False), base, f"{fmt} {name} {variant}")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("variant", ("poison-arena", "poison-lds"))
def test_taps_do_not_depend_on_what_memory_held(runs, variant, fmt, name):
    """The arena (every word a NaN) or every CU's LDS filled with 0xFF ahead of the forward: every compared tap finite and bit for bit the
    plain run's, eval and train -- g rows of dropped tiles, rows 120..127 of the last line, dead rounds and the holes of a pass-A tile
    are read by nobody."""
    for train in MODES:
        a = runs(variant, fmt, name, train)
        for k, v in a.items():
            if k.endswith(("_a", "_b")) and torch.is_tensor(v):
                assert torch.isfinite(v).all(), (variant, name, train, k)
        _identical(a, runs("default", fmt, name, train), f"{fmt} {name} {variant} {'train' if train else 'eval'}")
        for k in STAT_KEYS:
            assert torch.equal(a["stats"][k], runs("default", fmt, name, train)["stats"][k]), k


def _sum_bound(name, e, i):
    """What summing a channel's values and squares in fp32, in any order the kernels use, can move s_i / t_i by.  No fp32 chain is longer
    than D = min(n, 240 + tiles) terms: a workgroup adds the rows of a round (at most 240) or tile and then one total per round or tile
    it walks (at most all ceil(rows / 120) of them); the partials of the workgroups are added in fp64.  The sums are then off by at most
    D u sum |x| (u = 2^-24), so the mean by dm = D u sqrt(E x^2), E x^2 by dq = D u E x^2, the variance by dq + 2 |m| dm;
    s = w (var + eps)^-1/2 and t = b - m s follow.  -> (ds, dt), per channel maxima, for TWO runs (factor 2)."""
    ref = PC.reference64(name, True, keep_stats=True)[e]
    mask = PC.features(PC.case(name))[e][1]
    n = min(int(mask.sum()), 240 + (mask.numel() + 119) // 120)
    m, var, s = ref[f"_mean{i}"], ref[f"_var{i}"], ref[f"s{i}"]
    u = 2.0 ** -24
    q = var + m * m
    dm, dq = n * u * q.sqrt(), n * u * q
    dvar = dq + 2 * m.abs() * dm
    ds = s.abs() * dvar / (2 * (var + PC.BN_EPS))
    dt = s.abs() * dm + m.abs() * ds
    return 2 * float(ds.max()), 2 * float(dt.max())


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", FMTS)
def test_train_mode_across_work_splits(runs, fmt, name):
    """Train mode with one, two or all workgroups, without the live list, without packing: s1 / t1 / s2 / t2 agree within the fp32
    summation error of the statistics' own sums (_sum_bound; measured: at most 1 % of it, and at most 1.2 E_emu -- t2_b of `segments_long`
    with one workgroup walking all 51 rounds); out within the 16-bit bar of each run (test_sixteen_bit_taps_...), not bit for bit."""
    base = runs("default", fmt, name, True)
    E = PC.emu_error(name, True)
    for variant in ("grid1", "grid2", "nolive", "nopack"):
        got = runs(variant, fmt, name, True)
        for e in PC.PE:
            for i in BN:
                ds, dt = _sum_bound(name, e, i)
                for t, tol in ((f"s{i}_{e}", ds), (f"t{i}_{e}", dt)):
                    d = float((got[t] - base[t]).abs().max())
                    print(f"    {fmt} {name} {variant} {t}: |split - default| {d:.3e} (summation bound {tol:.3e}; "
                          f"{d / E[t, fmt]:.4f} E_emu)")
                    assert d <= tol, (variant, t, d, tol)
            d = float((got[f"out_{e}"] - base[f"out_{e}"]).abs().max())
            print(f"    {fmt} {name} {variant} out_{e}: |split - default| {d:.3e}")
            assert d <= 2 * PC.bar(name, True, f"out_{e}", fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_each_build_runs_the_kernels_it_names(runs, fmt):
    for train in MODES:
        k = runs("default", fmt, "ends", train)["kernels"]
        assert "pe_w_kernel" in k and "pe_mid_kernel" not in k and "pe_out_kernel" in k
        assert ("pe_pack_lines_kernel" in k) == (not train) and ("pe_stats1_kernel" in k) == train
        k = runs("nopack", fmt, "ends", train)["kernels"]
        assert "pe_w_kernel" in k and "pe_pack_lines_kernel" not in k
        k = runs("mid", fmt, "ends", train)["kernels"]
        assert "pe_mid_kernel" in k and "pe_w_kernel" not in k and "pe_pack_lines_kernel" not in k and ("pe_stats1_kernel" in k) == train
        k = runs("layerwise", fmt, "ends", train)["kernels"]
        assert "masked_maxpool_kernel" in k and not {"pe_w_kernel", "pe_mid_kernel", "pe_out_kernel", "pe_stats1_kernel"} & k
