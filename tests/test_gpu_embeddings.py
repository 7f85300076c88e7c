"""The Fourier embeddings (fo_w_kernel, fourier_fused_kernel three-sided and single-sided, fourier_layerwise), the ego state token
(ego_fused_kernel, ego_token_layerwise) and the token assembly (token_kernel, static_token_kernel) against the fp64 reference of
tests/embedding_cases.py, on designed batches whose three sides end on 1, 16, 17, 64, 65, 128 and 129 rows, whose one-dimensional side has
an empty, a partial and a second workgroup's second pass, whose sides own different numbers of workgroups, whose headings wrap several
turns, and one batch with static objects.  tests/test_embedding_cases.py proves on the CPU that a missing or misplaced wrap, swapped
halves, a dropped rank-1 term, a bias counted once, an overwriting side, shifted tiles or passes, a dropped pass, exchanged limit /
unknown embeddings, a wrong position row, a missing scale or pos_embed and a wrong key mask each move one of these taps by three bars.

What is compared.  fo_pos, fo_speed, fo_static: all rows against the reference on the batch's inputs.  r_emb: on the lines without a
valid point (the PointsEncoder's output is exactly zero there) it IS the reference-line embedding; on the others it is held against
points_cases' encoder reference plus the embedding within the sum of the two bars.  x_ego: eval mode, and train mode with drops on under
two seeds with the key mask restated from uniform01.  x_tokens: against the fp64 sum of the device's OWN taps (nat_out, x_ego, poly_pe,
fo_speed, fo_pos, fo_static) and the embedding tables, within the rounding of its five fp32 additions; where the position embedding is
added in place (static objects, layer-wise) fo_pos is the reference's and its 16-bit bar comes on top.  The exact-fp32 forward runs the
layer-wise scene encoder in place on x_tokens: not compared there.  These taps live in the engine's arena, so a write behind a side's last
row cannot be caught by a pre-filled tensor; the poisoned builds and the bit-for-bit repeat stand in (tests/test_gpu_heads.py pre-fills
the outputs the caller owns).

Bars.  16-bit builds: K[fmt] * E_emu[case, tap, fmt] (embedding_cases.K).  fp32: embedding_cases.FP32_BAR.  Needs a real MI355X:
`pytest -m gpu`."""
import os

import pytest
import torch

from tests import embedding_cases as EC
from tests import points_cases as PC

pytestmark = pytest.mark.gpu

LAYERWISE = {"RIFT_FOURIER_UNFUSED": "1", "RIFT_EGO_UNFUSED": "1", "RIFT_HEADS_UNFUSED": "1"}
BUILDS = {"default": {}, "fo_lds": {"RIFT_FO_W": "0"}, "layerwise": LAYERWISE, "poison-arena": {"RIFT_POISON_ARENA": "255"},
          "poison-lds": {"RIFT_POISON_LDS": "255"}}
ENV_KEYS = sorted({k for env in BUILDS.values() for k in env})
FMTS = ("bf16", "fp16")
SIXTEEN = [(b, f) for b in BUILDS for f in FMTS]
EVERY = SIXTEEN + [("default", "fp32")]                      # (the fp32 forward reads no switch: one build)
EGO_CASES = ("r1", "b15", "l128", "b17", "b33")              # 1, 15, 16, 17 and 33 scenes
PE_FP32_BAR = 1e-4                                           # tests/test_gpu_points_encoder.py: test_fp32_taps


@pytest.fixture(scope="module")
def ffi():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    _ffi.load_library()
    return _ffi


def _three_sided(build, fmt, name):
    """The three-sided launch exists: a 16-bit build with fused embeddings on a batch without static objects."""
    return fmt != "fp32" and build != "layerwise" and EC.SPEC[name][5] == 0


@pytest.fixture(scope="module")
def run(ffi):
    """run(build, fmt | "fp32", case, seed=None) -> {tap: CPU tensor, "again": the taps of a second forward, "launches": {label: count}
    of the first}.  seed: a train forward with drops on under that seed (BatchNorm statistics not updated), x_ego only.  One engine per
    build and format, made on first use with the build's switches in the environment and kept to the end of the module."""
    engines, cache = {}, {}

    def engine(build, fmt):
        if (build, fmt) not in engines:
            env = {} if fmt == "fp32" else BUILDS[build]
            old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
            os.environ.update(env)
            try:
                eng = ffi.Engine("cuda:0", operands="bf16" if fmt == "fp32" else fmt)
            finally:
                for k in ENV_KEYS:
                    os.environ.pop(k, None)
                    if old[k] is not None:
                        os.environ[k] = old[k]
            eng.load_state_dict({k: v.clone() for k, v in EC.case_weights().items()})
            engines[build, fmt] = eng
        return engines[build, fmt]

    def taps(eng, build, fmt, name, seed):
        if seed is not None:
            return {"x_ego": eng.tap("x_ego").view(-1, 128).cpu().clone()}
        s = EC.shapes(name)
        names = ["fo_speed", "r_emb", "x_ego", "nat_out", "poly_pe"] + (["fo_pos"] if _three_sided(build, fmt, name) else []) + \
                (["fo_static"] if s["S"] > 0 else []) + (["x_tokens"] if fmt != "fp32" else [])
        rows = {"fo_speed": s["nP"], "r_emb": s["nL"], "x_ego": s["bs"], "nat_out": s["bs"] * s["A"], "poly_pe": s["nP"], "fo_pos": s["nT"],
                "fo_static": s["nS"], "x_tokens": s["nT"]}
        return {t: eng.tap(t).view(rows[t], 128).cpu().clone() for t in names}

    def get(build, fmt, name, seed=None):
        key = (build, fmt, name, seed)
        if key not in cache:
            eng, data = engine(build, fmt), EC.case(name)
            kw = dict(fp32=fmt == "fp32") if seed is None else dict(fp32=fmt == "fp32", train=True, no_drop=False, bn_update=False, seed=seed)
            eng.prof_enable(True)
            eng.forward(data, **kw)
            torch.cuda.synchronize()
            rep = eng.prof_report()
            eng.prof_enable(False)
            got = taps(eng, build, fmt, name, seed)
            got["launches"] = {k: int(v["count"]) for k, v in rep.items()}
            eng.forward(data, **kw)
            torch.cuda.synchronize()
            got["again"] = taps(eng, build, fmt, name, seed)
            cache[key] = got
        return cache[key]

    yield get
    for eng in engines.values():
        eng.close()


def _launched(r, build, fmt, name):
    """Every run ran the kernels it names."""
    ran, S = r["launches"], EC.SPEC[name][5]
    what = (build, fmt, name, sorted(ran.items()))
    fused = fmt != "fp32" and build != "layerwise"
    if _three_sided(build, fmt, name):
        assert ran.get("fo_w_kernel", 0) == (0 if build == "fo_lds" else 1) and ran.get("fourier_fused_kernel", 0) == (1 if build == "fo_lds" else 0), what
    elif fused:                                     # static objects: speed limits, static shapes, token positions, reference lines, each on its own
        assert ran.get("fourier_fused_kernel", 0) == 4 and "fo_w_kernel" not in ran, what
    else:
        assert ran.get("fourier_feature_kernel", 0) == (4 if S > 0 else 3) and "fo_w_kernel" not in ran and "fourier_fused_kernel" not in ran, what
    assert ran.get("ego_fused_kernel", 0) == (1 if fused else 0) and ("ego_token_kernel" in ran) == (not fused), what
    assert ran.get("token_kernel", 0) == 1 and ran.get("static_token_kernel", 0) == (1 if S > 0 else 0), what


def _rows(got, build, fmt, name):
    """[(tap, |device - fp64|, E_emu part of the bar, rest of the bar)] of the Fourier taps, r_emb and the eval-mode x_ego of a 16-bit run
    (fmt "fp32": E_emu part 0, the rest the fp32 bars)."""
    data = EC.case(name)
    ref = EC.reference64(name)
    E = EC.emu_error(name)
    f32 = fmt == "fp32"
    e = lambda tap: 0.0 if f32 else E[tap, fmt]
    floor = EC.FP32_BAR if f32 else 0.0
    rows = []
    for t in ("fo_pos", "fo_speed", "fo_static", "x_ego"):
        if t in got:
            assert torch.isfinite(got[t]).all(), (build, fmt, name, t)
            rows.append((t, float((got[t].double() - ref[t]).abs().max()), e(t), floor))
    v, nv = EC.line_rows(data)
    assert torch.isfinite(got["r_emb"]).all(), (build, fmt, name, "r_emb")
    if bool(nv.any()):
        rows.append(("fo_ref", float((got["r_emb"].double() - ref["fo_ref"])[nv].abs().max()), e("fo_ref"), floor))
    r_pe, Epe = EC.r_pe_emu_error(name)
    rows.append(("r_emb", float((got["r_emb"].double() - (r_pe + ref["fo_ref"]))[v].abs().max()), e("fo_ref"),
                 floor + (PE_FP32_BAR if f32 else PC.K[fmt] * Epe[fmt])))
    return rows


@pytest.mark.parametrize("build,fmt", SIXTEEN)
def test_sixteen_bit_taps_within_k_operand_rounding_errors(run, build, fmt):
    """fo_pos, fo_speed, fo_static, the reference-line side and x_ego of every case: |device - fp64| <= K[fmt] * E_emu[case, tap, fmt]
    (r_emb on the lines with a valid point: plus the PointsEncoder's bar).  Measured on MI355X, worst device error / E_emu over all taps
    and cases: bf16 1.40 in every fused build (static, fo_static), layer-wise 1.20 (t128, x_ego); fp16 1.26 in every fused build (r17,
    fo_pos), layer-wise 1.18 (t65, x_ego) -- K = 3 for both formats."""
    worst, late = (0.0, None), []
    for name in EC.CASES:
        got = run(build, fmt, name)
        _launched(got, build, fmt, name)
        for t, err, e, rest in _rows(got, build, fmt, name):
            ratio = max(err - rest, 0.0) / e
            print(f"    {build} {fmt} {name} {t}: |device - fp64| {err:.3e}, E_emu {e:.3e}, rest of the bar {rest:.2e}, ratio {ratio:.2f} (K {EC.K[fmt]})")
            worst = max(worst, (ratio, (name, t)))
            if not err <= EC.K[fmt] * e + rest:
                late.append((name, t, err, EC.K[fmt] * e + rest))
    print(f"  {build} {fmt}: worst device error / E_emu = {worst[0]:.2f} at {worst[1]}")
    assert not late, late


def test_fp32_taps(run):
    """The exact-fp32 layer-wise path: fo_speed, fo_static, the reference-line side and x_ego within FP32_BAR of the fp64 reference
    (measured worst 1.218e-6, l129 fo_ref; the bar is twice that rounded up; r_emb on the lines with a valid point: plus the
    PointsEncoder's 1e-4, measured 1.4e-5)."""
    worst, late = (0.0, None), []
    for name in EC.CASES:
        got = run("default", "fp32", name)
        _launched(got, "default", "fp32", name)
        ref = EC.reference64(name)
        for t, err, _, bar in _rows(got, "default", "fp32", name):
            top = float(ref[t if t != "r_emb" else "fo_ref"].abs().max())
            print(f"    fp32 {name} {t}: |device - fp64| {err:.3e} (bar {bar:.1e}, max |tap| {top:.1f})")
            if t != "r_emb":
                worst = max(worst, (err, (name, t)))
            assert EC.FP32_BAR <= 1e-4 * max(1.0, top)
            if not err <= bar:
                late.append((name, t, err, bar))
    print(f"  fp32: worst |device - fp64| = {worst[0]:.3e} at {worst[1]}")
    assert not late, late


@pytest.mark.parametrize("build,fmt", [(b, f) for b, f in EVERY if b in ("default", "layerwise")])
def test_ego_token_under_state_dropout(run, build, fmt):
    """Train mode with drops on, two seeds, 1 / 15 / 16 / 17 / 33 scenes: x_ego against the reference under the key mask restated from
    uniform01 on the ego stream (tokens 3..5, p = 0.75; b33 has a scene with all three masked and one with none under both seeds).  Measured worst device error /
    E_emu: 1.23 (fp16, b15); fp32 5.1e-7."""
    late = []
    for name in EGO_CASES:
        for seed in EC.TRAIN_SEEDS:
            got = run(build, fmt, name, seed)
            assert got["launches"].get("ego_fused_kernel", 0) == (1 if fmt != "fp32" and build != "layerwise" else 0), (build, fmt, name)
            assert torch.isfinite(got["x_ego"]).all(), (build, fmt, name, seed)
            key = (seed, "fp32" if fmt == "fp32" else "16-bit")           # (whose random stream: embedding_cases.EGO_STREAM)
            err = float((got["x_ego"].double() - EC.reference64(name, key)["x_ego"]).abs().max())
            bar = EC.FP32_BAR if fmt == "fp32" else EC.K[fmt] * EC.emu_error(name, key)["x_ego", fmt]
            print(f"    {build} {fmt} {name} seed {seed} x_ego: |device - fp64| {err:.3e} (bar {bar:.2e})" +
                  ("" if fmt == "fp32" else f", ratio {err / EC.emu_error(name, key)['x_ego', fmt]:.2f}"))
            if not err <= bar:
                late.append((name, seed, err, bar))
            assert torch.equal(got["x_ego"], got["again"]["x_ego"]), (build, fmt, name, seed)
    assert not late, late


@pytest.mark.parametrize("build,fmt", SIXTEEN)
def test_tokens_are_the_sum_of_what_the_assembly_reads(run, build, fmt):
    """x_tokens, every row: the fp64 sum of the device's own nat_out (slot order, valid agents), x_ego, poly_pe, fo_speed or the unknown
    embedding, fo_pos, fo_static and the type / on-route / traffic-light tables, within ADDS fp32 roundings of the running sum
    (embedding_cases.sum_bar); where the position embedding is added in place, the reference's fo_pos and its 16-bit bar on top.  Measured: 0.36 of the summation bar at the most
    (5.5e-7 of 1.5e-6: b33)."""
    late = []
    for name in EC.CASES:
        got = run(build, fmt, name)
        t = {k: got[k] for k in ("nat_out", "x_ego", "poly_pe", "fo_speed", "fo_pos", "fo_static") if k in got}
        extra = 0.0
        if "fo_pos" not in t:
            t["fo_pos"] = EC.reference64(name)["fo_pos"]
            extra = EC.K[fmt] * EC.emu_error(name)["fo_pos", fmt]
        x, mag = EC.assemble64(EC.case(name), EC.case_weights(), t)
        s = EC.shapes(name)
        assert torch.isfinite(got["x_tokens"]).all(), (build, fmt, name)
        err = float((got["x_tokens"].view(s["bs"], s["N"], 128).double() - x).abs().max())
        bar = EC.sum_bar(mag) + extra
        print(f"    {build} {fmt} {name} x_tokens: |device - fp64 sum of its taps| {err:.3e} (bar {bar:.2e}; summation {EC.sum_bar(mag):.2e})")
        if not err <= bar:
            late.append((name, err, bar))
    assert not late, late


@pytest.mark.parametrize("build,fmt", EVERY)
def test_second_forward_is_bit_identical(run, build, fmt):
    for name in EC.CASES:
        got = run(build, fmt, name)
        for t, v in got["again"].items():
            if t == "nat_out":
                continue                            # (rows of padded agents are read by nobody: tests/test_gpu_history_encoder.py)
            assert torch.equal(v, got[t]), f"{build} {fmt} {name} {t}: {int((v != got[t]).sum())} words differ between two forwards"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("build", ("poison-arena", "poison-lds"))
def test_taps_do_not_depend_on_what_memory_held(run, build, fmt):
    """The arena (every word a NaN) or every CU's LDS filled with 0xFF ahead of the forward: every tap finite and bit for bit the plain
    run's -- the rows behind a side's last one, the empty second pass and the weight ring's other slot are read by nobody."""
    for name in EC.CASES:
        a, b = run(build, fmt, name), run("default", fmt, name)
        for t in ("fo_pos", "fo_speed", "fo_static", "r_emb", "x_ego", "poly_pe", "x_tokens"):
            if t in b:
                assert torch.isfinite(a[t]).all(), (build, fmt, name, t)
                assert torch.equal(a[t], b[t]), f"{build} {fmt} {name} {t}: {int((a[t] != b[t]).sum())} words differ from the plain run"
