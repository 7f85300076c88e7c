"""The planning decoder -- q_proj, the four DecoderLayers (dec_w_kernel in its four compiled variants, or the layer-wise launches) on the K | V^T
image of each of its four producers, cat_x_proj -- against the fp64 reference of tests/decoder_cases.py at every layer boundary the engine
can tap (q0, dec1, dec3, q_final), on the designed batches std80, std96, mid112, mid128, dense_r9 and dense_192, eval forward only (dropout:
tests/test_gpu_dropstats.py).  tests/test_decoder_cases.py proves on the CPU that a wrong mask row, key-tile edge, m_pos term, line tiling or
concatenation order moves one of these taps by three bars.

The reference is fed the DEVICE's own r_emb and enc_out taps, so device error and E_emu measure the decoder alone; a gate holds those two
taps against the oracle's within the suite's existing bars.  q0 and dec3 tap the same buffer: q0 is the `dec3` tap of a context with
RIFT_DEC_LAYERS=0, dec1 that of one with RIFT_DEC_LAYERS=2 (tests of such a context read taps only).

Bars.  16-bit builds: K[fmt] * E_emu[case, tap, fmt] -- E_emu = what rounding both operands of every contraction to the format costs the fp64
reference ON THE SAME INPUTS, K one factor per format for all taps and cases (decoder_cases.K; measured ratios in profiles/NOTES_r17.md).
fp32: decoder_cases.FP32_BAR.  Needs a real MI355X: `pytest -m gpu`."""
import os

import pytest
import torch

from tests import decoder_cases as DC
from tests import helpers as H

pytestmark = pytest.mark.gpu

MID = ("mid112", "mid128")
POISONED = ("std80", "mid112")
# build -> (operand format, environment of the context, cases)
BUILDS = {}
for _f in ("bf16", "fp16"):
    BUILDS.update({
        _f: (_f, {}, DC.CASES),
        f"{_f}-L0": (_f, {"RIFT_DEC_LAYERS": "0"}, DC.CASES),
        f"{_f}-L2": (_f, {"RIFT_DEC_LAYERS": "2"}, DC.CASES),
        f"{_f}-L22": (_f, {"RIFT_DEC_LAYERS": "22"}, DC.CASES),
        f"{_f}-layerwise": (_f, {"RIFT_DEC_UNFUSED": "1"}, DC.CASES),
        f"{_f}-layerwise-L2": (_f, {"RIFT_DEC_UNFUSED": "1", "RIFT_DEC_LAYERS": "2"}, DC.CASES),
        f"{_f}-kvfrag": (_f, {"RIFT_ENC_UNFUSED": "1"}, ("dense_r9",)),
        f"{_f}-kvfrag-L2": (_f, {"RIFT_ENC_UNFUSED": "1", "RIFT_DEC_LAYERS": "2"}, ("dense_r9",)),
        f"{_f}-dbg32": (_f, {"RIFT_DEC_DBG": "32"}, MID),
        f"{_f}-dbg32-L2": (_f, {"RIFT_DEC_DBG": "32", "RIFT_DEC_LAYERS": "2"}, MID),
        f"{_f}-poison": (_f, {"RIFT_POISON_ARENA": "255", "RIFT_POISON_LDS": "255"}, POISONED),
        f"{_f}-poison-L2": (_f, {"RIFT_POISON_ARENA": "255", "RIFT_POISON_LDS": "255", "RIFT_DEC_LAYERS": "2"}, POISONED),
    })
# the existing bars of the taps in front of the decoder: enc_out of valid tokens (test_gpu_parity.py: test_forward_eval), r_emb as a share of
# its largest value (test_gpu_parity.py: test_fused_fourier_embedding_matches_layerwise_path; fp32: test_forward_eval's)
ENC_BAR = {"fp32": 1e-4, "bf16": 4e-2, "fp16": 8e-3}
REMB_BAR = {"fp32": 1e-4, "bf16": 3e-2, "fp16": 3e-2}


@pytest.fixture(scope="module")
def ffi():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    _ffi.load_library()
    return _ffi


@pytest.fixture(scope="module")
def run(ffi):
    """run(build, case, mode) -> {r_emb (bs, R, 128), enc_out (bs, N, 128), dec (bs, R, 12, 128): the `dec3` tap, q_final, probability,
    launches {label: count}} as CPU tensors.  mode: "traj" (need_traj=True), "prob" (need_traj=False) or "fp32" (the exact-fp32 forward with
    the trajectory heads).  One engine per build, made on first use with the build's switches in the environment (the context reads them
    when it is created); every forward runs once."""
    engines, cache = {}, {}

    def engine(build):
        if build not in engines:
            fmt, env, _ = BUILDS[build]
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                eng = ffi.Engine("cuda:0", operands=fmt)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            eng.load_state_dict({k: v.clone() for k, v in DC.case_weights().items()})
            engines[build] = eng
        return engines[build]

    def get(build, name, mode="traj"):
        key = (build, name, mode)
        if key not in cache:
            assert name in BUILDS[build][2], key
            eng, data = engine(build), DC.case(name)
            kpm, r_kpm = DC.paddings(data)
            (bs, N), R = kpm.shape, r_kpm.shape[1]
            eng.prof_enable(True)
            out = eng.forward(data, need_traj=mode != "prob", fp32=mode == "fp32")
            torch.cuda.synchronize()
            rep = eng.prof_report()
            eng.prof_enable(False)
            cache[key] = {"r_emb": eng.tap("r_emb").view(bs, R, 128).cpu(), "enc_out": eng.tap("enc_out").view(bs, N, 128).cpu(),
                          "dec": eng.tap("dec3").view(bs, R, DC.M, 128).cpu(), "q_final": eng.tap("q_final").view(bs, R, DC.M, 128).cpu(),
                          "probability": out["probability"].cpu().clone(), "launches": {k: int(v["count"]) for k, v in rep.items()}}
        return cache[key]

    yield get
    for eng in engines.values():
        eng.close()


_refs = {}


def _reference(name, r):
    """(fp64 taps, E_emu) of the reference on a run's own r_emb / enc_out; shared by the runs whose inputs are bit for bit the same."""
    key = (name, hash(r["r_emb"].numpy().tobytes()), hash(r["enc_out"].numpy().tobytes()))
    if key not in _refs:
        kpm, r_kpm = DC.paddings(DC.case(name))
        assert torch.isfinite(r["r_emb"]).all() and torch.isfinite(r["enc_out"]).all(), name
        ref = DC.reference64(DC.case_weights(), r["r_emb"], r["enc_out"], kpm, r_kpm)
        _refs[key] = (ref, DC.emu_error(DC.case_weights(), r["r_emb"], r["enc_out"], kpm, r_kpm, ref))
    return _refs[key]


def _same_inputs(a, b, what):
    assert torch.equal(a["r_emb"], b["r_emb"]) and torch.equal(a["enc_out"], b["enc_out"]), f"{what}: r_emb / enc_out differ"


def _taps(run, build, name, mode="traj"):
    """{tap: device tensor} of a build and the run the reference inputs come from: dec3 and q_final of the build's own context, dec1 of its
    RIFT_DEC_LAYERS=2 twin, q0 of its RIFT_DEC_LAYERS=0 twin (where the build has them); the twins' r_emb / enc_out are the build's bit for bit."""
    base = run(build, name, mode)
    got = {"dec3": base["dec"], "q_final": base["q_final"]}
    fmt_build = build if mode != "fp32" else "bf16"
    for tap, twin in (("q0", f"{fmt_build}-L0"), ("dec1", f"{fmt_build}-L2")):
        if twin in BUILDS and name in BUILDS[twin][2]:
            t = run(twin, name, mode)
            _same_inputs(t, base, f"{twin} {name} {mode}")
            got[tap] = t["dec"]
    return got, base


def _launched(r, build, name):
    """Every case ran the kernels it names."""
    ran, env = r["launches"], BUILDS[build][1]
    if "RIFT_DEC_UNFUSED" in env:
        assert "dec_w_kernel" not in ran and "dec_kv_frag_kernel" not in ran, (build, name, sorted(ran))
    elif "RIFT_ENC_UNFUSED" in env:
        assert ran.get("dec_kv_frag_kernel") == 1 and ran.get("dec_w_kernel") == 1, (build, name, sorted(ran))
        assert not any(k.startswith("enc_") for k in ran), (build, name, sorted(ran))
    else:
        for k in DC.KERNELS[name]:
            assert ran.get(k) == 1, (build, name, k, sorted(ran))
        assert ("dec_kv_frag_kernel" in ran) == ("dec_kv_frag_kernel" in DC.KERNELS[name]), (build, name)
        assert len([k for k in ran if k.startswith("enc_")]) == 1, (build, name, sorted(ran))


@pytest.mark.parametrize("build", ["bf16", "fp16", "bf16-layerwise", "fp16-layerwise", "bf16-kvfrag", "fp16-kvfrag", "fp32"])
def test_decoder_inputs_are_the_oracles_within_the_existing_bars(run, build):
    """The gate: the device's r_emb (ALL rows -- the r2r quirk makes padded lines keys) and enc_out (valid tokens, and the ego slot that
    cat_x_proj reads even where it is padded) against the oracle's under the same weights, within the bars the suite already holds them to.
    Garbage in front of the decoder is reported here, not as a decoder error."""
    mode, b = ("fp32", "bf16") if build == "fp32" else ("traj", build)
    fmt = "fp32" if build == "fp32" else BUILDS[b][0]
    late = []
    for name in BUILDS[b][2]:
        r = run(b, name, mode)
        want_r, want_e, kpm, r_kpm, _ = DC.oracle_inputs(name)
        read = ~kpm
        read[:, 0] = True
        e_r = float((r["r_emb"].double() - want_r).abs().max())
        e_pad = float((r["r_emb"].double() - want_r)[r_kpm].abs().max()) if bool(r_kpm.any()) else 0.0
        e_e = float((r["enc_out"].double() - want_e)[read].abs().max())
        bar_r = REMB_BAR[fmt] * max(1.0, float(want_r.abs().max()))
        print(f"    {build} {name}: |r_emb - oracle| {e_r:.3e} (padded lines {e_pad:.3e}; bar {bar_r:.1e}), |enc_out - oracle| {e_e:.3e} (bar {ENC_BAR[fmt]:.0e})")
        assert torch.isfinite(r["r_emb"]).all() and torch.isfinite(r["enc_out"]).all(), (build, name)
        if not (e_r <= bar_r and e_e <= ENC_BAR[fmt]):
            late.append((name, e_r, bar_r, e_e, ENC_BAR[fmt]))
    assert not late, late


@pytest.mark.parametrize("build", ["bf16", "fp16", "bf16-layerwise", "fp16-layerwise", "bf16-kvfrag", "fp16-kvfrag"])
def test_sixteen_bit_taps_within_k_operand_rounding_errors(run, build):
    """Every tap the build offers, every case of the build, ALL rows (need_traj=True: the rows of padded lines are outputs):
    |device - reference64(device inputs)| <= K[fmt] * E_emu[case, tap, fmt].  Measured on MI355X, worst device error / E_emu over all taps and
    cases: bf16 fused 1.39
    (dense_r9, dec1), layer-wise 1.17, kvfrag 1.12; fp16 fused 1.16 (mid128, q_final), layer-wise 1.13, kvfrag 1.16 -- K = 3 for both formats; every
    figure in profiles/NOTES_r17.md."""
    fmt = BUILDS[build][0]
    worst, late = (0.0, None), []
    for name in BUILDS[build][2]:
        got, base = _taps(run, build, name)
        _launched(base, build, name)
        ref, E = _reference(name, base)
        for t in DC.TAPS:
            if t not in got:
                continue
            assert torch.isfinite(got[t]).all(), (build, name, t)
            err = float((got[t].double() - ref[t]).abs().max())
            ratio = err / E[t, fmt]
            print(f"    {build} {name} {t}: |device - fp64| {err:.3e}, E_emu {E[t, fmt]:.3e}, ratio {ratio:.2f} (K {DC.K[fmt]})")
            worst = max(worst, (ratio, (name, t)))
            if err > DC.K[fmt] * E[t, fmt]:
                late.append((name, t, err, DC.K[fmt] * E[t, fmt]))
    print(f"  {build}: worst device error / E_emu = {worst[0]:.2f} at {worst[1]}")
    assert not late, late


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_forward_without_trajectory_heads(run, fmt):
    """need_traj=False (DecWP::prob_only): the rows of valid lines within the same bars and BIT-IDENTICAL to the forward with the trajectory
    heads; the rows of padded lines leave the last layer as exact zeros (dec_w.h: their tiles skip the last layer's reference-line tiling)."""
    late = []
    for name in DC.CASES:
        a, b = run(fmt, name, "prob"), run(fmt, name, "traj")
        _launched(a, fmt, name)
        _same_inputs(a, b, f"{fmt} {name} prob / traj")
        r_kpm = DC.paddings(DC.case(name))[1]
        ref, E = _reference(name, a)
        assert bool(r_kpm.any())
        assert float(a["dec"][r_kpm].abs().max()) == 0.0, (fmt, name, "rows of padded lines behind the last layer")
        for t, g in (("dec3", a["dec"]), ("q_final", a["q_final"])):
            err = float((g.double() - ref[t])[~r_kpm].abs().max())
            print(f"    {fmt} {name} {t} (valid lines, no trajectory heads): |device - fp64| {err:.3e}, ratio {err / E[t, fmt]:.2f}")
            if err > DC.K[fmt] * E[t, fmt]:
                late.append((name, t, err, DC.K[fmt] * E[t, fmt]))
        assert torch.equal(a["dec"][~r_kpm], b["dec"][~r_kpm]) and torch.equal(a["q_final"][~r_kpm], b["q_final"][~r_kpm]), (fmt, name)
        assert torch.equal(a["probability"], b["probability"]), (fmt, name)
    assert not late, late


def test_fp32_taps(run):
    """The exact-fp32 layer-wise path: q0, dec1, dec3 and q_final of all rows within FP32_BAR of the fp64 reference on its own inputs
    (measured worst 1.09e-5, mid128 dec3; the bar is four times that rounded up, and under 1e-4 max(1, max |tap|): profiles/NOTES_r17.md)."""
    worst, late = (0.0, None), []
    for name in DC.CASES:
        got, base = _taps(run, "bf16", name, "fp32")
        assert "dec_w_kernel" not in base["launches"], name
        ref, _ = _reference(name, base)
        for t in DC.TAPS:
            err = float((got[t].double() - ref[t]).abs().max())
            print(f"    fp32 {name} {t}: |device - fp64| {err:.3e} (max |tap| {float(ref[t].abs().max()):.1f})")
            worst = max(worst, (err, (name, t)))
            assert DC.FP32_BAR <= 1e-4 * max(1.0, float(ref[t].abs().max()))
            if not err <= DC.FP32_BAR:
                late.append((name, t, err))
    print(f"  fp32: worst |device - fp64| = {worst[0]:.3e} at {worst[1]}")
    assert not late, late


def _identical(a, b, what, rows=None):
    for t in ("r_emb", "enc_out", "dec", "q_final", "probability"):
        x, y = (a[t], b[t]) if rows is None or t in ("r_emb", "enc_out") else (a[t][rows], b[t][rows])
        assert torch.isfinite(x).all(), f"{what}: tap {t}"
        assert torch.equal(x, y), f"{what}: tap {t} differs in {int((x != y).sum())} words"


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_dense_variant_in_place_of_the_eight_key_tile_kernel_is_bit_identical(run, fmt):
    """mid112 (compacted keys) and mid128 (slot order) with RIFT_DEC_DBG=32 (the dense-traffic variant, rounds of key tiles out of the same
    image) against the eight-key-tile kernel: dec1, dec3, q_final and the logits bit for bit."""
    for name in MID:
        _identical(run(f"{fmt}-dbg32", name), run(fmt, name), f"{fmt} {name} RIFT_DEC_DBG=32")
        _identical(run(f"{fmt}-dbg32-L2", name), run(f"{fmt}-L2", name), f"{fmt} {name} RIFT_DEC_DBG=32, dec1")


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_taps_do_not_depend_on_what_arena_and_lds_held(run, fmt):
    """std80 and mid112 with the arena and every CU's LDS filled with 0xFF ahead of the launches (every word a NaN) against the plain run:
    every tap bit for bit -- no kernel of the chain reads a key tile, a mask entry or a row nobody wrote."""
    for name in POISONED:
        _identical(run(f"{fmt}-poison", name), run(fmt, name), f"{fmt} {name} poison")
        _identical(run(f"{fmt}-poison-L2", name), run(f"{fmt}-L2", name), f"{fmt} {name} poison, dec1")


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_two_launches_of_two_layers_are_one_launch_of_four(run, fmt):
    """RIFT_DEC_LAYERS=22: layers [0, 2) and [2, 4) as two launches, the rows travelling through the query array -- every row of every tap
    equals the single launch bit for bit, with and without the trajectory heads."""
    for name in DC.CASES:
        for mode in ("traj", "prob"):
            two, one = run(f"{fmt}-L22", name, mode), run(fmt, name, mode)
            assert two["launches"].get("dec_w_kernel") == 2 and one["launches"].get("dec_w_kernel") == 1, (fmt, name, mode)
            assert {k: v for k, v in two["launches"].items() if k != "dec_w_kernel"} == \
                   {k: v for k, v in one["launches"].items() if k != "dec_w_kernel"}, (fmt, name, mode)
            _identical(two, one, f"{fmt} {name} {mode} RIFT_DEC_LAYERS=22")


# One eval forward of `full` (2 scenes, 84 token slots, R <= 6) with the trajectory heads and without any switch: the launch record of the
# commit before RIFT_DEC_LAYERS existed, measured with that commit's library on MI355X (profiles/NOTES_r17.md).
FULL_LAUNCHES = {"bn_finalize_t_kernel": 2, "dec_w_kernel": 1, "ego_fused_kernel": 1, "ego_heads_kernel": 1, "enc_fused_kernel": 1, "fo_w_kernel": 1,
                 "fpn_tail_kernel": 1, "gemm_bf16_m4n2": 2, "heads3_fused_kernel": 2, "nat_l0w_kernel": 1, "nat_l1w_kernel": 1, "nat_l2w_kernel": 1,
                 "pe_out_kernel": 1, "pe_pack_lines_kernel": 1, "pe_w_kernel": 1, "pi_forward_kernel": 1, "prep_kernel": 1, "q0_fused_kernel": 1,
                 "token_kernel": 1}


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_default_forward_issues_the_launches_it_always_did(ffi, fmt):
    """Without RIFT_DEC_LAYERS the forward records exactly FULL_LAUNCHES; with it, the same record but for the decoder's own launches."""
    data = H.build_batch("full")["cur_pluto_feature_torch"]
    recs = {}
    for layers in (None, "0", "2", "22"):
        old = os.environ.pop("RIFT_DEC_LAYERS", None)
        if layers is not None:
            os.environ["RIFT_DEC_LAYERS"] = layers
        try:
            eng = ffi.Engine("cuda:0", operands=fmt)
        finally:
            os.environ.pop("RIFT_DEC_LAYERS", None)
            if old is not None:
                os.environ["RIFT_DEC_LAYERS"] = old
        eng.load_state_dict({k: v.clone() for k, v in H.weights().items()})
        eng.prof_enable(True)
        eng.forward(data, need_traj=True)
        torch.cuda.synchronize()
        recs[layers] = {k: int(v["count"]) for k, v in eng.prof_report().items()}
        eng.prof_enable(False)
        eng.close()
    print(f"    {fmt} full: {sorted(recs[None].items())}")
    assert recs[None] == FULL_LAUNCHES, sorted(recs[None].items())
    rest = lambda r: {k: v for k, v in r.items() if k != "dec_w_kernel"}
    assert recs[None]["dec_w_kernel"] == 1 and "dec_w_kernel" not in recs["0"] and recs["2"]["dec_w_kernel"] == 1 and recs["22"]["dec_w_kernel"] == 2
    assert rest(recs["0"]) == rest(recs["2"]) == rest(recs["22"]) == rest(recs[None])
