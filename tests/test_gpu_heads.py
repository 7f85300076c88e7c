"""The output heads -- heads3_fused_kernel on the planning rows (`trajectory`) and on the agent rows gathered from the encoder output
(`prediction`), ego_heads_kernel (`hidden`, `ref_free_trajectory`), and the layer-wise MLPLayer launches with interleave_traj_kernel --
against the fp64 reference of tests/heads_cases.py, on the designed batches one, b15, b16, b17, b33, p128, plan1056 and pred1056: planning
rows under one 128-row tile, a multiple of it, a multiple plus 12 and nine tiles (the second group of 8 tiles x 3 heads); prediction rows
from A = 2 to nine tiles, with tiles that start inside a scene; 1, 15, 16, 17 and 33 ego rows around the 16 of an ego_heads_kernel
workgroup.  tests/test_heads_cases.py proves on the CPU that a wrong component order, step mapping, gather offset or stride, a neighbour
tile's row, a LayerNorm over half the hidden layer, a missing ReLU or two dropped n-tiles moves one of these outputs by three bars.

The reference is fed the DEVICE's own enc_out and q_final taps, so device error and E_emu measure the heads alone.  trajectory is compared
on the valid lines, prediction on the valid agents, the ego heads on all scenes.  The caller owns the output tensors: they are pre-filled,
and every word behind the last row must still hold the fill after the forward.

Bars.  16-bit builds: K[fmt] * E_emu[case, tap, fmt] -- E_emu = what rounding both operands of every contraction to the format costs the
fp64 reference ON THE SAME INPUTS, K one factor per format for all taps, cases and builds (heads_cases.K).  fp32: heads_cases.FP32_BAR.
Needs a real MI355X: `pytest -m gpu`."""
import os

import pytest
import torch

from tests import heads_cases as HC

pytestmark = pytest.mark.gpu

LAYERWISE = {"RIFT_FOURIER_UNFUSED": "1", "RIFT_EGO_UNFUSED": "1", "RIFT_HEADS_UNFUSED": "1"}
BUILDS = {"default": {}, "layerwise": LAYERWISE, "poison-arena": {"RIFT_POISON_ARENA": "255"}, "poison-lds": {"RIFT_POISON_LDS": "255"}}
ENV_KEYS = sorted({k for env in BUILDS.values() for k in env})
FMTS = ("bf16", "fp16")
EVERY = [(b, f) for b in BUILDS for f in FMTS] + [("default", "fp32")]          # (the fp32 forward reads no switch: one build)
FILL, TAIL = -7777.0, 4096                  # what the output tensors hold ahead of a forward; words behind the last row of each


@pytest.fixture(scope="module")
def ffi():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    _ffi.load_library()
    return _ffi


@pytest.fixture(scope="module")
def run(ffi):
    """run(build, fmt | "fp32", case, need_traj=True) -> {tap: CPU tensor in the oracle's shape, "again": the same taps of a second forward,
    "tails": {tap: the words behind the last row}, "enc_out", "q_final", "launches": {label: count} of the first forward}.  One engine per
    build and format, made on first use with the build's switches in the environment (the context reads them when it is created) and kept
    to the end of the module."""
    from rift_amd._abi import RiftOutputs
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
            eng.load_state_dict({k: v.clone() for k, v in HC.case_weights().items()})
            engines[build, fmt] = eng
        return engines[build, fmt]

    def forward(eng, data, need_traj, fp32, shp):
        """One forward into pre-filled tensors of the caller's; with need_traj off the three trajectory outputs are not offered."""
        bs, R, per = shp["bs"], shp["R"], shp["per"]
        want = {"probability": (bs, R, 12), "hidden": (bs, 128)}
        if need_traj:
            want.update(trajectory=(bs, R, 12, 80, 6), prediction=(bs, per, 80, 6), ref_free_trajectory=(bs, 80, 4))
        fb, keep = ffi.feature_batch(data, eng.device)
        o = RiftOutputs()
        bufs = {}
        for k, s in want.items():
            bufs[k] = torch.full((torch.Size(s).numel() + TAIL,), FILL, device=eng.device)
            setattr(o, k, bufs[k].data_ptr())
        flags = (ffi.F_NEED_TRAJ if need_traj else 0) | (ffi.F_FP32 if fp32 else 0)
        eng.forward_raw(fb, o, flags, 0)
        eng.check_finite()
        torch.cuda.synchronize()
        got = {k: bufs[k][:-TAIL].view(s).cpu() for k, s in want.items()}
        tails = {k: bufs[k][-TAIL:].cpu() for k in want}
        del keep
        return got, tails

    def get(build, fmt, name, need_traj=True):
        key = (build, fmt, name, need_traj)
        if key not in cache:
            eng, data, shp = engine(build, fmt), HC.case(name), HC.shapes(name)
            eng.prof_enable(True)
            got, tails = forward(eng, data, need_traj, fmt == "fp32", shp)
            rep = eng.prof_report()
            eng.prof_enable(False)
            got["enc_out"] = eng.tap("enc_out").view(shp["bs"], shp["N"], 128).cpu()
            got["q_final"] = eng.tap("q_final").view(shp["bs"], shp["R"], HC.M, 128).cpu()
            got["tails"], got["launches"] = tails, {k: int(v["count"]) for k, v in rep.items()}
            got["again"] = forward(eng, data, need_traj, fmt == "fp32", shp)[0]
            cache[key] = got
        return cache[key]

    yield get
    for eng in engines.values():
        eng.close()


_refs = {}


def _reference(name, r):
    """(fp64 outputs, E_emu) of the reference on a run's own enc_out / q_final; shared by the runs whose inputs are bit for bit the same.
    The inputs are read where the heads read them: the ego slot and the agent slots 1 .. A - 1 of enc_out, all of q_final."""
    A = HC.SPEC[name][2]
    enc = r["enc_out"][:, :A]
    key = (name, hash(enc.numpy().tobytes()), hash(r["q_final"].numpy().tobytes()))
    if key not in _refs:
        valid = torch.cat([torch.ones(enc.shape[0], 1, dtype=torch.bool), HC.masks(HC.case(name))[1]], 1)
        assert torch.isfinite(enc[valid]).all() and torch.isfinite(r["q_final"]).all(), name
        enc_in = torch.nan_to_num(r["enc_out"])             # (rows of padded tokens may hold anything: their outputs are not compared)
        ref = HC.reference64(HC.case_weights(), enc_in, r["q_final"], A)
        _refs[key] = (ref, HC.emu_error(HC.case_weights(), enc_in, r["q_final"], HC.case(name), ref))
    return _refs[key]


def _errors(got, name, taps=HC.TAPS):
    """[(tap, max |device - fp64| over the compared part, max |reference|)]; every compared value finite."""
    ref, _ = _reference(name, got)
    data = HC.case(name)
    dev, want = HC.compared({t: got[t] for t in taps}, data), HC.compared(ref, data)
    rows = []
    for t in taps:
        assert dev[t].shape == want[t].shape and dev[t].numel() > 0, (name, t)
        assert torch.isfinite(dev[t]).all(), (name, t)
        assert not bool((dev[t] == FILL).any()), (name, t, "a compared row still holds the fill")
        rows.append((t, float((dev[t].double() - want[t]).abs().max()), float(want[t].abs().max())))
    return rows


def _launched(r, build, fmt, need_traj=True):
    """Every run ran the kernels it names."""
    ran = r["launches"]
    fused = fmt != "fp32" and build != "layerwise"
    assert ran.get("heads3_fused_kernel", 0) == (2 if fused and need_traj else 0), (build, fmt, sorted(ran.items()))
    assert ran.get("ego_heads_kernel", 0) == (1 if fused else 0), (build, fmt, sorted(ran.items()))
    assert ("interleave_traj_kernel" in ran) == (not fused and need_traj), (build, fmt, sorted(ran.items()))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("build", tuple(BUILDS))
def test_sixteen_bit_outputs_within_k_operand_rounding_errors(run, build, fmt):
    """trajectory (valid lines), prediction (valid agents), hidden and ref_free_trajectory of every case:
    |device - reference64(device inputs)| <= K[fmt] * E_emu[case, tap, fmt].  Measured on MI355X, worst device error / E_emu over all taps
    and cases: bf16 fused and poisoned 1.0000, layer-wise 1.0001 (plan1056, ref_free_trajectory); fp16 fused and poisoned 1.0035 (b17,
    ref_free_trajectory), layer-wise 1.0001 -- K = 3 for both formats."""
    worst, late = (0.0, None), []
    for name in HC.CASES:
        got = run(build, fmt, name)
        _launched(got, build, fmt)
        E = _reference(name, got)[1]
        for t, err, _ in _errors(got, name):
            ratio = err / E[t, fmt]
            print(f"    {build} {fmt} {name} {t}: |device - fp64| {err:.3e}, E_emu {E[t, fmt]:.3e}, ratio {ratio:.2f} (K {HC.K[fmt]})")
            worst = max(worst, (ratio, (name, t)))
            if not err <= HC.K[fmt] * E[t, fmt]:
                late.append((name, t, err, HC.K[fmt] * E[t, fmt]))
    print(f"  {build} {fmt}: worst device error / E_emu = {worst[0]:.2f} at {worst[1]}")
    assert not late, late


def test_fp32_outputs(run):
    """The exact-fp32 layer-wise path: all four outputs within FP32_BAR of the fp64 reference on its own inputs (measured worst 1.911e-6,
    p128 prediction; the bar is twice that rounded up, and under 1e-4 max(1, max |tap|))."""
    worst, late = (0.0, None), []
    for name in HC.CASES:
        got = run("default", "fp32", name)
        _launched(got, "default", "fp32")
        for t, err, top in _errors(got, name):
            print(f"    fp32 {name} {t}: |device - fp64| {err:.3e} (max |tap| {top:.1f})")
            worst = max(worst, (err, (name, t)))
            assert HC.FP32_BAR <= 1e-4 * max(1.0, top)
            if not err <= HC.FP32_BAR:
                late.append((name, t, err))
    print(f"  fp32: worst |device - fp64| = {worst[0]:.3e} at {worst[1]}")
    assert not late, late


@pytest.mark.parametrize("build,fmt", [(b, f) for b, f in EVERY if b in ("default", "layerwise")])
def test_hidden_without_the_trajectory_heads(run, build, fmt):
    """need_traj off (ego_heads_kernel's `ref` pointer is null; no heads3_fused_kernel launch): hidden is still written, within its bar
    and bit for bit the forward's with the trajectory heads."""
    for name in HC.CASES:
        a, b = run(build, fmt, name, False), run(build, fmt, name, True)
        _launched(a, build, fmt, need_traj=False)
        A = HC.SPEC[name][2]
        assert torch.equal(a["enc_out"][:, 0], b["enc_out"][:, 0]), (build, fmt, name)
        E = _reference(name, b)[1]
        (_, err, _), = _errors({**b, "hidden": a["hidden"]}, name, taps=("hidden",))
        bar = HC.FP32_BAR if fmt == "fp32" else HC.K[fmt] * E["hidden", fmt]
        print(f"    {build} {fmt} {name} hidden (no trajectory heads): |device - fp64| {err:.3e} (bar {bar:.2e})")
        assert err <= bar, (name, err, bar)
        assert torch.equal(a["hidden"], b["hidden"]), (build, fmt, name)
        assert set(a["tails"]) == {"probability", "hidden"} and A >= 2


@pytest.mark.parametrize("build,fmt", EVERY)
def test_second_forward_is_bit_identical_and_nothing_is_written_behind_the_last_row(run, build, fmt):
    """Two forwards of a case: the compared part of every output bit for bit.  The words behind the last row of every output tensor
    (trajectory: row bs R 12, prediction: row bs (A - 1), the ego heads and the logits: row bs) still hold what the caller put there."""
    for name in HC.CASES:
        for need_traj in (True, False):
            if not need_traj and build not in ("default", "layerwise"):
                continue
            got = run(build, fmt, name, need_traj)
            taps = HC.TAPS if need_traj else ("hidden",)
            data = HC.case(name)
            one, two = HC.compared({t: got[t] for t in taps}, data), HC.compared({t: got["again"][t] for t in taps}, data)
            for t in taps:
                assert torch.equal(one[t], two[t]), f"{build} {fmt} {name} {t}: {int((one[t] != two[t]).sum())} words differ between two forwards"
            for t, tail in got["tails"].items():
                assert bool((tail == FILL).all()), f"{build} {fmt} {name} {t}: {int((tail != FILL).sum())} words written behind the last row"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("build", ("poison-arena", "poison-lds"))
def test_outputs_do_not_depend_on_what_memory_held(run, build, fmt):
    """The arena (every word a NaN) or every CU's LDS filled with 0xFF ahead of the forward: the compared part of every output finite
    and bit for bit the plain run's -- the zero rows that pad the last tile of heads3_fused_kernel and the rows ego_heads_kernel clamps
    to come from nowhere else."""
    for name in HC.CASES:
        a, b = run(build, fmt, name), run("default", fmt, name)
        data = HC.case(name)
        ca, cb = HC.compared({t: a[t] for t in HC.TAPS}, data), HC.compared({t: b[t] for t in HC.TAPS}, data)
        assert torch.equal(a["q_final"], b["q_final"]), (build, fmt, name)
        for t in HC.TAPS:
            assert torch.isfinite(ca[t]).all(), (build, fmt, name, t)
            assert torch.equal(ca[t], cb[t]), f"{build} {fmt} {name} {t}: {int((ca[t] != cb[t]).sum())} words differ from the plain run"
