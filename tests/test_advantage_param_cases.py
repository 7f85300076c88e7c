"""The arena advantage on the host: the restatement of tests/advantage_param_cases.py against the oracle's z-score and the literal
leave-one-out, the conditions its inputs must satisfy, include/rift_advantage.h against its hand-written ctypes mirror
(rift_amd/_abi_advantage.py) and against the library, and every refusal of the entry.  No GPU."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import advantage as oadv
from tests import advantage_param_cases as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rift_advantage.h")


def _generator():
    spec = importlib.util.spec_from_file_location("abi_trampolines", os.path.join(REPO, "tools", "gen", "abi_trampolines.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_case_table_covers_every_kind():
    cases = [A.case(k) for k in range(len(A.SHAPES))]
    assert {(c["mask_kind"], c["dist"]) for c in cases} == {(m, d) for m in A.MASKS for d in A.DISTS}
    assert {(c["n"], c["Rcap"]) for c in cases} == {(n, r) for n in A.NS for r in A.RCAPS} | {A.BIG}
    assert any(c["r_count"] is None for c in cases)
    rc = np.concatenate([c["r_count"] for c in cases if c["r_count"] is not None])
    assert (rc == 0).any() and all((c["r_count"] == c["Rcap"]).any() for c in cases if c["r_count"] is not None)
    G = np.concatenate([A.valid_of(c).reshape(c["n"], -1).sum(1) for c in cases])
    assert {0, 1, 2} <= set(G.tolist()) and G.max() == 204
    used = set()
    for k in range(len(A.SHAPES)):
        used |= {s for s in A.settings(k) if A.is_case(A.case(k), *s)}
    assert used == {(b, s, c, e) for b in A.BASELINES for s in A.SCALES for c in A.CLIPS for e in A.EPSS}
    # what is left out: eps = 0 alone, and only where a denominator is exactly 0
    for k in range(len(A.SHAPES)):
        for s in A.settings(k):
            if not A.is_case(A.case(k), *s):
                st = A.restate(A.case(k), *s)[2]
                assert s[3] == 0.0 and ((s[1] == "group_std" and st[2] > 0) or (s[1] == "batch_rms" and st[3] == 0.0)), (k, s)


def test_default_parameters_restate_the_oracles_zscore():
    worst = 0.0
    for k in range(len(A.SHAPES)):
        c = A.case(k)
        adv, _, stats = A.restate(c, "mean", "group_std", 0.0, 1e-5)
        valid = A.valid_of(c)
        for i in range(c["n"]):
            x = c["returns"][i][valid[i]]
            if x.size:
                worst = max(worst, float(np.max(np.abs(adv[i][valid[i]] - oadv.group_zscore(x)))))
            assert np.all(adv[i][~valid[i]] == 0.0)
        assert stats[0] == valid.sum() and stats[3] == 0.0 and stats[4] == 0.0
    print(f"restatement against oracle.advantage.group_zscore: {worst:.2e}")
    assert worst < 1e-12


def test_leave_one_out_is_the_mean_of_the_others():
    worst = 0.0
    for k in range(len(A.SHAPES)):
        c = A.case(k)
        adv, _, _ = A.restate(c, "leave_one_out", "none", 0.0, 1e-5)
        worst = max(worst, float(np.max(np.abs(adv - A.loo_literal(c)))))
    print(f"leave-one-out against x - mean(others): {worst:.2e}")
    assert worst < 1e-9


def test_no_value_sits_at_the_clip():
    """A condition on the inputs: in every clipped case every value before the clamp is further than CLIP_MARGIN from +-clip, so that the
    number of clamped candidates cannot differ by rounding."""
    closest, clamped = np.inf, 0
    for k in range(len(A.SHAPES)):
        c = A.case(k)
        valid = A.valid_of(c)
        for s in A.settings(k):
            if s[2] > 0 and A.is_case(c, *s):
                _, raw, stats = A.restate(c, *s)
                closest = min(closest, float(np.min(np.abs(np.abs(raw[valid]) - s[2]), initial=np.inf)))
                clamped += int(stats[4])
    print(f"closest value to a clip: {closest:.2e}; clamped in all: {clamped}")
    assert closest > A.CLIP_MARGIN and clamped > 0


def _declarations():
    """[(name, [(type, parameter)])] of every function the extension header declares, in header order."""
    text = _generator().strip_comments(open(HEADER).read())
    out = []
    for m in re.finditer(r"^(\w[\w \*]*?)\s+(riftga_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        assert m.group(1) == "int", m.group(0)
        params = []
        for a in (x.strip() for x in " ".join(m.group(3).split()).split(",")):
            pm = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a)
            params.append((pm.group(1).strip(), pm.group(2)))
        out.append((m.group(2), params))
    return out


def test_mirror_matches_the_header_by_the_generators_type_table():
    from rift_amd import _abi_advantage
    gen = _generator()
    decls = _declarations()
    assert [n for n, _ in decls] == list(_abi_advantage.EXPORTS) and len(decls) == 2
    text = open(HEADER).read()
    assert set(re.findall(r"\b(riftga_[a-z0-9_]+)\s*\(", text)) == set(_abi_advantage.EXPORTS)          # comments name no entry that does not exist
    assert not re.findall(r"^\s*(?:int|void|const char\*)\s+rift_[a-z0-9_]+\s*\(", gen.strip_comments(text), re.M)      # it declares nothing of rift_hip.h's
    known = {"RiftCtx": "opaque", "RiftAdvantageParams": "struct"}
    ns = {"C": ctypes, "RiftAdvantageParams": _abi_advantage.RiftAdvantageParams}
    for name, params in decls:
        restype, argtypes = _abi_advantage.SIGNATURES[name]
        assert restype is ctypes.c_int
        want = [eval(gen.ctype(t, known, f"{name}, parameter {p}"), ns) for t, p in params]      # noqa: S307 (the generator's own spellings)
        assert argtypes == want, (name, argtypes, want)
    assert decls[1][1][0] == ("RiftCtx*", "ctx")


def test_struct_layout_and_enumerators_as_a_c_compiler_has_them(tmp_path):
    from rift_amd import _abi_advantage as M
    from rift_amd import _ffi
    st = M.RiftAdvantageParams
    assert ctypes.sizeof(st) == 24
    enums = ["RIFTGA_BASELINE_MEAN", "RIFTGA_BASELINE_LEAVE_ONE_OUT", "RIFTGA_BASELINE_NONE", "RIFTGA_SCALE_GROUP_STD", "RIFTGA_SCALE_BATCH_RMS",
             "RIFTGA_SCALE_NONE"]
    assert [getattr(M, e) for e in enums] == [0, 1, 2, 0, 1, 2]
    assert list(_ffi.ADVANTAGE_BASELINES.values()) == [0, 1, 2] and list(_ffi.ADVANTAGE_SCALES.values()) == [0, 1, 2]
    assert tuple(_ffi.ADVANTAGE_BASELINES) == A.BASELINES and tuple(_ffi.ADVANTAGE_SCALES) == A.SCALES
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rift_advantage.h"', 'int main(void) {', '  printf("%zu", sizeof(RiftAdvantageParams));']
    lines += [f'  printf(" %zu", offsetof(RiftAdvantageParams, {f}));' for f, _ in st._fields_]
    lines += [f'  printf(" %d", {e});' for e in enums] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    size, *rest = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert size == ctypes.sizeof(st) == 24
    assert rest[:4] == [getattr(st, f).offset for f, _ in st._fields_] and rest[4:] == [getattr(M, e) for e in enums]
    body = re.search(r"typedef\s+struct\s+RiftAdvantageParams\s*\{(.*?)\}", _generator().strip_comments(open(HEADER).read()), re.S).group(1)
    fields = [d.strip() for stmt in body.split(";") if stmt.strip() for d in re.sub(r"^\s*\w+\s+", "", stmt.strip()).split(",")]
    assert fields == [f for f, _ in st._fields_]                                                        # every field, in order


def test_advantage_params_by_name():
    from rift_amd import _ffi
    p = _ffi.advantage_params()
    assert (p.baseline, p.scale, p.eps, p.clip) == (0, 0, 1e-5, 0.0)
    p = _ffi.advantage_params("leave_one_out", "batch_rms", clip=1.5, eps=0.0)
    assert (p.baseline, p.scale, p.eps, p.clip) == (1, 1, 0.0, 1.5)
    with pytest.raises(ValueError, match="loo.*known.*mean.*leave_one_out.*none"):
        _ffi.advantage_params(baseline="loo")
    with pytest.raises(ValueError, match="std.*known.*group_std.*batch_rms.*none"):
        _ffi.advantage_params(scale="std")


def test_library_exports_the_extension_and_refuses_a_null_context():
    from rift_amd import _abi_advantage, _ffi, build
    build.build()
    lib = _ffi.load_library()
    for name, (restype, argtypes) in _abi_advantage.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the defaults need no context and no device
    p = _abi_advantage.RiftAdvantageParams(7, 7, -1.0, -1.0)
    assert lib.riftga_params_default(ctypes.byref(p)) == 0 and (p.baseline, p.scale, p.eps, p.clip) == (0, 0, 1e-5, 0.0)
    assert bytes(memoryview(p)) == bytes(memoryview(_ffi.advantage_params()))
    assert lib.riftga_params_default(None) == -1
    # a null context is refused before anything is touched (no GPU here), whatever else the call carries
    assert lib.riftga_arena_advantage(None, None, None, None, 0, 1, ctypes.byref(p), None, None, None) == -1
    assert lib.riftga_arena_advantage(None, None, None, None, 4, 6, None, None, None, None) == -1
    bad = _abi_advantage.RiftAdvantageParams(3, 0, 1e-5, 0.0)
    assert lib.riftga_arena_advantage(None, None, None, None, -1, 0, ctypes.byref(bad), None, None, None) == -1
    nm = shutil.which("llvm-nm") or next((p for p in ("/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm") if os.path.exists(p)), None) \
        or shutil.which("nm")
    if nm is None:
        pytest.skip("no llvm-nm / nm")
    out = subprocess.check_output([nm, "--defined-only", "-D", build.LIB], text=True)
    exported = {w[2] for w in (line.split(None, 2) for line in out.splitlines()) if len(w) == 3 and re.fullmatch(r"riftga_[a-z0-9_]+", w[2])}
    assert exported == set(_abi_advantage.EXPORTS)


_REFUSALS = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "adv_params.h"
static int fails = 0;
static void expect(const char* what, const char* got, const char* want) {
  const bool ok = want ? (got && strstr(got, want)) : !got;
  if (!ok) { ++fails; printf("FAIL %s: got %s, want %s\n", what, got ? got : "(accepted)", want ? want : "(accepted)"); }
}
int main() {
  double ret[12] = {0}, adv[12] = {0};
  RiftAdvantageParams d;
  riftga_params_set_default(&d);
  if (d.baseline != RIFTGA_BASELINE_MEAN || d.scale != RIFTGA_SCALE_GROUP_STD || d.eps != 1e-5 || d.clip != 0.0) { ++fails; printf("FAIL defaults\n"); }
  expect("defaults", riftga_refusal(ret, 1, 1, &d, adv), nullptr);
  expect("params NULL", riftga_refusal(ret, 1, 1, nullptr, adv), "params == NULL");
  RiftAdvantageParams p = d;
  p.baseline = 3; expect("baseline 3", riftga_refusal(ret, 1, 1, &p, adv), "baseline"); p.baseline = -1; expect("baseline -1", riftga_refusal(ret, 1, 1, &p, adv), "baseline");
  p = d; p.scale = 3; expect("scale 3", riftga_refusal(ret, 1, 1, &p, adv), "scale"); p.scale = -1; expect("scale -1", riftga_refusal(ret, 1, 1, &p, adv), "scale");
  for (int b = 0; b < 3; ++b) for (int s = 0; s < 3; ++s) { p = d; p.baseline = b; p.scale = s; expect("pair", riftga_refusal(ret, 1, 1, &p, adv), nullptr); }
  const double bad[4] = {NAN, INFINITY, -INFINITY, -1e-300};
  for (int i = 0; i < 4; ++i) {
    p = d; p.eps = bad[i]; expect("eps", riftga_refusal(ret, 1, 1, &p, adv), "eps");
    p = d; p.clip = bad[i]; expect("clip", riftga_refusal(ret, 1, 1, &p, adv), "clip");
  }
  p = d; p.eps = 0.0; p.clip = 1.5; expect("eps 0, clip 1.5", riftga_refusal(ret, 1, 1, &p, adv), nullptr);
  expect("n < 0", riftga_refusal(ret, -1, 1, &d, adv), "n < 0");
  expect("Rcap 0", riftga_refusal(ret, 1, 0, &d, adv), "Rcap < 1");
  expect("returns NULL", riftga_refusal(nullptr, 1, 1, &d, adv), "NULL");
  expect("advantage NULL", riftga_refusal(ret, 1, 1, &d, nullptr), "NULL");
  expect("in place", riftga_refusal(ret, 1, 1, &d, ret), "advantage == returns");
  expect("n == 0 with null pointers", riftga_refusal(nullptr, 0, 1, &d, nullptr), nullptr);
  if (riftga_scratch_doubles(5) != 5 * RIFTGA_NPART + RIFTGA_NTOT) { ++fails; printf("FAIL scratch\n"); }
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def test_every_refusal_of_the_entry_on_the_host(tmp_path):
    """csrc/adv_params.h's host half (the refusals riftga_arena_advantage decides before any launch) in a stand-alone program built by g++
    with the address and undefined-behaviour sanitizers, run directly."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = tmp_path / "refusals.cpp"
    src.write_text(_REFUSALS)
    exe = tmp_path / "refusals"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "rift_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
