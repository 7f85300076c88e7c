"""include/rift_select.h against its hand-written ctypes mirror (rift_amd/_abi_select.py) and against the library, and the host half of
the extension (csrc/select_params.h: defaults and every refusal riftcs_control_tick adds to rift_control_tick's own).  No GPU."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rift_select.h")


def _generator():
    spec = importlib.util.spec_from_file_location("abi_trampolines", os.path.join(REPO, "tools", "gen", "abi_trampolines.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _declarations():
    """[(name, [(type, parameter)])] of every function the extension header declares, in header order."""
    text = _generator().strip_comments(open(HEADER).read())
    out = []
    for m in re.finditer(r"^(\w[\w \*]*?)\s+(riftcs_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        assert m.group(1) == "int", m.group(0)
        params = []
        for a in (x.strip() for x in " ".join(m.group(3).split()).split(",")):
            pm = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a)
            params.append((pm.group(1).strip(), pm.group(2)))
        out.append((m.group(2), params))
    return out


def test_mirror_matches_the_header_by_the_generators_type_table():
    from rift_amd import _abi, _abi_select
    gen = _generator()
    decls = _declarations()
    assert [n for n, _ in decls] == list(_abi_select.EXPORTS) == ["riftcs_params_default", "riftcs_control_tick"]
    text = open(HEADER).read()
    assert set(re.findall(r"\b(riftcs_[a-z0-9_]+)\s*\(", text)) == set(_abi_select.EXPORTS)            # comments name no entry that does not exist
    assert not re.findall(r"^\s*(?:int|void|const char\*)\s+rift_[a-z0-9_]+\s*\(", gen.strip_comments(text), re.M)      # it declares nothing of rift_hip.h's
    known = {"RiftCtx": "opaque", "RiftSelectParams": "struct", "RiftControlCBV": "struct"}
    ns = {"C": ctypes, "RiftSelectParams": _abi_select.RiftSelectParams, "RiftControlCBV": _abi.RiftControlCBV}
    for name, params in decls:
        restype, argtypes = _abi_select.SIGNATURES[name]
        assert restype is ctypes.c_int
        want = [eval(gen.ctype(t, known, f"{name}, parameter {p}"), ns) for t, p in params]      # noqa: S307 (the generator's own spellings)
        assert argtypes == want, (name, argtypes, want)
    # every argument of rift_control_tick up to n_slots, with its type, then params and u, then rift_control_tick's last two
    base = _abi.SIGNATURES["rift_control_tick"][1]
    mine = _abi_select.SIGNATURES["riftcs_control_tick"][1]
    assert len(decls[1][1]) == 16 and mine[:12] == base[:12] and mine[14:] == base[12:]
    assert [p for _, p in decls[1][1]][12:14] == ["params", "u"] and decls[1][1][0] == ("RiftCtx*", "ctx")


def test_struct_layout_and_enumerators_as_a_c_compiler_has_them(tmp_path):
    from rift_amd import _abi_select as M
    from rift_amd import _ffi
    st = M.RiftSelectParams
    assert ctypes.sizeof(st) == 16 and [getattr(st, f).offset for f, _ in st._fields_] == [0, 4, 8]
    enums = ["RIFTCS_GREEDY", "RIFTCS_SAMPLE"]
    assert [getattr(M, e) for e in enums] == [0, 1] and _ffi.SELECT_MODES == {"greedy": 0, "sample": 1}
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rift_select.h"', 'int main(void) {', '  printf("%zu", sizeof(RiftSelectParams));']
    lines += [f'  printf(" %zu", offsetof(RiftSelectParams, {f}));' for f, _ in st._fields_]
    lines += [f'  printf(" %d", {e});' for e in enums] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    size, *rest = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert size == ctypes.sizeof(st) == 16
    assert rest[:3] == [getattr(st, f).offset for f, _ in st._fields_] and rest[3:] == [0, 1]
    body = re.search(r"typedef\s+struct\s+RiftSelectParams\s*\{(.*?)\}", _generator().strip_comments(open(HEADER).read()), re.S).group(1)
    fields = [d.strip() for stmt in body.split(";") if stmt.strip() for d in re.sub(r"^\s*\w+\s+", "", stmt.strip()).split(",")]
    assert fields == [f for f, _ in st._fields_]                                                        # every field, in order


def test_select_params_by_name():
    from rift_amd import _ffi
    p = _ffi.select_params()
    assert (p.mode, p.reserved, p.temperature) == (0, 0, 1.0)
    p = _ffi.select_params("sample", 0.7)
    assert (p.mode, p.reserved, p.temperature) == (1, 0, 0.7)
    with pytest.raises(ValueError, match="softmax.*known.*greedy.*sample"):
        _ffi.select_params(mode="softmax")


def test_library_exports_the_extension_and_refuses_a_null_context():
    from rift_amd import _abi_select, _ffi, build
    build.build()
    lib = _ffi.load_library()
    for name, (restype, argtypes) in _abi_select.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the defaults need no context and no device
    p = _abi_select.RiftSelectParams(7, 7, -1.0)
    assert lib.riftcs_params_default(ctypes.byref(p)) == 0 and (p.mode, p.reserved, p.temperature) == (0, 0, 1.0)
    assert bytes(memoryview(p)) == bytes(memoryview(_ffi.select_params()))
    assert lib.riftcs_params_default(None) == -1
    # a null context is refused before anything is touched (no GPU here), whatever else the call carries
    assert lib.riftcs_control_tick(None, None, None, None, 1, 80, None, 0, 1, 10, None, 0, ctypes.byref(p), None, None, None) == -1
    assert lib.riftcs_control_tick(None, None, None, None, 4, 80, None, 3, 10, 10, None, 8, None, None, None, None) == -1
    bad = _abi_select.RiftSelectParams(2, 0, 1.0)
    assert lib.riftcs_control_tick(None, None, None, None, 0, 0, None, -1, 0, 0, None, -1, ctypes.byref(bad), None, None, None) == -1
    nm = shutil.which("llvm-nm") or next((p for p in ("/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm") if os.path.exists(p)), None) \
        or shutil.which("nm")
    if nm is None:
        pytest.skip("no llvm-nm / nm")
    out = subprocess.check_output([nm, "--defined-only", "-D", build.LIB], text=True)
    exported = {w[2] for w in (line.split(None, 2) for line in out.splitlines()) if len(w) == 3 and re.fullmatch(r"riftcs_[a-z0-9_]+", w[2])}
    assert exported == set(_abi_select.EXPORTS) and len(exported) == 2


_REFUSALS = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "select_params.h"
static int fails = 0;
static void expect(const char* what, const char* got, const char* want) {
  const bool ok = want ? (got && strstr(got, want)) : !got;
  if (!ok) { ++fails; printf("FAIL %s: got %s, want %s\n", what, got ? got : "(accepted)", want ? want : "(accepted)"); }
}
int main() {
  RiftSelectParams d;
  riftcs_params_set_default(&d);
  if (d.mode != RIFTCS_GREEDY || d.reserved != 0 || d.temperature != 1.0) { ++fails; printf("FAIL defaults\n"); }
  double u[3] = {0.0, 0.5, 0.99999999999999989};
  expect("defaults, no u", riftcs_refusal(&d, nullptr, 3), nullptr);
  expect("params NULL", riftcs_refusal(nullptr, u, 3), "params == NULL");
  RiftSelectParams p = d;
  p.mode = 2; expect("mode 2", riftcs_refusal(&p, u, 3), "mode"); p.mode = -1; expect("mode -1", riftcs_refusal(&p, u, 3), "mode");
  p = d; p.reserved = 1; expect("reserved", riftcs_refusal(&p, u, 3), "reserved != 0");
  const double bad[5] = {NAN, INFINITY, -INFINITY, 0.0, -1.0};
  for (int m = 0; m < 2; ++m) for (int i = 0; i < 5; ++i) { p = d; p.mode = m; p.temperature = bad[i]; expect("temperature", riftcs_refusal(&p, u, 3), "temperature"); }
  p = d; p.mode = RIFTCS_SAMPLE; p.temperature = 0.05;
  expect("sample", riftcs_refusal(&p, u, 3), nullptr);
  expect("sample, u NULL", riftcs_refusal(&p, nullptr, 3), "u == NULL");
  expect("sample, u NULL, K 0", riftcs_refusal(&p, nullptr, 0), nullptr);
  expect("sample, K < 0 is the tick's refusal", riftcs_refusal(&p, nullptr, -1), nullptr);
  const double badu[5] = {NAN, 1.0, -1e-300, INFINITY, 1.5};
  for (int i = 0; i < 5; ++i) for (int k = 0; k < 3; ++k) {
    double v[3] = {0.1, 0.2, 0.3}; v[k] = badu[i];
    expect("u", riftcs_refusal(&p, v, 3), "u[k]");
    expect("u beyond K is not read", riftcs_refusal(&p, v, k), nullptr);
    expect("u in GREEDY is not read", riftcs_refusal(&d, v, 3), nullptr);
  }
  p.temperature = 1.0; if (riftcs_inv_temperature(&p) != 1.0f) { ++fails; printf("FAIL 1 / 1\n"); }
  p.temperature = 0.05; if (riftcs_inv_temperature(&p) != (float)(1.0 / 0.05)) { ++fails; printf("FAIL 1 / 0.05\n"); }
  p.temperature = 1e-300; if (!isfinite(riftcs_inv_temperature(&p))) { ++fails; printf("FAIL the reciprocal stays finite\n"); }
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def test_every_refusal_of_the_extension_on_the_host(tmp_path):
    """csrc/select_params.h (what riftcs_control_tick refuses before any launch, ahead of rift_control_tick's refusals) in a stand-alone
    program built by g++ with the address and undefined-behaviour sanitizers, run directly."""
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
