"""include/rift_offroad.h against its hand-written ctypes mirror (rift_amd/_abi_offroad.py) and against the library, and the host half of the
extension (csrc/offroad_params.h: defaults and every refusal the riftof_ entries add to the wrapped entries' own).  No GPU."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rift_offroad.h")


def _generator():
    spec = importlib.util.spec_from_file_location("abi_trampolines", os.path.join(REPO, "tools", "gen", "abi_trampolines.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _declarations():
    """[(name, [(type, parameter)])] of every function the extension header declares, in header order."""
    text = _generator().strip_comments(open(HEADER).read())
    out = []
    for m in re.finditer(r"^(\w[\w \*]*?)\s+(riftof_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        assert m.group(1) == "int", m.group(0)
        params = []
        for a in (x.strip() for x in " ".join(m.group(3).split()).split(",")):
            pm = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a)
            params.append((pm.group(1).strip(), pm.group(2)))
        out.append((m.group(2), params))
    return out


def test_mirror_matches_the_header_by_the_generators_type_table():
    from rift_amd import _abi, _abi_drivable, _abi_footprint, _abi_offroad
    gen = _generator()
    decls = _declarations()
    assert [n for n, _ in decls] == list(_abi_offroad.EXPORTS) == ["riftof_params_default", "riftof_off_road_matrix", "riftof_group_advantage_tick"]
    text = open(HEADER).read()
    assert set(re.findall(r"\b(riftof_[a-z0-9_]+)\s*\(", text)) == set(_abi_offroad.EXPORTS)          # comments name no entry that does not exist
    assert not re.findall(r"^\s*(?:int|void|const char\*)\s+rift_[a-z0-9_]+\s*\(", gen.strip_comments(text), re.M)      # it declares nothing of rift_hip.h's
    assert not re.findall(r"^\s*(?:int|void|const char\*)\s+rift(?:cs|dm|ga|fp)_[a-z0-9_]+\s*\(", gen.strip_comments(text), re.M)      # nor of the other extensions
    known = {"RiftCtx": "opaque", "RiftOffRoadParams": "struct", "RiftCollisionParams": "struct", "RiftEvalParams": "struct", "RiftTickCBV": "struct"}
    ns = {"C": ctypes, "RiftOffRoadParams": _abi_offroad.RiftOffRoadParams, "RiftCollisionParams": _abi_footprint.RiftCollisionParams,
          "RiftEvalParams": _abi.RiftEvalParams, "RiftTickCBV": _abi.RiftTickCBV}
    for name, params in decls:
        restype, argtypes = _abi_offroad.SIGNATURES[name]
        assert restype is ctypes.c_int
        want = [eval(gen.ctype(t, known, f"{name}, parameter {p}"), ns) for t, p in params]      # noqa: S307 (the generator's own spellings)
        assert argtypes == want, (name, argtypes, want)
    # riftdm_off_road_matrix's arguments with the vertices behind the centre and the mask behind n, then offroad, off_road, which, stream
    base, mine = _abi_drivable.SIGNATURES["riftdm_off_road_matrix"][1], _abi_offroad.SIGNATURES["riftof_off_road_matrix"][1]
    assert [p for _, p in decls[1][1]] == ["ctx", "center", "vertices", "n", "mask", "H", "W", "ox", "oy", "heading", "params", "offroad", "off_road",
                                            "which", "stream"]
    assert mine[:2] + mine[3:4] + mine[5:11] + mine[12:13] + mine[14:] == base
    # every argument of riftfp_group_advantage_tick up to and including collision, the off-road params, then its last four
    base, mine = _abi_footprint.SIGNATURES["riftfp_group_advantage_tick"][1], _abi_offroad.SIGNATURES["riftof_group_advantage_tick"][1]
    assert len(decls[2][1]) == 19 and mine[:14] == base[:14] and mine[15:] == base[14:]
    assert [p for _, p in decls[2][1]][12:15] == ["params", "collision", "offroad"] and decls[2][1][14][0] == "const RiftOffRoadParams*"


def test_struct_layout_and_enumerators_as_a_c_compiler_has_them(tmp_path):
    from rift_amd import _abi_offroad as M
    from rift_amd import _ffi
    st = M.RiftOffRoadParams
    assert ctypes.sizeof(st) == 8 and [getattr(st, f).offset for f, _ in st._fields_] == [0, 4]
    enums = ["RIFTOF_CENTER", "RIFTOF_FOOTPRINT"]
    assert [getattr(M, e) for e in enums] == [0, 1] and _ffi.OFFROAD_EXTENTS == {"center": 0, "footprint": 1}
    body = re.search(r"typedef\s+struct\s+RiftOffRoadParams\s*\{(.*?)\}", _generator().strip_comments(open(HEADER).read()), re.S).group(1)
    fields = [d.strip() for stmt in body.split(";") if stmt.strip() for d in re.sub(r"^\s*\w+\s+", "", stmt.strip()).split(",")]
    assert fields == [f for f, _ in st._fields_]                                                        # every field, in order
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rift_offroad.h"', 'int main(void) {', '  printf("%zu", sizeof(RiftOffRoadParams));']
    lines += [f'  printf(" %zu", offsetof(RiftOffRoadParams, {f}));' for f, _ in st._fields_]
    lines += [f'  printf(" %d", {e});' for e in enums] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    size, *rest = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert size == ctypes.sizeof(st) == 8
    assert rest[:2] == [getattr(st, f).offset for f, _ in st._fields_] and rest[2:] == [0, 1]


def test_offroad_params_by_name():
    from rift_amd import _ffi
    p = _ffi.offroad_params()
    assert (p.extent, p.reserved) == (0, 0)
    p = _ffi.offroad_params("footprint")
    assert (p.extent, p.reserved) == (1, 0)
    with pytest.raises(ValueError, match="area.*known.*center.*footprint"):
        _ffi.offroad_params(extent="area")


def test_library_exports_the_extension_and_refuses_a_null_context():
    from rift_amd import _abi_offroad, _ffi, build
    build.build()
    lib = _ffi.load_library()
    for name, (restype, argtypes) in _abi_offroad.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the defaults need no context and no device
    p = _abi_offroad.RiftOffRoadParams(7, 7)
    assert lib.riftof_params_default(ctypes.byref(p)) == 0 and (p.extent, p.reserved) == (0, 0)
    assert bytes(memoryview(p)) == bytes(memoryview(_ffi.offroad_params()))
    assert lib.riftof_params_default(None) == -1
    # a null context is refused before anything is touched (no GPU here), whatever else the call carries
    ev = _ffi.eval_params()
    assert lib.riftof_off_road_matrix(None, None, None, 1, None, 16, 16, 0.0, 0.0, 0.0, ctypes.byref(ev), ctypes.byref(p), None, None, None) == -1
    assert lib.riftof_off_road_matrix(None, None, None, 0, None, 0, 0, 0.0, 0.0, 0.0, None, None, None, None, None) == -1
    bad = _abi_offroad.RiftOffRoadParams(2, 0)
    col = _ffi.collision_params()
    assert lib.riftof_group_advantage_tick(None, None, 1, 80, None, 0, None, None, None, None, None, None, None, ctypes.byref(col), ctypes.byref(bad),
                                           None, None, None, None) == -1
    assert lib.riftof_group_advantage_tick(None, None, 1, 80, None, 1, None, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    nm = shutil.which("llvm-nm") or next((p for p in ("/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm") if os.path.exists(p)), None) \
        or shutil.which("nm")
    if nm is None:
        pytest.skip("no llvm-nm / nm")
    out = subprocess.check_output([nm, "--defined-only", "-D", build.LIB], text=True)
    exported = {w[2] for w in (line.split(None, 2) for line in out.splitlines()) if len(w) == 3 and re.fullmatch(r"riftof_[a-z0-9_]+", w[2])}
    assert exported == set(_abi_offroad.EXPORTS) and len(exported) == 3
    # the prefix is its own: no riftof_ name is taken for one of the other sets
    assert not any(re.fullmatch(r"rift_[a-z0-9_]+|rift(?:cs|dm|ga|fp)_[a-z0-9_]+", n) for n in exported)


_REFUSALS = r"""
#include <stdio.h>
#include <string.h>
#include <limits.h>
#include "offroad_params.h"
static int fails = 0;
static void expect(const char* what, const char* got, const char* want) {
  const bool ok = want ? (got && strstr(got, want)) : !got;
  if (!ok) { ++fails; printf("FAIL %s: got %s, want %s\n", what, got ? got : "(accepted)", want ? want : "(accepted)"); }
}
int main() {
  RiftOffRoadParams d;
  d.extent = 9; d.reserved = 9;
  riftof_params_set_default(&d);
  if (d.extent != RIFTOF_CENTER || d.reserved != 0 || sizeof(d) != 8) { ++fails; printf("FAIL defaults\n"); }
  expect("defaults", riftof_refusal(&d), nullptr);
  expect("params NULL", riftof_refusal(nullptr), "params == NULL");
  RiftOffRoadParams p = d;
  p.extent = RIFTOF_FOOTPRINT; expect("footprint", riftof_refusal(&p), nullptr);
  const int bad[6] = {2, -1, 3, 256, INT_MAX, INT_MIN};
  for (int i = 0; i < 6; ++i) { p = d; p.extent = bad[i]; expect("extent", riftof_refusal(&p), "extent outside {0, 1}"); }
  const int res[4] = {1, -1, INT_MAX, INT_MIN};
  for (int m = 0; m < 2; ++m) for (int i = 0; i < 4; ++i) { p = d; p.extent = m; p.reserved = res[i]; expect("reserved", riftof_refusal(&p), "reserved != 0"); }
  p.extent = 2; p.reserved = 1; expect("the extent is named first", riftof_refusal(&p), "extent");
  // riftof_off_road_matrix: the corners are needed under FOOTPRINT and for `which`; the pointers are compared, never read
  float v[8]; uint8_t w[1];
  p = d;
  expect("center, no vertices, no which", riftof_matrix_refusal(&p, nullptr, nullptr), nullptr);
  expect("center, vertices, no which", riftof_matrix_refusal(&p, v, nullptr), nullptr);
  expect("center, vertices, which", riftof_matrix_refusal(&p, v, w), nullptr);
  expect("center, no vertices, which", riftof_matrix_refusal(&p, nullptr, w), "vertices == NULL with which given");
  p.extent = RIFTOF_FOOTPRINT;
  expect("footprint, vertices", riftof_matrix_refusal(&p, v, nullptr), nullptr);
  expect("footprint, vertices, which", riftof_matrix_refusal(&p, v, w), nullptr);
  expect("footprint, no vertices", riftof_matrix_refusal(&p, nullptr, nullptr), "vertices == NULL under FOOTPRINT");
  expect("footprint, no vertices, which", riftof_matrix_refusal(&p, nullptr, w), "vertices == NULL under FOOTPRINT");
  expect("matrix: params NULL", riftof_matrix_refusal(nullptr, v, w), "params == NULL");
  p.extent = 5; expect("matrix: the extent ahead of the vertices", riftof_matrix_refusal(&p, nullptr, w), "extent outside {0, 1}");
  p.extent = 1; p.reserved = 3; expect("matrix: reserved ahead of the vertices", riftof_matrix_refusal(&p, nullptr, w), "reserved != 0");
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def test_every_refusal_of_the_extension_on_the_host(tmp_path):
    """csrc/offroad_params.h (what the riftof_ entries refuse before any launch, ahead of the wrapped entries' refusals) in a stand-alone
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
