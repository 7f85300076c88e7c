"""include/rift_footprint.h against its hand-written ctypes mirror (rift_amd/_abi_footprint.py) and against the library, and the host half
of the extension (csrc/collision_params.h: defaults and every refusal the riftfp_ entries add to the wrapped entries' own).  No GPU."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rift_footprint.h")


def _generator():
    spec = importlib.util.spec_from_file_location("abi_trampolines", os.path.join(REPO, "tools", "gen", "abi_trampolines.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _declarations():
    """[(name, [(type, parameter)])] of every function the extension header declares, in header order."""
    text = _generator().strip_comments(open(HEADER).read())
    out = []
    for m in re.finditer(r"^(\w[\w \*]*?)\s+(riftfp_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        assert m.group(1) == "int", m.group(0)
        params = []
        for a in (x.strip() for x in " ".join(m.group(3).split()).split(",")):
            pm = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a)
            params.append((pm.group(1).strip(), pm.group(2)))
        out.append((m.group(2), params))
    return out


def test_mirror_matches_the_header_by_the_generators_type_table():
    from rift_amd import _abi, _abi_drivable, _abi_footprint
    gen = _generator()
    decls = _declarations()
    assert [n for n, _ in decls] == list(_abi_footprint.EXPORTS) == ["riftfp_params_default", "riftfp_collision_matrix", "riftfp_group_advantage_tick"]
    text = open(HEADER).read()
    assert set(re.findall(r"\b(riftfp_[a-z0-9_]+)\s*\(", text)) == set(_abi_footprint.EXPORTS)          # comments name no entry that does not exist
    assert not re.findall(r"^\s*(?:int|void|const char\*)\s+rift_[a-z0-9_]+\s*\(", gen.strip_comments(text), re.M)      # it declares nothing of rift_hip.h's
    assert not re.findall(r"^\s*(?:int|void|const char\*)\s+rift(?:cs|dm|ga)_[a-z0-9_]+\s*\(", gen.strip_comments(text), re.M)      # nor of the other extensions
    known = {"RiftCtx": "opaque", "RiftCollisionParams": "struct", "RiftEvalParams": "struct", "RiftTickCBV": "struct"}
    ns = {"C": ctypes, "RiftCollisionParams": _abi_footprint.RiftCollisionParams, "RiftEvalParams": _abi.RiftEvalParams, "RiftTickCBV": _abi.RiftTickCBV}
    for name, params in decls:
        restype, argtypes = _abi_footprint.SIGNATURES[name]
        assert restype is ctypes.c_int
        want = [eval(gen.ctype(t, known, f"{name}, parameter {p}"), ns) for t, p in params]      # noqa: S307 (the generator's own spellings)
        assert argtypes == want, (name, argtypes, want)
    # rift_collision_matrix's arguments up to Ts, then params, collision, first_actor, stream
    base, mine = _abi.SIGNATURES["rift_collision_matrix"][1], _abi_footprint.SIGNATURES["riftfp_collision_matrix"][1]
    assert len(decls[1][1]) == 11 and mine[:7] == base[:7] and mine[8] == base[7] and mine[10] == base[8]
    assert [p for _, p in decls[1][1]][7:] == ["params", "collision", "first_actor", "stream"] and decls[1][1][0] == ("RiftCtx*", "ctx")
    # every argument of riftdm_group_advantage_tick up to and including params, the collision params, then its last four
    base, mine = _abi_drivable.SIGNATURES["riftdm_group_advantage_tick"][1], _abi_footprint.SIGNATURES["riftfp_group_advantage_tick"][1]
    assert len(decls[2][1]) == 18 and mine[:13] == base[:13] and mine[14:] == base[13:]
    assert [p for _, p in decls[2][1]][12:14] == ["params", "collision"] and decls[2][1][13][0] == "const RiftCollisionParams*"


def test_struct_layout_and_enumerators_as_a_c_compiler_has_them(tmp_path):
    from rift_amd import _abi_footprint as M
    from rift_amd import _ffi
    st = M.RiftCollisionParams
    assert ctypes.sizeof(st) == 8 and [getattr(st, f).offset for f, _ in st._fields_] == [0, 4]
    enums = ["RIFTFP_ENVELOPE", "RIFTFP_FOOTPRINT"]
    assert [getattr(M, e) for e in enums] == [0, 1] and _ffi.COLLISION_MODES == {"envelope": 0, "footprint": 1}
    body = re.search(r"typedef\s+struct\s+RiftCollisionParams\s*\{(.*?)\}", _generator().strip_comments(open(HEADER).read()), re.S).group(1)
    fields = [d.strip() for stmt in body.split(";") if stmt.strip() for d in re.sub(r"^\s*\w+\s+", "", stmt.strip()).split(",")]
    assert fields == [f for f, _ in st._fields_]                                                        # every field, in order
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rift_footprint.h"', 'int main(void) {', '  printf("%zu", sizeof(RiftCollisionParams));']
    lines += [f'  printf(" %zu", offsetof(RiftCollisionParams, {f}));' for f, _ in st._fields_]
    lines += [f'  printf(" %d", {e});' for e in enums] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    size, *rest = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert size == ctypes.sizeof(st) == 8
    assert rest[:2] == [getattr(st, f).offset for f, _ in st._fields_] and rest[2:] == [0, 1]


def test_collision_params_by_name():
    from rift_amd import _ffi
    p = _ffi.collision_params()
    assert (p.mode, p.reserved) == (0, 0)
    p = _ffi.collision_params("footprint")
    assert (p.mode, p.reserved) == (1, 0)
    with pytest.raises(ValueError, match="sat.*known.*envelope.*footprint"):
        _ffi.collision_params(mode="sat")


def test_library_exports_the_extension_and_refuses_a_null_context():
    from rift_amd import _abi_footprint, _ffi, build
    build.build()
    lib = _ffi.load_library()
    for name, (restype, argtypes) in _abi_footprint.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the defaults need no context and no device
    p = _abi_footprint.RiftCollisionParams(7, 7)
    assert lib.riftfp_params_default(ctypes.byref(p)) == 0 and (p.mode, p.reserved) == (0, 0)
    assert bytes(memoryview(p)) == bytes(memoryview(_ffi.collision_params()))
    assert lib.riftfp_params_default(None) == -1
    # a null context is refused before anything is touched (no GPU here), whatever else the call carries
    assert lib.riftfp_collision_matrix(None, None, 1, 40, None, 0, 40, ctypes.byref(p), None, None, None) == -1
    assert lib.riftfp_collision_matrix(None, None, 0, 0, None, -1, 0, None, None, None, None) == -1
    bad = _abi_footprint.RiftCollisionParams(2, 0)
    assert lib.riftfp_group_advantage_tick(None, None, 1, 80, None, 0, None, None, None, None, None, None, None, ctypes.byref(bad), None, None, None, None) == -1
    assert lib.riftfp_group_advantage_tick(None, None, 1, 80, None, 1, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    nm = shutil.which("llvm-nm") or next((p for p in ("/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm") if os.path.exists(p)), None) \
        or shutil.which("nm")
    if nm is None:
        pytest.skip("no llvm-nm / nm")
    out = subprocess.check_output([nm, "--defined-only", "-D", build.LIB], text=True)
    exported = {w[2] for w in (line.split(None, 2) for line in out.splitlines()) if len(w) == 3 and re.fullmatch(r"riftfp_[a-z0-9_]+", w[2])}
    assert exported == set(_abi_footprint.EXPORTS) and len(exported) == 3
    # the prefix is its own: no riftfp_ name is taken for one of the other sets
    assert not any(re.fullmatch(r"rift_[a-z0-9_]+|rift(?:cs|dm|ga)_[a-z0-9_]+", n) for n in exported)


_REFUSALS = r"""
#include <stdio.h>
#include <string.h>
#include <limits.h>
#include "collision_params.h"
static int fails = 0;
static void expect(const char* what, const char* got, const char* want) {
  const bool ok = want ? (got && strstr(got, want)) : !got;
  if (!ok) { ++fails; printf("FAIL %s: got %s, want %s\n", what, got ? got : "(accepted)", want ? want : "(accepted)"); }
}
int main() {
  RiftCollisionParams d;
  d.mode = 9; d.reserved = 9;
  riftfp_params_set_default(&d);
  if (d.mode != RIFTFP_ENVELOPE || d.reserved != 0 || sizeof(d) != 8) { ++fails; printf("FAIL defaults\n"); }
  expect("defaults", riftfp_refusal(&d), nullptr);
  expect("params NULL", riftfp_refusal(nullptr), "params == NULL");
  RiftCollisionParams p = d;
  p.mode = RIFTFP_FOOTPRINT; expect("footprint", riftfp_refusal(&p), nullptr);
  const int bad[6] = {2, -1, 3, 256, INT_MAX, INT_MIN};
  for (int i = 0; i < 6; ++i) { p = d; p.mode = bad[i]; expect("mode", riftfp_refusal(&p), "mode outside {0, 1}"); }
  const int res[4] = {1, -1, INT_MAX, INT_MIN};
  for (int m = 0; m < 2; ++m) for (int i = 0; i < 4; ++i) { p = d; p.mode = m; p.reserved = res[i]; expect("reserved", riftfp_refusal(&p), "reserved != 0"); }
  p.mode = 2; p.reserved = 1; expect("the mode is named first", riftfp_refusal(&p), "mode");
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def test_every_refusal_of_the_extension_on_the_host(tmp_path):
    """csrc/collision_params.h (what the riftfp_ entries refuse before any launch, ahead of the wrapped entries' refusals) in a stand-alone
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
