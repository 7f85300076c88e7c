"""include/rift_drivable.h -- the drivable-area-map extension of the C-ABI, with a header and a symbol prefix (`riftdm_`) of its own --
against its hand-written ctypes mirror (rift_amd/_abi_drivable.py) and against the library, on the CPU: what tests/test_host_api.py holds
for include/rift_hip.h and its generated mirror, held here for the extension."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rift_drivable.h")


def _generator():
    spec = importlib.util.spec_from_file_location("abi_trampolines", os.path.join(REPO, "tools", "gen", "abi_trampolines.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _declarations():
    """[(name, [(type, parameter)])] of every function the extension header declares, in header order."""
    text = _generator().strip_comments(open(HEADER).read())
    out = []
    for m in re.finditer(r"^(\w[\w \*]*?)\s+(riftdm_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        assert m.group(1) == "int", m.group(0)
        params = []
        for a in (x.strip() for x in " ".join(m.group(3).split()).split(",")):
            pm = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a)
            params.append((pm.group(1).strip(), pm.group(2)))
        out.append((m.group(2), params))
    return out


def test_mirror_matches_the_header_by_the_generators_type_table():
    from rift_amd import _abi, _abi_drivable
    gen = _generator()
    decls = _declarations()
    assert [n for n, _ in decls] == list(_abi_drivable.EXPORTS) and len(decls) == 6
    text = open(HEADER).read()
    assert set(re.findall(r"\b(riftdm_[a-z0-9_]+)\s*\(", text)) == set(_abi_drivable.EXPORTS)          # comments name no entry that does not exist
    assert not re.findall(r"^\s*(?:int|void|const char\*)\s+rift_[a-z0-9_]+\s*\(", gen.strip_comments(text), re.M)      # it declares nothing of rift_hip.h's
    known = {"RiftCtx": "opaque", "RiftEvalParams": "struct", "RiftTickCBV": "struct", "RiftDrivableInfo": "struct"}
    ns = {"C": ctypes, "RiftEvalParams": _abi.RiftEvalParams, "RiftTickCBV": _abi.RiftTickCBV, "RiftDrivableInfo": _abi_drivable.RiftDrivableInfo}
    for name, params in decls:
        assert params[0] == ("RiftCtx*", "ctx"), name
        restype, argtypes = _abi_drivable.SIGNATURES[name]
        assert restype is ctypes.c_int
        want = [eval(gen.ctype(t, known, f"{name}, parameter {p}"), ns) for t, p in params]      # noqa: S307 (the generator's own spellings)
        assert argtypes == want, (name, argtypes, want)
    # the entry that takes rift_group_advantage_tick_ex's arguments takes exactly those
    assert _abi_drivable.SIGNATURES["riftdm_group_advantage_tick"][1] == _abi.SIGNATURES["rift_group_advantage_tick_ex"][1]


def test_struct_layout_as_a_c_compiler_lays_it_out(tmp_path):
    from rift_amd import _abi_drivable
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    st = _abi_drivable.RiftDrivableInfo
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rift_drivable.h"', 'int main(void) {', '  printf("%zu", sizeof(RiftDrivableInfo));']
    lines += [f'  printf(" %zu", offsetof(RiftDrivableInfo, {f}));' for f, _ in st._fields_] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    size, *offs = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert size == ctypes.sizeof(st) == 64
    assert offs == [getattr(st, f).offset for f, _ in st._fields_]
    body = re.search(r"typedef\s+struct\s+RiftDrivableInfo\s*\{(.*?)\}", _generator().strip_comments(open(HEADER).read()), re.S).group(1)
    fields = [d.strip() for stmt in body.split(";") if stmt.strip() for d in re.sub(r"^\s*\w+\s+", "", stmt.strip()).split(",")]
    assert fields == [f for f, _ in st._fields_]                                                        # every field, in order


def test_library_exports_the_extension_and_nothing_else_with_its_prefix():
    from rift_amd import _abi_drivable, _ffi, build
    build.build()
    lib = _ffi.load_library()
    for name, (restype, argtypes) in _abi_drivable.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # a null context is refused before anything is touched (no GPU here)
    assert lib.riftdm_clear(None) == -1 and lib.riftdm_info(None, None) == -1
    nm = shutil.which("llvm-nm") or next((p for p in ("/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm") if os.path.exists(p)), None) \
        or shutil.which("nm")
    if nm is None:
        pytest.skip("no llvm-nm / nm")
    out = subprocess.check_output([nm, "--defined-only", "-D", build.LIB], text=True)
    exported = {w[2] for w in (line.split(None, 2) for line in out.splitlines()) if len(w) == 3 and re.fullmatch(r"riftdm_[a-z0-9_]+", w[2])}
    assert exported == set(_abi_drivable.EXPORTS)
