"""Host-side mirror of the reference API (CPU-only checks; no compute calls)."""
import ctypes
import os
import re

import pytest
import torch

from tests import helpers as H


def test_state_dict_matches_reference_manifest():
    from rift_amd.planning.pluto.model.pluto_model import PlanningModel
    m = PlanningModel(radius=120)
    sd = m.state_dict()
    man = H.manifest()
    assert list(sd.keys()) == list(man.keys())          # names AND order
    for k, v in sd.items():
        assert list(v.shape) == man[k], k
    assert sum(p.numel() for p in m.parameters()) == 4240589
    # perturbed fixture weights load strictly
    m.load_state_dict(H.weights(), strict=True)


def test_model_refuses_cpu_forward():
    from rift_amd.planning.pluto.model.pluto_model import PlanningModel
    m = PlanningModel(radius=120)
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP device"):
        m.forward(H.build_batch("small")["cur_pluto_feature_torch"])


def test_library_exports_every_declared_symbol():
    """The C-ABI library loads on a GPU-less box and exports every function include/rift_hip.h declares."""
    from rift_amd import _ffi, build
    build.build()
    lib = _ffi.load_library()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rift_hip.h")).read()
    declared = set(re.findall(r"\b(rift_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in rift_hip.h but not exported"
    assert set(_ffi.EXPORTS) == declared


def _generator():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("abi_trampolines", os.path.join(repo, "tools", "gen", "abi_trampolines.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trampolines_are_generated_from_the_header():
    """csrc/abi.cpp / abi_list.h (the exported symbols: routing onto the bf16- or fp16-operand build that owns a context) and
    rift_amd/_abi.py (the ctypes mirror the Python binding applies) are what tools/gen/abi_trampolines.py derives from
    include/rift_hip.h -- the header stays the single statement of the interface."""
    mod = _generator()
    lst, cpp = mod.render()
    assert open(mod.OUT_LIST).read() == lst and open(mod.OUT_CPP).read() == cpp, "run python tools/gen/abi_trampolines.py"
    assert open(mod.OUT_PY).read() == mod.binding(), "run python tools/gen/abi_trampolines.py"
    from rift_amd import _ffi
    lib = _ffi.load_library()
    for sym in ("rift_vtable_bf16", "rift_vtable_fp16"):          # one table per operand-format build
        assert hasattr(lib, sym), sym
    # no GPU here: creating a context for an unknown operand format is refused before any device call
    ctx = ctypes.c_void_p()
    assert lib.rift_ctx_create_ex(0, 7, ctypes.byref(ctx)) == -1


def test_format_free_entries_are_defined_once_and_the_context_types_cannot_collide():
    """The objects of the library (csrc/shared.hip is compiled once, csrc/engine.hip once per operand format), read with nm:
    (a) the two engine builds define no common symbol of a context type -- each build's context is a type of its own namespace, so no
        destructor or member function of one can be linked in place of the other's;
    (b) every operand-format-free entry (tools/gen/abi_trampolines.py: FORMAT_FREE) is defined in shared.o and in neither engine object;
    (c) the device-memory hooks are defined in shared.o only;
    (d) the library exports the `rift_*` symbols of tests/golden/exported_symbols.txt (the functions include/rift_hip.h declares, by the
        generator's own parse, and one table per engine build), no more and no fewer."""
    import shutil
    import subprocess
    from rift_amd import build
    build.build()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    nm = shutil.which("llvm-nm") or next((p for p in ("/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm") if os.path.exists(p)), None) \
        or shutil.which("nm")
    if nm is None:
        pytest.skip("no llvm-nm / nm")
    objs = {n: os.path.join(build.OBJ, n + ".o") for n in ("engine_bf", "engine_hf", "shared")}
    if not all(os.path.exists(p) for p in objs.values()):          # (a library that was up to date, its objects cleaned away)
        build.build(force=True)

    def defined(path, flags=("-C",), kinds="TWV"):
        out = subprocess.check_output([nm, "--defined-only", *flags, path], text=True)
        return {line.split(None, 2)[2] for line in out.splitlines() if len(line.split(None, 2)) == 3 and line.split(None, 2)[1] in kinds}

    sym = {n: defined(p) for n, p in objs.items()}
    # (a)
    both = {s for s in sym["engine_bf"] & sym["engine_hf"] if "RiftCtx::" in s or "Ctx::~" in s}
    assert not both, both
    assert any(s.startswith("rift_bf::Ctx::~Ctx") for s in sym["engine_bf"]) and any(s.startswith("rift_hf::Ctx::~Ctx") for s in sym["engine_hf"])
    # (b), (c)
    gen = _generator()
    assert len(gen.FORMAT_FREE) == 29 and not set(gen.FORMAT_FREE) & set(gen.SPECIAL) and not set(gen.FORMAT_FREE) & set(gen.NO_CTX)

    def names(symbols):          # "rift::abi::rift_gae(RiftCtx*, ...)" -> "rift_gae"
        return {s.split("(")[0].split("::")[-1] for s in symbols if "::abi::rift_" in s.split("(")[0]} | {s.split("(")[0] for s in symbols if s.startswith("rift_dev_")}
    for name in gen.FORMAT_FREE + ("rift_dev_alloc", "rift_dev_free"):
        assert name in names(sym["shared"]), f"{name} is not defined in shared.o"
        assert name not in names(sym["engine_bf"]) and name not in names(sym["engine_hf"]), f"{name} is defined in an engine build"
    assert all(s.split("(")[0].startswith("rift::abi::") for s in sym["shared"] if "::abi::rift_" in s.split("(")[0])
    # (d)
    exported = {s for s in defined(build.LIB, ("-D",), "TWVRDB") if re.fullmatch(r"rift_[a-z0-9_]+", s)}      # (mangled names: C symbols only)
    golden = set(open(os.path.join(repo, "tests", "golden", "exported_symbols.txt")).read().split())
    declared = {name for _, name, _ in gen.declarations(open(gen.HEADER).read())}
    assert golden == declared | {"rift_vtable_bf16", "rift_vtable_fp16"}
    assert exported == golden, (sorted(exported - golden), sorted(golden - exported))


def test_bench_kernel_labels_resolve_in_the_committed_counter_tables():
    """bench.py's roofline object reads HBM traffic and MFMA counters of the dominant kernel from the newest committed PMC passes
    (profiles/rNN_pmc_*): every kernel the newest committed bench line lists must resolve there, so that a renamed kernel shows up here
    and not as a silent `traffic: null` at round end."""
    import glob
    import importlib.util
    import json
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench", os.path.join(repo, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    lines = sorted(glob.glob(os.path.join(repo, "profiles", "r*_bench.json")))
    assert lines and bench.pmc_traffic_file() is not None
    assert os.path.basename(lines[-1])[:3] == os.path.basename(bench.pmc_traffic_file())[:3], "bench line and traffic table of different rounds"
    roof = json.load(open(lines[-1]))["roofline"]
    for label in roof["per_kernel_ms_per_step"]:
        assert bench.pmc_traffic(label) is not None, f"{label}: no traffic entry in {bench.pmc_traffic_file()}"
    big = [k for k, ms in roof["per_kernel_ms_per_step"].items() if ms > 0.05]
    for label in big:
        assert bench.pmc_mfma(label) is not None, f"{label}: no MFMA counters in the committed pass"


def test_struct_layouts_match_header_sizes():
    from rift_amd import _ffi
    # 6 int32 + 26 pointers + 1 int32 (padded) ; 5 pointers ; 8 pointers + 2 floats ; 11 pointers
    assert ctypes.sizeof(_ffi.RiftFeatureBatch) == 24 + 26 * 8 + 8
    assert ctypes.sizeof(_ffi.RiftOutputs) == 40
    assert ctypes.sizeof(_ffi.RiftLossIn) == 72
    assert ctypes.sizeof(_ffi.RiftLossOut) == 88   # 11 pointers (incl. the optional f64 exchange buffer)
    assert ctypes.sizeof(_ffi.RiftTensorDesc) == 8 + 8 + 8 + 8 + 32


def test_ctypes_structs_match_the_header_as_a_c_compiler_lays_it_out(tmp_path):
    """include/rift_hip.h compiled by gcc as C: sizeof and every field offset of every struct the header defines, as the Python binding
    mirrors it (a ctypes Structure that drifts from the header corrupts arguments silently), and the size of every scalar C type of the
    generator's mapping table against the ctypes type it maps to."""
    import shutil
    import subprocess
    from rift_amd import _abi
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(repo, "include", "rift_hip.h")).read()
    structs = {n: c for n, c in vars(_abi).items() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure}
    assert set(structs) == set(re.findall(r"\}\s*(Rift\w+)\s*;", hdr)) and len(structs) == 13          # every `typedef struct { ... } Name;`
    scalars = _generator().SCALARS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rift_hip.h"', 'int main(void) {']
    for name, st in structs.items():
        lines.append(f'  printf("{name} %zu", sizeof({name}));')
        for field, *_ in st._fields_:
            lines.append(f'  printf(" %zu", offsetof({name}, {field}));')
        lines.append('  printf("\\n");')
    for c in scalars:
        lines.append(f'  printf("scalar:{c} %zu\\n", sizeof({c}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I", os.path.join(repo, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    assert len(out) == len(structs) + len(scalars)
    for line in out:
        name, size, *offs = line.split()
        if name.startswith("scalar:"):
            c = name.split(":", 1)[1]
            assert ctypes.sizeof(getattr(ctypes, scalars[c])) == int(size), (c, scalars[c], size)
            continue
        st = structs[name]
        assert ctypes.sizeof(st) == int(size), (name, ctypes.sizeof(st), size)
        assert [getattr(st, f).offset for f, *_ in st._fields_] == [int(o) for o in offs], name


def test_bound_signatures_match_a_table_written_from_the_header():
    """argtypes and restype of the loaded library against rows typed here by hand from include/rift_hip.h, independently of the generator:
    the entries where a slip is silent (a float where the header says double passes every CPU test and corrupts the argument)."""
    from rift_amd import _ffi, build
    build.build()
    lib = _ffi.load_library()
    vp, i, u32, f, d, P = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_float, ctypes.c_double, ctypes.POINTER
    table = {
        # ctx, rewards f64*, undones, values, next_values, unterminated, float gamma, float lambda_, int n, advantages, stream
        "rift_gae": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, f, f, i, vp, vp]),
        # ctx, rewards, dones, double gamma, int n, returns, stream
        "rift_discounted_return": (ctypes.c_int, [vp, vp, vp, d, i, vp, vp]),
        # ctx, out, int accumulate, float max_norm, total_norm, stream
        "rift_loss_finalize_clip": (ctypes.c_int, [vp, P(_ffi.RiftLossOut), i, f, vp, vp]),
        # ctx, rollout_center, int n_points, off_road_mask, int H, int W, double origin_x, origin_y, heading, res_x, res_y, off_x, off_y, off_road, stream
        "rift_off_road_matrix": (ctypes.c_int, [vp, vp, i, vp, i, i, d, d, d, d, d, d, d, vp, vp]),
        # ctx, batch, out, int flags, uint32_t seed, stream
        "rift_forward": (ctypes.c_int, [vp, P(_ffi.RiftFeatureBatch), P(_ffi.RiftOutputs), i, u32, vp]),
        # ctx, out, int accumulate, float max_norm, total_norm, int n_tensors, params, grads, exp_avg, exp_avg_sq, steps, lr, weight_decay,
        # double step_new, beta1, beta2, eps, stream
        "rift_update_tail": (ctypes.c_int, [vp, P(_ffi.RiftLossOut), i, f, vp, i, vp, vp, vp, vp, vp, vp, vp, d, d, d, d, vp]),
        # ctx, delta_dis, delta_angle, speed, acc, ang_vel, ang_acc, collision, int collision_ld, off_road, int off_road_ld, int G, int Ts,
        # params, returns, terms, stream
        "rift_rollout_return_ex": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i, vp, i, i, i, P(_ffi.RiftEvalParams), vp, vp, vp]),
        # ctx, trajectory, probability, ref_free_trajectory, int Rb, int Tfull, cbvs, int K, int topk, int sample_interval, pid_state,
        # int n_slots, decision, stream
        "rift_control_tick": (ctypes.c_int, [vp, vp, vp, vp, i, i, P(_ffi.RiftControlCBV), i, i, i, vp, i, vp, vp]),
        "rift_last_error": (ctypes.c_char_p, [vp]),
        "rift_ctx_destroy": (None, [vp]),
    }
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype)
        assert list(fn.argtypes) == argtypes, (name, fn.argtypes)
    # every other entry: bound, with the arity of its declaration
    gen = _generator()
    decls = gen.declarations(open(gen.HEADER).read())
    assert len(decls) == 53 == len(_ffi.EXPORTS) and [n for _, n, _ in decls] == list(_ffi.EXPORTS)
    for _, name, params in decls:
        assert len(getattr(lib, name).argtypes) == len(params), name


def test_generator_refuses_a_type_outside_its_table():
    """A parameter or field whose C type the mapping table does not hold is an error that names the declaration, not a guess."""
    gen = _generator()
    good = "typedef struct RiftCtx RiftCtx;\ntypedef struct RiftP { double a; const float* b; } RiftP;\nint rift_good(RiftCtx* ctx, const RiftP* p, float x);\n"
    text = gen.binding(good)
    assert '"rift_good": (C.c_int, [C.c_void_p, C.POINTER(RiftP), C.c_float])' in text
    with pytest.raises(ValueError, match=r"rift_bad, parameter x.*long double"):
        gen.binding(good + "int rift_bad(RiftCtx* ctx, long double x);\n")
    with pytest.raises(ValueError, match=r"rift_bad, parameter q.*RiftUnknown"):
        gen.binding(good + "int rift_bad(RiftCtx* ctx, const RiftUnknown* q);\n")
    with pytest.raises(ValueError, match=r"struct RiftQ, field n.*size_t"):
        gen.binding(good + "typedef struct RiftQ { size_t n; } RiftQ;\n")
    with pytest.raises(ValueError, match=r"RIFT_B"):
        gen.binding(good + "enum { RIFT_A = 1, RIFT_B };\n")


def test_stream_plan_orders_every_reader_behind_the_preparation(tmp_path):
    """csrc/fwd_plan.h (host-only) compiled by g++ and run over every combination of its inputs.  Checked against the placement table
    written out here, independently of the header's formulas: where the preparation, the history chain, the map chain and the late
    data-parallel mask fill run and which event waits are issued; that every stream carrying a reader of the preparation's outputs is
    the preparation's stream or reaches it through waits issued before that reader; that nothing forks while profiling, sizing or fp32."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bools = ["two_streams", "nat_fused", "nat_aside", "fp32", "prof_on", "dry", "prep_set", "dp_on"]
    outs = ["prefetched", "forked", "nat_aside", "prep_on", "history_on", "map_on", "dp_fill_on", "dp_fill_late", "side_waits_prep", "fork_from_main",
            "main_waits_prep", "join_once"]
    src = tmp_path / "plan.cpp"
    names = bools + ["side_gate"]
    src.write_text("\n".join(
        ['#include <cstdio>', '#include "fwd_plan.h"', 'int main() {', '  const int sizes[4] = {32, 64, 65, 256};',
         f'  for (int m = 0; m < {2 ** len(names)}; ++m) for (int s = 0; s < 4; ++s) {{', '    PlanIn in;']
        + [f'    in.{b} = (m >> {k}) & 1;' for k, b in enumerate(names)]
        + ['    in.bs = sizes[s];', '    const StreamPlan p = plan_streams(in);',
           '    printf("%d %d ' + " ".join(["%d"] * len(outs)) + '\\n", m, in.bs, ' + ", ".join(f"(int)p.{o}" for o in outs) + ');', '  }', '  return 0;', '}']))
    exe = tmp_path / "plan"
    subprocess.check_call([gxx, "-std=c++17", "-I", os.path.join(repo, "rift_amd", "csrc"), str(src), "-o", str(exe)])
    CALLER, PREPARE, SIDE = 0, 1, 2
    n = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        m, bs, *vals = map(int, line.split())
        i = {b: (m >> k) & 1 for k, b in enumerate(names)}
        i["bs"] = bs
        p = dict(zip(outs, vals))
        n += 1
        quiet = not (i["prof_on"] or i["dry"])
        forked = bool(i["two_streams"] and i["nat_fused"] and not i["fp32"] and quiet)
        prefetched = bool(i["prep_set"] and quiet)
        assert (p["forked"], p["prefetched"]) == (forked, prefetched), i
        if i["prof_on"] or i["dry"] or i["fp32"]:
            assert not p["forked"], i
        # ---- the placement table: (prep launch, side waits, history chain, map chain, caller waits before token assembly)
        side_waits, caller_waits = set(), set()
        if p["side_waits_prep"]: side_waits.add("ev_prep")
        if p["fork_from_main"]: side_waits.add("ev_fork")
        if p["join_once"]: side_waits.add("ev_join2")
        if p["main_waits_prep"]: caller_waits.add("ev_prep")
        if p["forked"]: caller_waits.add("ev_join")
        if p["nat_aside"] and not p["join_once"]: caller_waits.add("ev_join2")
        row = (p["prep_on"], side_waits, p["history_on"], p["map_on"], caller_waits)
        if not forked and not prefetched:
            want = (CALLER, set(), CALLER, CALLER, set())
        elif not forked:
            want = (PREPARE, set(), CALLER, CALLER, {"ev_prep"})
        elif not prefetched:
            want = (CALLER, {"ev_fork"}, CALLER, SIDE, {"ev_join"})
        elif i["side_gate"] > 0:
            want = (PREPARE, {"ev_prep", "ev_fork"}, CALLER, SIDE, {"ev_prep", "ev_join"})
        elif not i["nat_aside"]:
            want = (PREPARE, {"ev_prep"}, CALLER, SIDE, {"ev_prep", "ev_join"})
        elif i["bs"] > 64:
            want = (PREPARE, {"ev_prep"}, PREPARE, SIDE, {"ev_join", "ev_join2"} | ({"ev_prep"} if i["dp_on"] else set()))
        else:
            want = (PREPARE, {"ev_prep", "ev_join2"}, PREPARE, SIDE, {"ev_join"} | ({"ev_prep"} if i["dp_on"] else set()))
        assert row == want, (i, p)
        assert not p["nat_aside"] or (forked and prefetched), i
        # ---- the late mask fill: on the map chain's stream, and only with the preparation prefetched under data parallelism
        assert p["dp_fill_late"] == int(bool(i["dp_on"]) and prefetched), i
        assert p["dp_fill_on"] == (p["map_on"] if p["dp_fill_late"] else CALLER), i
        # ---- ordering: edges stream -> stream of the event waits.  ev_prep is recorded on the prepare stream behind the preparation and
        # ev_fork on the caller's behind whatever it holds by then: both precede the chains.  ev_join (side, behind the map chain) and
        # ev_join2 (prepare, behind the history chain) order the token assembly only.
        early = set()
        if p["side_waits_prep"]: early.add((PREPARE, SIDE))
        if p["fork_from_main"]: early.add((CALLER, SIDE))
        if p["main_waits_prep"]: early.add((PREPARE, CALLER))
        late = set(early)
        if p["forked"]: late.add((SIDE, CALLER))
        if p["nat_aside"]: late.add((PREPARE, SIDE) if p["join_once"] else (PREPARE, CALLER))

        def reaches(edges, dst):
            seen, todo = {p["prep_on"]}, [p["prep_on"]]
            while todo:
                s = todo.pop()
                for a, b in edges:
                    if a == s and b not in seen:
                        seen.add(b)
                        todo.append(b)
            return dst in seen
        assert reaches(early, p["history_on"]), ("history chain unordered", i, p)
        assert reaches(early, p["map_on"]), ("map chain unordered", i, p)
        if i["dp_on"]:
            assert reaches(early, p["dp_fill_on"]), ("mask fill unordered", i, p)
        assert reaches(late, CALLER), ("token assembly unordered", i, p)
    assert n == 2 ** 9 * 4


def test_kernel_plan_picks_one_consistent_path_per_stage(tmp_path):
    """csrc/fwd_kernels.h (host-only) compiled by g++ and run over its inputs, by groups of fields; every field of every row is compared
    with the table written out here, independently of the header's formulas, and the invariants that tie the stages together hold in
    every row.  A group crosses every input its fields read, directly or through another field, at the smallest shapes on both sides of
    every boundary (token slots 96 | 97, 112 | 113, 192 | 193; reference lines 8 | 9, 16 | 17; agents 256 | 257; static objects 0 | 1;
    scenes 84 | 85, 107 | 108, 128 | 129, 192 | 193; RIFT_DEC_DEFER unset, 0, 64; the eight-wave encoder build and a four-wave one).
    To keep the test at a few seconds, the group of the decoder's launches (`dec_now`, `dec_later`), which reads the shape only through
    `dec`, crosses all its inputs at four shapes -- the two sides of the tile | dense boundary, each with R = 8 and R = 17; the two groups
    before it check `dec` and the deferral at every boundary."""
    import shutil
    import subprocess
    import numpy as np
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B = (0, 1)
    default = dict(nat_fused=1, dec_fused=1, enc_fused=1, pe_fused=1, fo_fused=1, fpn_fused=1, ego_fused=1, heads_fused=1, pi_fused=1, fo_w=1, pe_w=1,
                   nat_compact=1, pe_live=1, pe_pack=1, rank_in_prep=1, enc112=1, dec_defer_max=-1, dec_split=1, dec_layers=4, dec_ts=0,
                   fp32=0, train=0, drop=0, need_traj=0, want_traj=0, defer_head=0, prof_on=0, forked=1, bs=32, A=64, Mp=20, S=0, R=4, enc_nw=8)
    ins = list(default)
    # token slots N = A + Mp + S with Mp = 20, S = 0: the agents carry the boundary
    slots = [n - 20 for n in (96, 97, 112, 113, 192, 193)]
    enc_dec = dict(enc_fused=B, dec_fused=B, enc112=B, fp32=B, enc_nw=(8, 4), A=slots, R=(8, 9, 16, 17))
    defer = dict(defer_head=B, prof_on=B, dec_ts=B, need_traj=B, dec_split=B, dec_defer_max=(-1, 0, 64), bs=(84, 85, 107, 108, 128, 129, 192, 193))
    groups = [
        dict(nat_fused=B, fpn_fused=B, nat_compact=B, rank_in_prep=B, ego_fused=B, fp32=B, A=(256, 257)),                       # history, ego
        dict(pe_fused=B, pe_w=B, pe_pack=B, pe_live=B, fo_fused=B, fo_w=B, fp32=B, train=B, forked=B, S=B),                   # PointsEncoders, Fourier, q0
        enc_dec,                                                                                                              # encoder, operand image, decoder path
        dict(enc_dec, **defer),                                                                                               # deferral and split
        dict(defer, dec_layers=(0, 2, 22, 4), drop=B, dec_fused=B, fp32=B, enc_fused=B, enc112=B, enc_nw=(8, 4), A=(76, 77), R=(8, 17)),      # the decoder's launches
        dict(heads_fused=B, pi_fused=B, fp32=B, need_traj=B, want_traj=B),                                                    # heads
    ]
    outs = ["hist_wave", "fpn_fused", "nat_compact", "rank_in_prep", "ego_fused", "pe", "pe_stats_persistent", "pe_pack", "pe_live", "fourier", "q0_early",
            "enc", "enc_image", "enc_kpm_x0p", "dec_kv_frag", "dec", "dec_n_now", "dec_now[0].l0", "dec_now[0].l1", "dec_now[1].l0", "dec_now[1].l1",
            "dec_defer", "dec_split", "dec_later.l0", "dec_later.l1", "pi_fused", "heads_fused", "head_traj"]
    code = ['#include <cstdio>', '#include <initializer_list>', '#include "fwd_kernels.h"', 'static void row(const KernelIn& in) {', '  const KernelPlan p = plan_kernels(in);',
            '  const short r[] = {' + ", ".join(f"(short)in.{k}" for k in ins) + ", " + ", ".join(f"(short)p.{o}" for o in outs) + '};',
            '  fwrite(r, sizeof(r), 1, stdout);', '}', 'int main() {']
    n_rows = 0
    for g in groups:
        code += ['  {', '    KernelIn in;'] + [f'    in.{k} = {v};' for k, v in default.items()]
        for k, vals in g.items():
            code.append(f'    for (int {k} : {{{", ".join(map(str, vals))}}}) {{ in.{k} = {k};')
        code.append('    row(in);' + ' }' * len(g))
        code.append('  }')
        n_rows += int(np.prod([len(v) for v in g.values()]))
    code += ['  return 0;', '}']
    src = tmp_path / "kplan.cpp"
    src.write_text("\n".join(code))
    exe = tmp_path / "kplan"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-I", os.path.join(repo, "rift_amd", "csrc"), str(src), "-o", str(exe)])
    t = np.ascontiguousarray(np.frombuffer(subprocess.check_output([str(exe)]), dtype=np.int16).reshape(-1, len(ins) + len(outs)).T)
    assert t.shape[1] == n_rows
    i = {k: (t[j] != 0 if default[k] in (0, 1) and k != "S" else t[j]) for j, k in enumerate(ins)}      # flags as booleans, numbers as they are
    p = {o: t[len(ins) + j] for j, o in enumerate(outs)}
    N, R, bs, bf = i["A"] + i["Mp"] + i["S"], i["R"], i["bs"], ~i["fp32"]

    def same(name, want):
        bad = np.flatnonzero(p[name] != np.asarray(want).astype(np.int16))
        assert bad.size == 0, (name, {k: int(t[j][bad[0]]) for j, k in enumerate(ins)}, int(p[name][bad[0]]))

    # ---- the table.  History: wave-private levels in the 16-bit mode; the fused FPN tail only behind them; compaction only with both; the
    # in-launch ranking only with compaction and up to 256 agents
    wave = i["nat_fused"] & bf
    same("hist_wave", wave); same("fpn_fused", wave & i["fpn_fused"]); same("nat_compact", wave & i["fpn_fused"] & i["nat_compact"])
    same("rank_in_prep", wave & i["fpn_fused"] & i["nat_compact"] & i["rank_in_prep"] & (i["A"] <= 256))
    same("ego_fused", bf & i["ego_fused"])
    # ---- PointsEncoders: 0 layer-wise, 1 pair + pe_mid_kernel, 2 pair + pe_w_kernel
    LAYERWISE = 0
    pe = np.select([i["fp32"] | ~i["pe_fused"], i["pe_w"]], [LAYERWISE, 2], 1)
    same("pe", pe); same("pe_stats_persistent", (pe == 2) & i["train"]); same("pe_pack", (pe == 2) & i["pe_pack"])
    same("pe_live", (pe == 2) & i["train"] & i["pe_live"])
    # ---- Fourier: 0 layer-wise, 1 one launch per embedding, 2 three in one by fourier_fused_kernel, 3 three in one by fo_w_kernel
    fo = np.select([i["fp32"] | ~i["fo_fused"], (pe == LAYERWISE) | (i["S"] > 0), i["fo_w"]], [LAYERWISE, 1, 3], 2)
    same("fourier", fo); same("q0_early", i["forked"] & (fo >= 2))
    # ---- scene encoder: 0 layer-wise, 1 fused on 96 rows, 2 fused on 112 rows, 3 enc_w_kernel.  Image: 0 none, 1 key tiles, 2 dense
    tail = i["dec_fused"] & (R <= 8) & (i["enc_nw"] == 8)
    enc = np.select([i["fp32"] | ~i["enc_fused"], N <= 96, (N <= 112) & i["enc112"] & tail, N <= 192], [LAYERWISE, 1, 2, 3], LAYERWISE)
    img = np.select([(enc == 1) & tail, enc == 2, (enc == 3) & i["dec_fused"] & (R <= 16)], [1, 2, 2], 0)
    same("enc", enc); same("enc_image", img); same("enc_kpm_x0p", (img > 0) & (enc != 3))
    # ---- decoder: 0 layer-wise, 1 fused on key tiles, 2 fused dense.  The kernel takes R <= 8 and N <= 96 from the encoder's tile image
    # only, and every other shape up to R = 16, N = 192 from a dense image
    small = (R <= 8) & (N <= 96)
    dec = np.select([i["fp32"] | ~i["dec_fused"], small & (img == 1), ~small & (R <= 16) & (N <= 192)], [LAYERWISE, 1, 2], LAYERWISE)
    same("dec", dec); same("dec_kv_frag", (dec == 2) & (img == 0))
    # ---- deferral: the measured table of batch sizes, by value (without / with the trajectory heads), or RIFT_DEC_DEFER
    wins = {False: {84: 1, 85: 0, 107: 0, 108: 1, 128: 1, 129: 1, 192: 1, 193: 0, 32: 1}, True: {84: 1, 85: 1, 107: 1, 108: 1, 128: 1, 129: 0, 192: 0, 193: 0, 32: 1}}
    table = np.array([wins[bool(tr)][int(b)] for tr, b in zip(i["need_traj"], bs)], dtype=bool)
    size_ok = np.where(i["dec_defer_max"] < 0, table, bs <= i["dec_defer_max"])
    defer_ = (dec != LAYERWISE) & i["defer_head"] & size_ok & ~i["prof_on"] & ~i["dec_ts"]
    split = defer_ & i["dec_split"] & ~i["need_traj"]
    same("dec_defer", defer_); same("dec_split", split)
    # ---- the decoder's launches: (number now, first range, second range, the deferred range)
    two = ~defer_ & (i["dec_layers"] == 22) & (dec != LAYERWISE) & ~i["drop"]
    want = np.zeros((7, n_rows), dtype=np.int64)
    want[:] = np.array([1, 0, 4, 0, 0, 0, 0])[:, None]                                  # all four layers, one launch
    for cond, vals in ((i["dec_layers"] == 0, [0, 0, 0, 0, 0, 0, 0]), (i["dec_layers"] == 2, [1, 0, 2, 0, 0, 0, 0]), (two, [2, 0, 2, 2, 4, 0, 0]),
                       (defer_, [0, 0, 0, 0, 0, 0, 4]), (split, [1, 0, 2, 0, 0, 2, 4])):       # (later rows override earlier ones)
        want[:, cond] = np.array(vals)[:, None]
    for j, name in enumerate(["dec_n_now", "dec_now[0].l0", "dec_now[0].l1", "dec_now[1].l0", "dec_now[1].l1", "dec_later.l0", "dec_later.l1"]):
        same(name, want[j])
    # ---- heads
    same("pi_fused", bf & i["pi_fused"]); same("heads_fused", bf & i["heads_fused"]); same("head_traj", i["need_traj"] & i["want_traj"])

    # ---- invariants, in all rows
    def holds(cond, what):
        bad = np.flatnonzero(~np.asarray(cond, dtype=bool))
        assert bad.size == 0, (what, {k: int(t[j][bad[0]]) for j, k in enumerate(ins)})
    q = {k: v != 0 for k, v in p.items()}          # (the plan's flags as booleans; the enums and layer numbers are read from p)
    f32 = i["fp32"]
    holds(~f32 | ((p["hist_wave"] + p["fpn_fused"] + p["nat_compact"] + p["rank_in_prep"] + p["ego_fused"] + p["pe"] + p["fourier"] + p["enc"] + p["enc_image"]
                   + p["dec_kv_frag"] + p["dec"] + p["dec_defer"] + p["dec_split"] + p["pi_fused"] + p["heads_fused"] + p["pe_pack"] + p["pe_live"]
                   + p["pe_stats_persistent"] + p["q0_early"]) == 0), "fp32: every stage layer-wise, nothing compacted, decoder not deferred")
    makers = (p["enc_image"] > 0).astype(int) + p["dec_kv_frag"]
    holds((p["dec"] == 0) | (makers == 1), "fused decoder: exactly one producer of the K | V^T image")
    holds((p["dec"] != 1) | ((p["enc_image"] == 1) & (N <= 96) & (R <= 8)), "tile variant: the encoder's tile image, N <= 96, R <= 8")
    holds((p["dec"] != 2) | (p["enc_image"] == 2) | q["dec_kv_frag"], "dense variant: a dense image")
    holds((p["enc_image"] != 2) | (p["enc"] == 2) | (p["enc"] == 3), "dense image from the wide encoder or enc_w_kernel")
    holds((p["enc_image"] != 1) | (p["enc"] == 1), "tile image from the 96-row encoder")
    holds((p["dec"] != 0) | (makers == 0), "layer-wise decoder: nobody makes the image")
    holds(~q["enc_kpm_x0p"] | (p["enc_image"] > 0), "kpm_c and x0p only with an image")
    holds(~q["nat_compact"] | (q["hist_wave"] & q["fpn_fused"]), "nat_compact => wave-private history and fused FPN")
    holds(~q["rank_in_prep"] | (q["nat_compact"] & (i["A"] <= 256)), "rank_in_prep => nat_compact and A <= 256")
    holds((p["fourier"] < 2) | ((p["pe"] > 0) & (i["S"] == 0)), "three-in-one Fourier => the pair and S = 0")
    holds(~q["q0_early"] | (i["forked"] & (p["fourier"] >= 2)), "q0_early => forked and that launch")
    holds(~q["dec_defer"] | (i["defer_head"] & (p["dec"] > 0) & ~i["prof_on"]), "dec_defer => defer_head, fused decoder, not profiling")
    holds(~q["dec_split"] | (q["dec_defer"] & ~i["need_traj"]), "dec_split => dec_defer and no trajectory heads")
    holds(~(q["pe_pack"] | q["pe_live"] | q["pe_stats_persistent"]) | (p["pe"] == 2), "pe_pack, pe_live, persistent statistics => pe_w_kernel")
    # every layer of a fused decoder that is not cut short by RIFT_DEC_LAYERS runs exactly once, now or later
    full = (p["dec"] > 0) & (q["dec_defer"] | ((i["dec_layers"] != 0) & (i["dec_layers"] != 2)))
    ran = (p["dec_now[0].l1"] - p["dec_now[0].l0"]) + (p["dec_now[1].l1"] - p["dec_now[1].l0"]) + (p["dec_later.l1"] - p["dec_later.l0"])
    holds(~full | (ran == 4), "four decoder layers in all")


def test_product_package_never_touches_the_oracle():
    """oracle/ is test infrastructure: nothing under rift_amd/ may import or reference it."""
    import pathlib
    repo = pathlib.Path(__file__).resolve().parents[1]
    offenders = []
    for root in (repo / "rift_amd", repo / "tools"):          # tools/: profiling / micro-benchmarks of the product, same rule
        for f in list(root.rglob("*.py")) + list(root.rglob("*.h")) + list(root.rglob("*.hip")) + list(root.rglob("*.sh")):
            txt = f.read_text()
            if "import oracle" in txt or "from oracle" in txt or "oracle/" in txt:
                offenders.append(str(f))
    assert not offenders, offenders
    # bench.py and __graft_entry__.py may use it only inside cpu_baseline() / smoke()
    import ast
    for name, allowed in (("bench.py", {"cpu_baseline"}), ("__graft_entry__.py", {"smoke"})):
        tree = ast.parse((repo / name).read_text())
        for fn in [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.Module))]:
            for node in (fn.body if isinstance(fn, ast.Module) else []):
                if isinstance(node, (ast.Import, ast.ImportFrom)):
                    mod = node.module if isinstance(node, ast.ImportFrom) else ",".join(a.name for a in node.names)
                    assert "oracle" not in (mod or ""), f"{name}: module-level oracle import"
        for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
            uses = any(isinstance(n, (ast.Import, ast.ImportFrom)) and "oracle" in ((n.module if isinstance(n, ast.ImportFrom) else ",".join(a.name for a in n.names)) or "")
                       for n in ast.walk(fn))
            assert not uses or fn.name in allowed, f"{name}: {fn.name} imports the oracle"


def test_scene_dump_round_trip(tmp_path):
    """save_scenes / load_scenes (the dump format BASELINE config 0's "pre-dumped rollout scenes" needs): 8 ragged scenes come back with
    identical keys, dtypes, shapes and values, and collate to the same padded batch."""
    from rift_amd import synthetic as syn
    from rift_amd.replay import load_scenes, save_scenes
    scenes = [syn.make_scene(900 + i, num_agents=10 + i, num_polygons=6 + (i % 3), r_min=1, r_max=4) for i in range(8)]
    path = str(tmp_path / "replay.npz")
    save_scenes(path, scenes)
    back = load_scenes(path)
    assert len(back) == 8

    def same(a, b, where):
        if isinstance(a, dict):
            assert set(a) == set(b), where
            for k in a:
                same(a[k], b[k], f"{where}/{k}")
        else:
            a, b = torch.as_tensor(a), torch.as_tensor(b)
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where

    for i, (s, t) in enumerate(zip(scenes, back)):
        same(s["feature"], t["feature"], f"scene {i} feature")
        same(s["extras"], t["extras"], f"scene {i} extras")
    b0 = syn.collate_features([s["feature"] for s in scenes])
    b1 = syn.collate_features([s["feature"] for s in back])
    same(b0, b1, "collated batch")
    with pytest.raises(ValueError):
        import numpy as np
        np.savez(str(tmp_path / "other.npz"), x=np.zeros(3))
        load_scenes(str(tmp_path / "other.npz"))
