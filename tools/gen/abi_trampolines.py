"""Generates rift_amd/csrc/abi_list.h, rift_amd/csrc/abi.cpp and rift_amd/_abi.py from include/rift_hip.h.

librift_hip.so carries two builds of the engine -- bf16 and fp16 MFMA operands (csrc/opfmt.h) -- and ONE set of exported `rift_*`
symbols.  An exported function whose entry depends on the build (context, model load, forward, streams, profiler, taps) is a trampoline
that reads the operand format a context was created with (RiftCtxCore::opfmt, csrc/ctx_core.h) and calls the same entry point
of the build that owns the context through that build's RiftVTable (csrc/abi_table.h: the RIFT_FN list of abi_list.h).  The entries that
do not depend on the operand format (FORMAT_FREE below) exist once per library (csrc/shared.hip, namespace rift::abi): their trampolines
null-check the context and call them directly, and abi_list.h names them in a second list, RIFT_SHARED_FN.  The trampolines are derived
from the declarations of the header, so the header stays the single statement of the interface (tests/test_host_api.py regenerates the
files and compares).

rift_amd/_abi.py is the Python side of the same statement: the header's enumerators and integer #defines as ints, one ctypes.Structure
per `typedef struct`, SIGNATURES (name -> restype, argtypes) and bind(lib).  One table maps the types: int / int32_t -> c_int32,
uint32_t -> c_uint32, int64_t -> c_int64, float -> c_float, double -> c_double, uint8_t -> c_uint8; a pointer to a struct of the header ->
POINTER(it); char* -> c_char_p; every other pointer -> c_void_p (the type alone cannot tell a device pointer from a host array).  A type
outside the table is an error that names the declaration.

    python tools/gen/abi_trampolines.py          # rewrites the three files in place
    python tools/gen/abi_trampolines.py --check  # exit status 1 when one of them differs
"""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(REPO, "include", "rift_hip.h")
OUT_LIST = os.path.join(REPO, "rift_amd", "csrc", "abi_list.h")
OUT_CPP = os.path.join(REPO, "rift_amd", "csrc", "abi.cpp")
OUT_PY = os.path.join(REPO, "rift_amd", "_abi.py")

# entry points the trampoline file implements by hand (they create a context / work without one)
SPECIAL = {"rift_ctx_create", "rift_ctx_create_ex", "rift_ctx_operand_format", "rift_ctx_destroy", "rift_last_error"}
# entry points without a context that are the same in every build: implemented once, in the trampoline file, from a host-only header
NO_CTX = ("rift_ctx_create_ex", "rift_ctx_operand_format", "rift_objective_params_default")
# entry points that depend on no operand format: defined once per library in csrc/shared.hip, called without a table
FORMAT_FREE = ("rift_loss_backward", "rift_loss_backward_ex", "rift_head_backward", "rift_loss_finalize", "rift_loss_finalize_clip", "rift_update_tail",
               "rift_clip_grad_norm", "rift_adamw_step", "rift_critic_forward", "rift_critic_loss_backward", "rift_critic_finalize", "rift_critic_backward",
               "rift_gae", "rift_discounted_return", "rift_normalize_advantage", "rift_group_advantage", "rift_rollout", "rift_rollout_return",
               "rift_rollout_return_ex", "rift_ref_line_info", "rift_other_vehicle_rollout", "rift_collision_matrix", "rift_off_road_matrix",
               "rift_group_advantage_tick", "rift_group_advantage_tick_ex", "rift_control_tick", "rift_collate", "rift_sft_teacher_mode",
               "rift_eval_params_default")


def strip_comments(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def declarations(text):
    """[(return type, name, [(param type, param name)])] of every `rift_*` function the header declares."""
    text = strip_comments(text)
    out = []
    for m in re.finditer(r"^(int|void|const char\*)\s+(rift_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        params = []
        for a in [x.strip() for x in args.split(",")]:
            pm = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a)
            params.append((pm.group(1).strip(), pm.group(2)))
        out.append((ret, name, params))
    return out


SCALARS = {"int": "c_int32", "int32_t": "c_int32", "uint32_t": "c_uint32", "int64_t": "c_int64", "float": "c_float", "double": "c_double",
           "uint8_t": "c_uint8"}
POINTEES = set(SCALARS) | {"void", "char", "int8_t"}          # what a `c_void_p` may point to, beside the header's own types
RETURNS = {"int": "C.c_int", "void": "None", "const char*": "C.c_char_p"}


def ctype(typ, known, where):
    """The ctypes spelling of one C type of the header (the table of the module docstring); `known`: the header's own type names ->
    "struct" | "opaque" | "fn".  A type outside the table raises, naming the declaration `where`."""
    base = " ".join(t for t in typ.replace("*", " ").split() if t != "const")
    stars = typ.count("*")
    if stars == 0 and base in SCALARS:
        return "C." + SCALARS[base]
    if stars == 0 and known.get(base) in ("struct", "fn"):
        return base
    if stars == 1 and known.get(base) == "struct":
        return f"C.POINTER({base})"
    if stars == 1 and base == "char":
        return "C.c_char_p"
    if stars >= 1 and (base in POINTEES or base in known):
        return "C.c_void_p"
    raise ValueError(f"{where}: no ctypes mapping for the C type `{typ}`")


def binding(text=None):
    """The text of rift_amd/_abi.py for the header `text` (default: include/rift_hip.h): constants, structs, SIGNATURES and bind()."""
    text = strip_comments(open(HEADER).read() if text is None else text)
    out = ['"""GENERATED by tools/gen/abi_trampolines.py from include/rift_hip.h -- do not edit.',
           "", "The ctypes mirror of the C-ABI: the header's constants, structs and function signatures; bind(lib) applies them to a loaded library.",
           '"""', "import ctypes as C", ""]
    consts = []          # (name, value) of every enumerator and every integer #define, in header order
    for m in re.finditer(r"\benum\s*\{([^}]*)\}\s*;|^[ \t]*#define[ \t]+(RIFT_\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M):
        if m.group(2):
            consts.append((m.group(2), m.group(3)))
            continue
        for e in filter(None, (x.strip() for x in m.group(1).split(","))):
            em = re.fullmatch(r"(RIFT_\w+)\s*=\s*(-?\d+)", e)
            if not em:
                raise ValueError(f"enum {{ {' '.join(m.group(1).split())} }}: enumerator `{e}` is not NAME = integer")
            consts.append((em.group(1), em.group(2)))
    out += [f"{name} = {value}" for name, value in consts] + ["", ""]
    # the header's own types, in header order: opaque handles, structs, function-pointer typedefs
    types = sorted([(m.start(), "opaque", m) for m in re.finditer(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;", text)]
                   + [(m.start(), "struct", m) for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, re.S)]
                   + [(m.start(), "fn", m) for m in re.finditer(r"typedef\s+(\w+)\s*\(\s*\*\s*(\w+)\s*\)\s*\(([^)]*)\)\s*;", text)], key=lambda t: t[0])
    known = {}
    for _, kind, m in types:
        if kind == "opaque":
            known[m.group(2)] = kind
        elif kind == "fn":
            ret, name, params = m.group(1), m.group(2), [p.strip() for p in m.group(3).split(",")]
            args = [ctype(re.match(r"^(.*?)\w+$", p).group(1), known, f"typedef {name}") for p in params]
            out += [f"{name} = C.CFUNCTYPE({', '.join([ctype(ret, known, f'typedef {name}')] + args)})", "", ""]
            known[name] = kind
        else:
            name, body = m.group(3), m.group(2)
            fields = []
            for stmt in filter(None, (" ".join(s.split()) for s in body.split(";"))):
                sm = re.match(r"^((?:const )?\w+)\s*(.*)$", stmt)          # `const float` | `*a, *b` or `a[4]`
                for d in sm.group(2).split(",") if sm else [""]:
                    dm = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[(\d+)\])?\s*", d)
                    if not dm:
                        raise ValueError(f"struct {name}: cannot read the field declaration `{stmt}`")
                    t = ctype(sm.group(1) + dm.group(1), known, f"struct {name}, field {dm.group(2)}")
                    fields.append(f'("{dm.group(2)}", {t} * {dm.group(3)})' if dm.group(3) else f'("{dm.group(2)}", {t})')
            out += [f"class {name}(C.Structure):", "    _fields_ = [" + ",\n                ".join(fields) + "]", "", ""]
            known[name] = kind
    out += ["# name -> (restype, [argtypes]) of every function the header declares, in header order", "SIGNATURES = {"]
    for ret, name, params in declarations(text):
        args = [ctype(t, known, f"{name}, parameter {n}") for t, n in params]
        out.append(f'    "{name}": ({RETURNS[ret]}, [{", ".join(args)}]),')
    out += ["}", "EXPORTS = list(SIGNATURES)", "", "",
            "def bind(lib):", '    """Check that `lib` exports every function of the header and set its argtypes / restype."""',
            "    for name in EXPORTS:", "        if not hasattr(lib, name):",
            '            raise RuntimeError(f"librift_hip.so does not export {name}")',
            "    for name, (restype, argtypes) in SIGNATURES.items():", "        fn = getattr(lib, name)",
            "        fn.argtypes, fn.restype = argtypes, restype", "    return lib"]
    return "\n".join(out) + "\n"


def render():
    text = open(HEADER).read()
    decls = declarations(text)
    assert set(FORMAT_FREE) <= {d[1] for d in decls}, set(FORMAT_FREE) - {d[1] for d in decls}
    per_build = [d for d in decls if d[1] not in NO_CTX and d[1] not in FORMAT_FREE]
    shared = [d for d in decls if d[1] in FORMAT_FREE]
    lst = ["// GENERATED by tools/gen/abi_trampolines.py from include/rift_hip.h -- two X-macro lists; define one or both macros before including.",
           "// RIFT_FN(name): the entry points every engine build implements (its RiftVTable).",
           "#ifdef RIFT_FN"]
    lst += [f"RIFT_FN({name})" for _, name, _ in per_build]
    lst += ["#endif", "// RIFT_SHARED_FN(name): the operand-format-free entry points, defined once per library (shared.hip: rift::abi).", "#ifdef RIFT_SHARED_FN"]
    lst += [f"RIFT_SHARED_FN({name})" for _, name, _ in shared]
    lst += ["#endif"]
    cpp = ["// GENERATED by tools/gen/abi_trampolines.py from include/rift_hip.h -- do not edit.",
           "// The exported C-ABI of librift_hip.so: trampolines onto the engine build (bf16 / fp16 MFMA operands, csrc/opfmt.h) that owns the context.",
           "#include <stdlib.h>",
           "#include <string.h>",
           "",
           '#include "abi_table.h"',
           '#include "ctx_core.h"',
           '#include "objective_params.h"',
           "",
           'extern "C" const RiftVTable rift_vtable_bf16;',
           "#if defined(RIFT_ABI_BF16_ONLY)      // the diagnostic library (build.py: build_stats) carries the bf16-operand build only",
           "#define RIFT_VT_FP16 (static_cast<const RiftVTable*>(nullptr))",
           "#else",
           'extern "C" const RiftVTable rift_vtable_fp16;',
           "#define RIFT_VT_FP16 (&rift_vtable_fp16)",
           "#endif",
           "",
           "// the operand-format-free entries (shared.hip), declared with the types of the header",
           "namespace rift { namespace abi {",
           "#define RIFT_SHARED_FN(name) decltype(::name) name;",
           '#include "abi_list.h"',
           "#undef RIFT_SHARED_FN",
           "}}",
           "",
           "// the operand format a context was created with (ctx_core.h: RiftCtxCore, the one definition of the handle)",
           "static inline const RiftVTable& vt(const RiftCtx* ctx) {",
           "  return (ctx->opfmt == RIFT_OPERANDS_FP16 && RIFT_VT_FP16) ? *RIFT_VT_FP16 : rift_vtable_bf16;",
           "}",
           "",
           'extern "C" {',
           "",
           "int rift_ctx_create_ex(int device, int operand_format, RiftCtx** ctx) {",
           "  if (operand_format == RIFT_OPERANDS_BF16) return rift_vtable_bf16.rift_ctx_create(device, ctx);",
           "  if (operand_format == RIFT_OPERANDS_FP16 && RIFT_VT_FP16) return RIFT_VT_FP16->rift_ctx_create(device, ctx);",
           "  return RIFT_ERR_ARG;",
           "}",
           "",
           "// RIFT_OPERANDS=fp16 selects the fp16-operand build for hosts that do not call rift_ctx_create_ex; the default is bf16",
           "int rift_ctx_create(int device, RiftCtx** ctx) {",
           '  const char* ev = getenv("RIFT_OPERANDS");',
           '  return rift_ctx_create_ex(device, ev && strcmp(ev, "fp16") == 0 ? RIFT_OPERANDS_FP16 : RIFT_OPERANDS_BF16, ctx);',
           "}",
           "",
           "int rift_ctx_operand_format(RiftCtx* ctx) { return ctx ? ctx->opfmt : RIFT_ERR_ARG; }",
           "",
           "void rift_ctx_destroy(RiftCtx* ctx) { if (ctx) vt(ctx).rift_ctx_destroy(ctx); }",
           "",
           'const char* rift_last_error(RiftCtx* ctx) { return ctx ? vt(ctx).rift_last_error(ctx) : "null context"; }',
           "",
           "int rift_objective_params_default(int kind, RiftObjectiveParams* out) {",
           "  return out && rift_objective_params_set_default(kind, out) ? RIFT_OK : RIFT_ERR_ARG;",
           "}",
           ""]
    for ret, name, params in [d for d in decls if d[1] not in NO_CTX]:
        if name in SPECIAL:
            continue
        assert params[0][1] == "ctx" and ret == "int", name
        sig = ", ".join(f"{t} {n}" for t, n in params)
        call = ", ".join(n for _, n in params)
        cpp.append(f"{ret} {name}({sig}) {{")
        cpp.append(f"  if (!ctx) return RIFT_ERR_ARG;")
        cpp.append(f"  return {'rift::abi::' if name in FORMAT_FREE else 'vt(ctx).'}{name}({call});")
        cpp.append("}")
        cpp.append("")
    cpp.append('}  // extern "C"')
    return "\n".join(lst) + "\n", "\n".join(cpp) + "\n"


if __name__ == "__main__":
    files = list(zip((OUT_LIST, OUT_CPP, OUT_PY), render() + (binding(),)))
    if len(sys.argv) > 1 and sys.argv[1] == "--check":
        sys.exit(0 if all(os.path.exists(p) and open(p).read() == t for p, t in files) else 1)
    for p, t in files:
        open(p, "w").write(t)
