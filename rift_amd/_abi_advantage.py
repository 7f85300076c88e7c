"""The ctypes mirror of include/rift_advantage.h, the arena-advantage extension of the C-ABI (two `riftga_*` entries, one struct, two
enumerations).

Written by hand with the type table of tools/gen/abi_trampolines.py (int / int32_t -> c_int32, double -> c_double, a pointer to a struct ->
POINTER(it), every other pointer -> c_void_p), as rift_amd/_abi_drivable.py is; tests/test_advantage_param_cases.py compiles the header and
holds this file to it: names, arity, every argument type, the struct's size and field offsets, the enumerators, and the symbols the
library exports.
"""
import ctypes as C

RIFTGA_BASELINE_MEAN, RIFTGA_BASELINE_LEAVE_ONE_OUT, RIFTGA_BASELINE_NONE = 0, 1, 2
RIFTGA_SCALE_GROUP_STD, RIFTGA_SCALE_BATCH_RMS, RIFTGA_SCALE_NONE = 0, 1, 2


class RiftAdvantageParams(C.Structure):
    _fields_ = [("baseline", C.c_int32),
                ("scale", C.c_int32),
                ("eps", C.c_double),
                ("clip", C.c_double)]


_vp, _i = C.c_void_p, C.c_int32

# name -> (restype, [argtypes]) of every function the header declares, in header order
SIGNATURES = {
    "riftga_params_default": (C.c_int, [C.POINTER(RiftAdvantageParams)]),
    "riftga_arena_advantage": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, C.POINTER(RiftAdvantageParams), _vp, _vp, _vp]),
}
EXPORTS = list(SIGNATURES)


def bind(lib):
    """Check that `lib` exports every function of the header and set its argtypes / restype."""
    for name, (restype, argtypes) in SIGNATURES.items():
        if not hasattr(lib, name):
            raise RuntimeError(f"librift_hip.so does not export {name}")
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    return lib
