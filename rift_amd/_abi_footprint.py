"""The ctypes mirror of include/rift_footprint.h, the collision-test extension of the C-ABI (three `riftfp_*` entries, one struct, one
enumeration).

Written by hand with the type table of tools/gen/abi_trampolines.py (int / int32_t -> c_int32, double -> c_double, a pointer to a struct ->
POINTER(it), every other pointer -> c_void_p), as rift_amd/_abi_select.py is; tests/test_footprint_abi_host.py compiles the header and holds
this file to it: names, arity, every argument type, the struct's size and field offsets, the enumerators, and the symbols the library
exports.
"""
import ctypes as C

from rift_amd._abi import RiftEvalParams, RiftTickCBV

RIFTFP_ENVELOPE, RIFTFP_FOOTPRINT = 0, 1


class RiftCollisionParams(C.Structure):
    _fields_ = [("mode", C.c_int32),
                ("reserved", C.c_int32)]


_vp, _i = C.c_void_p, C.c_int32

# name -> (restype, [argtypes]) of every function the header declares, in header order
SIGNATURES = {
    "riftfp_params_default": (C.c_int, [C.POINTER(RiftCollisionParams)]),
    "riftfp_collision_matrix": (C.c_int, [_vp, _vp, _i, _i, _vp, _i, _i, C.POINTER(RiftCollisionParams), _vp, _vp, _vp]),
    "riftfp_group_advantage_tick": (C.c_int, [_vp, _vp, _i, _i, C.POINTER(RiftTickCBV), _i, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(RiftEvalParams),
                                              C.POINTER(RiftCollisionParams), _vp, _vp, _vp, _vp]),
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
