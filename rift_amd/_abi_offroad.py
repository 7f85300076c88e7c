"""The ctypes mirror of include/rift_offroad.h, the off-road-extent extension of the C-ABI (three `riftof_*` entries, one struct, one
enumeration).

Written by hand with the type table of tools/gen/abi_trampolines.py (int / int32_t -> c_int32, double -> c_double, a pointer to a struct ->
POINTER(it), every other pointer -> c_void_p), as rift_amd/_abi_footprint.py is; tests/test_offroad_abi_host.py compiles the header and holds
this file to it: names, arity, every argument type, the struct's size and field offsets, the enumerators, and the symbols the library
exports.
"""
import ctypes as C

from rift_amd._abi import RiftEvalParams, RiftTickCBV
from rift_amd._abi_footprint import RiftCollisionParams

RIFTOF_CENTER, RIFTOF_FOOTPRINT = 0, 1


class RiftOffRoadParams(C.Structure):
    _fields_ = [("extent", C.c_int32),
                ("reserved", C.c_int32)]


_vp, _i, _d = C.c_void_p, C.c_int32, C.c_double

# name -> (restype, [argtypes]) of every function the header declares, in header order
SIGNATURES = {
    "riftof_params_default": (C.c_int, [C.POINTER(RiftOffRoadParams)]),
    "riftof_off_road_matrix": (C.c_int, [_vp, _vp, _vp, _i, _vp, _i, _i, _d, _d, _d, C.POINTER(RiftEvalParams), C.POINTER(RiftOffRoadParams),
                                         _vp, _vp, _vp]),
    "riftof_group_advantage_tick": (C.c_int, [_vp, _vp, _i, _i, C.POINTER(RiftTickCBV), _i, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(RiftEvalParams),
                                              C.POINTER(RiftCollisionParams), C.POINTER(RiftOffRoadParams), _vp, _vp, _vp, _vp]),
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
