"""The ctypes mirror of include/rift_drivable.h, the drivable-area-map extension of the C-ABI (six `riftdm_*` entries and one struct).

Written by hand with the type table of tools/gen/abi_trampolines.py (int / int32_t -> c_int32, int64_t -> c_int64, double -> c_double, a
pointer to a struct -> POINTER(it), every other pointer -> c_void_p); tests/test_drivable_abi_host.py compiles the header and holds this
file to it: names, arity, every argument type, the struct's size and field offsets, and the symbols the library exports.
"""
import ctypes as C

from rift_amd._abi import RiftEvalParams, RiftTickCBV


class RiftDrivableInfo(C.Structure):
    _fields_ = [("n_polys", C.c_int32),
                ("n_vertices", C.c_int32),
                ("nx", C.c_int32),
                ("ny", C.c_int32),
                ("max_cell_list", C.c_int32),
                ("reserved", C.c_int32),
                ("cell", C.c_double),
                ("margin", C.c_double),
                ("x0", C.c_double),
                ("y0", C.c_double),
                ("device_bytes", C.c_int64)]


_vp, _i, _d = C.c_void_p, C.c_int32, C.c_double
_TICK = [_vp, _vp, _i, _i, C.POINTER(RiftTickCBV), _i, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(RiftEvalParams), _vp, _vp, _vp, _vp]

# name -> (restype, [argtypes]) of every function the header declares, in header order
SIGNATURES = {
    "riftdm_load": (C.c_int, [_vp, _vp, _vp, _i, _d, _d, _vp]),
    "riftdm_clear": (C.c_int, [_vp]),
    "riftdm_info": (C.c_int, [_vp, C.POINTER(RiftDrivableInfo)]),
    "riftdm_off_road_matrix": (C.c_int, [_vp, _vp, _i, _i, _i, _d, _d, _d, C.POINTER(RiftEvalParams), _vp, _vp]),
    "riftdm_raster": (C.c_int, [_vp, _i, _i, _d, _d, _d, C.POINTER(RiftEvalParams), _vp, _vp]),
    "riftdm_group_advantage_tick": (C.c_int, _TICK),
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
