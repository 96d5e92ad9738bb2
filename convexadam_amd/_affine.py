"""ctypes binding of the affine model (include/convexadam_affine.h) onto the handle _lib.lib() returns.

A table of its own, as _prep.py and _field.py have, typed by _lib.bind: _lib.SIGNATURES mirrors include/convexadam_hip.h name for name, AFFINE_SIGNATURES mirrors
include/convexadam_affine.h the same way (tests/test_affine_abi.py).  All headers describe the one libconvexadam_hip.so; CVX_ABI_VERSION is
unchanged."""
import ctypes as C
import functools

from . import _lib

_vp, _i, _i64, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
_FIELD = [_vp, _i, _i64, _i64]          # pointer, elements are double, component stride, voxel stride

# name -> (restype, argtypes)
AFFINE_SIGNATURES = {
    "cvx_affine_lts_workspace_bytes": (_sz, [_i64]),
    "cvx_affine_lts_f32": (_i, [_vp, _i, _vp, _i, _i64, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "cvx_affine_field_f64": (_i, [_vp, _i, _i, _i] + _FIELD + _FIELD + [_vp]),
}


@functools.lru_cache(maxsize=None)
def lib():
    """The library handle of _lib.lib() with the affine entry points typed (raises if one is missing: there is no fallback)."""
    return _lib.bind(_lib.lib(), AFFINE_SIGNATURES)
