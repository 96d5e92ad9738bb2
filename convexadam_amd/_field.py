"""ctypes binding of the displacement-field operators (include/convexadam_field.h) onto the handle _lib.lib() returns.

A table of its own, as _prep.py has, typed by _lib.bind: _lib.SIGNATURES mirrors include/convexadam_hip.h name for name, FIELD_SIGNATURES mirrors
include/convexadam_field.h the same way (tests/test_fieldops_abi.py).  All headers describe the one libconvexadam_hip.so;
CVX_ABI_VERSION is unchanged."""
import ctypes as C
import functools

from . import _lib

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_FIELD = [_vp, _i, _i64, _i64]          # pointer, elements are double, component stride, voxel stride

# name -> (restype, argtypes)
FIELD_SIGNATURES = {
    "cvx_field_invert_f64": (_i, _FIELD + [_i, _i, _i, _i, _d] + _FIELD + [_vp, _vp, _vp, _vp]),
    "cvx_field_compose_f64": (_i, _FIELD + _FIELD + [_i, _i, _i] + _FIELD + [_vp]),
}


@functools.lru_cache(maxsize=None)
def lib():
    """The library handle of _lib.lib() with the field operators typed (raises if one is missing: there is no fallback)."""
    return _lib.bind(_lib.lib(), FIELD_SIGNATURES)
