"""ctypes binding of the preprocessing entry points (include/convexadam_prep.h) onto the handle _lib.lib() returns.

A table of its own, typed by _lib.bind: _lib.SIGNATURES mirrors include/convexadam_hip.h name for name, PREP_SIGNATURES mirrors
include/convexadam_prep.h the same way (tests/test_prep_abi.py).  Both headers describe the one libconvexadam_hip.so; CVX_ABI_VERSION is
unchanged."""
import ctypes as C
import functools

from . import _lib

CVX_PREP_CLAMP, CVX_PREP_POSITIVE = 1, 2

_vp, _i, _f, _sz, _ll = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_longlong

# name -> (restype, argtypes)
PREP_SIGNATURES = {
    "cvx_prep_stats_workspace_bytes": (_sz, [_ll]),
    "cvx_prep_stats_f32": (_i, [_vp, _ll, _i, _f, _f, _i, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    "cvx_prep_normalise_f32": (_i, [_vp, _ll, _vp, C.POINTER(C.c_float), _i, _vp, _vp]),
    "cvx_prep_nonzero_mask_workspace_bytes": (_sz, [_i, _i, _i]),
    "cvx_prep_nonzero_mask_u8": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, C.POINTER(C.c_int), _vp, _sz, _vp]),
    "cvx_prep_mask_bbox_i32": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
}


@functools.lru_cache(maxsize=None)
def lib():
    """The library handle of _lib.lib() with the preprocessing entry points typed (raises if one is missing: there is no fallback)."""
    return _lib.bind(_lib.lib(), PREP_SIGNATURES)
