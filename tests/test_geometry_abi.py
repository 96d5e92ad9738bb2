"""CPU checks of the geometry entry points (csrc/geometry.hip): header and binding declare the same two symbols, the ABI version is
unchanged, and every refusal returns its status code and message before anything is launched.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cvx_resample_linear_f64", "cvx_field_to_grid_f64")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    return _lib.lib()


def doubles(v):
    return (C.c_double * len(v))(*v)


IDENT = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]


def test_header_and_binding_declare_the_symbols(L):
    from convexadam_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "convexadam_hip.h")).read(), flags=re.S)
    for name in NAMES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert decl, "%s is not declared in the header" % name
        assert name in _lib.SIGNATURES and hasattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(decl.group(1).split(","))
        assert args[-1] is C.c_void_p                                   # the stream
    assert re.search(r"#define\s+CVX_ABI_VERSION\s+2\b", src)
    assert L.cvx_version() == 2 == _lib.ABI_VERSION
    assert "geometry.hip" in __import__("convexadam_amd.csrc.build", fromlist=["SOURCES"]).SOURCES


def test_resample_refusals(L):
    a, b = C.c_void_p(1 << 20), C.c_void_p(2 << 20)

    def call(src=a, s64=0, sext=(4, 5, 6), out=b, o64=0, oext=(3, 4, 5), m=IDENT + [0.0, 0.0, 0.0], default=0.0):
        return L.cvx_resample_linear_f64(src, s64, *sext, out, o64, *oext, doubles(m) if m is not None else None, default, None)

    assert call(src=None) == -1 and b"null" in L.cvx_last_error()
    assert call(out=None) == -1 and b"null" in L.cvx_last_error()
    assert call(m=None) == -1 and b"null" in L.cvx_last_error()
    for which in ("sext", "oext"):
        for i in range(3):
            for bad in (0, -2):
                ext = [4, 5, 6]
                ext[i] = bad
                assert call(**{which: tuple(ext)}) == -1 and b"extent" in L.cvx_last_error(), (which, i, bad)
    big = (1 << 11, 1 << 10, 1 << 10)                                   # 2^31 voxels: one more than an int holds
    assert call(sext=big) == -1 and b"2^31" in L.cvx_last_error()
    assert call(oext=big) == -1 and b"2^31" in L.cvx_last_error()
    assert call(oext=(1 << 16, 1 << 16, 1)) == -1 and b"2^31" in L.cvx_last_error()
    assert call(out=a) == -1 and b"overlaps" in L.cvx_last_error()
    assert call(out=C.c_void_p((1 << 20) + 4 * 5 * 6 * 4 - 4)) == -1 and b"overlaps" in L.cvx_last_error()          # on src's last voxel
    assert call(src=C.c_void_p((2 << 20) + 3 * 4 * 5 * 8 - 8), o64=1) == -1 and b"overlaps" in L.cvx_last_error()   # on out's last voxel
    for k in range(12):
        for bad in (NAN, INF, -INF):
            m = IDENT + [0.0, 0.0, 0.0]
            m[k] = bad
            assert call(m=m) == -1 and b"non-finite" in L.cvx_last_error(), (k, bad)
    for bad in (NAN, INF, -INF):
        assert call(default=bad) == -1 and b"non-finite" in L.cvx_last_error()


def test_field_to_grid_refusals(L):
    f, mv, c, w = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)
    V = 4 * 5 * 6

    def call(field=f, f64=1, cs=1, vs=3, fext=(4, 5, 6), m=IDENT + [0.0, 0.0, 0.0], r=IDENT, ratio=(1.0, 1.0, 1.0), moving=mv, m64=0,
             mext=(3, 4, 5), carried=c, warped=w, w64=0):
        opt = lambda v: doubles(list(v)) if v is not None else None      # noqa: E731
        return L.cvx_field_to_grid_f64(field, f64, cs, vs, *fext, opt(m), opt(r), opt(ratio), moving, m64, *mext, carried, warped, w64, None)

    assert call(field=None) == -1 and b"null" in L.cvx_last_error()
    assert call(m=None) == -1 and b"null" in L.cvx_last_error()
    assert call(r=None) == -1 and b"null" in L.cvx_last_error()
    assert call(ratio=None) == -1 and b"null" in L.cvx_last_error()
    assert call(carried=None, warped=None) == -1 and b"no output" in L.cvx_last_error()
    assert call(moving=None) == -1 and b"needs the moving volume" in L.cvx_last_error()
    for which in ("fext", "mext"):
        for i in range(3):
            for bad in (0, -2):
                ext = [4, 5, 6]
                ext[i] = bad
                assert call(**{which: tuple(ext)}) == -1 and b"extent" in L.cvx_last_error(), (which, i, bad)
    big = (1 << 11, 1 << 10, 1 << 10)
    assert call(fext=big) == -1 and b"2^31" in L.cvx_last_error()
    assert call(mext=big) == -1 and b"2^31" in L.cvx_last_error()
    for cs, vs in ((0, 3), (1, 0), (-1, 3), (1, -3), (1, 2), (V - 1, 1), (2, 5), (1 << 41, 1), (1, 1 << 21)):
        assert call(cs=cs, vs=vs) == -1 and b"strides" in L.cvx_last_error(), (cs, vs)
    assert call(carried=f) == -1 and b"overlaps" in L.cvx_last_error()
    assert call(carried=mv) == -1 and b"overlaps" in L.cvx_last_error()
    assert call(warped=f) == -1 and b"overlaps" in L.cvx_last_error()
    assert call(warped=mv) == -1 and b"overlaps" in L.cvx_last_error()
    assert call(warped=C.c_void_p((1 << 20) + 3 * V * 8 - 8)) == -1 and b"overlaps" in L.cvx_last_error()            # on the field's last element
    assert call(f64=0, cs=V, vs=1, warped=C.c_void_p((1 << 20) + 3 * V * 4 - 4)) == -1 and b"overlaps" in L.cvx_last_error()
    assert call(warped=c) == -1 and b"outputs overlap" in L.cvx_last_error()
    assert call(warped=C.c_void_p((3 << 20) + 3 * 4 * 5 * 3 * 8 - 8)) == -1 and b"outputs overlap" in L.cvx_last_error()
    for name, n in (("m", 12), ("r", 9), ("ratio", 3)):
        for k in range(n):
            for bad in (NAN, INF, -INF):
                v = {"m": IDENT + [0.0, 0.0, 0.0], "r": list(IDENT), "ratio": [1.0, 1.0, 1.0]}[name]
                v[k] = bad
                assert call(**{name: v}) == -1 and b"non-finite" in L.cvx_last_error(), (name, k, bad)


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    from convexadam_amd import geometry
    from convexadam_amd.convex_adam_utils import register_images, resample_device, rescale_displacement_field_device  # noqa: F401  (re-exported)
    import convexAdam.convex_adam_utils as shim
    for name in ("grid_of", "index_map", "resample_device", "rescale_displacement_field_device", "register_images"):
        assert getattr(shim, name) is getattr(geometry, name)
    g = geometry.Grid((6, 5, 4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(IDENT))
    with pytest.raises(RuntimeError, match="no CPU"):
        geometry.resample_device(torch.zeros(4, 5, 6), g, g)
    with pytest.raises(RuntimeError, match="no CPU"):
        geometry.rescale_displacement_field_device(torch.zeros(4, 5, 6, 3), g, g, g)
