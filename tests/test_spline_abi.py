"""CPU checks of the spline entry points (include/convexadam_spline.h): the header and the binding table list the same names, the library
exports them, none of them leaked into the other six headers or tables, the table is typed lazily, the ABI version is unchanged, the
Python names are re-exported, there is no CPU path, and every bad argument is refused with a message before anything touches a device
(the pointers below are not memory: a launch would fault)."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "convexadam_spline.h")
NAMES = ["cvx_map_coordinates_cubic_f64", "cvx_resample_cubic_f64", "cvx_spline_prefilter_f64"]
OTHER_HEADERS = ("convexadam_hip.h", "convexadam_prep.h", "convexadam_field.h", "convexadam_affine.h", "convexadam_soft.h", "convexadam_sim.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from abi_headers import header_functions, header_source  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _spline
    return _spline.lib()


def test_header_and_table_list_the_same_names(L):
    from convexadam_amd import _lib, _spline
    names = header_functions(HEADER)
    assert names == NAMES and names == sorted(_spline.SPLINE_SIGNATURES) and _spline.SPLINE_SIGNATURES is _lib.SPLINE_SIGNATURES
    for table in (_lib.SIGNATURES, _lib.PREP_SIGNATURES, _lib.FIELD_SIGNATURES, _lib.AFFINE_SIGNATURES, _lib.SOFT_SIGNATURES, _lib.SIM_SIGNATURES):
        assert not set(names) & set(table), "the spline entry points have a table of their own"
    src = header_source(HEADER)
    for other in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "cvx_spline" not in text and "_cubic_f64" not in text, other
        # ... and the new header names no entry point of the others, in its comments either
        for n in header_functions(os.path.join(ROOT, "include", other)):
            assert not re.search(r"\b%s\b" % n, open(HEADER).read()), (other, n)
    for n in names:
        assert hasattr(L, n), "libconvexadam_hip.so does not export %s" % n
        assert getattr(L, n).restype is _spline.SPLINE_SIGNATURES[n][0]
        assert getattr(L, n).argtypes == _spline.SPLINE_SIGNATURES[n][1]
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1)
        assert len(args.split(",")) == len(_spline.SPLINE_SIGNATURES[n][1]), n
        assert args.split(",")[-1].strip() == "void* stream", n


def test_the_table_is_typed_lazily_on_the_shared_handle_and_a_missing_name_is_refused(L, monkeypatch):
    import inspect
    from convexadam_amd import _lib
    assert L is _lib.lib() and _lib.spline_lib() is L
    assert "SPLINE_SIGNATURES" not in inspect.getsource(_lib._typed), "lib() types four tables; the spline table is typed by spline_lib()"
    monkeypatch.setitem(_lib.SPLINE_SIGNATURES, "cvx_spline_no_such_entry", (C.c_int, []))
    monkeypatch.setattr(_lib, "_spline_typed", None)
    with pytest.raises(RuntimeError, match="lacks the entry point cvx_spline_no_such_entry: rebuild with"):
        _lib.spline_lib()


def test_version_is_unchanged(L):
    from convexadam_amd import _lib
    assert L.cvx_version() == 2 == _lib.ABI_VERSION
    main = open(os.path.join(ROOT, "include", "convexadam_hip.h")).read()
    assert re.search(r"#define\s+CVX_ABI_VERSION\s+2\b", main)


def test_python_names_are_reexported():
    import inspect
    from convexadam_amd import apply_convex, convex_adam_utils, geometry, spline
    import convexAdam.apply_convex as shim
    for n in ("spline_coefficients", "warp_cubic"):
        assert getattr(convex_adam_utils, n) is getattr(spline, n)
    assert inspect.signature(apply_convex.apply_convex).parameters["order"].default == 1
    assert list(inspect.signature(apply_convex.apply_convex).parameters) == ["disp", "moving", "device", "order"]
    assert inspect.signature(geometry.resample_device).parameters["order"].default == 1
    assert list(inspect.signature(geometry.resample_device).parameters) == ["src", "src_grid", "out_grid", "default", "order"]
    assert list(inspect.signature(spline.warp_cubic).parameters) == ["moving", "disp", "prefiltered"]
    assert shim.apply_convex is apply_convex.apply_convex
    for word in ("orders 2, 4 and 5", "boundary modes", "cvx_field_to_grid_f64", "histogram", "registration itself", "gradients"):
        assert word in spline.__doc__, "the module says what is not built: %s" % word


def test_other_orders_are_refused_before_anything_else():
    import numpy as np
    from convexadam_amd.apply_convex import apply_convex, main
    from convexadam_amd.geometry import resample_device
    for order in (0, 2, 4, 5, "3", None):
        with pytest.raises(ValueError, match="order must be 1"):
            apply_convex(np.zeros((2, 3, 4, 3)), np.zeros((2, 3, 4)), order=order)
        with pytest.raises(ValueError, match="order must be 1"):
            resample_device(None, None, None, order=order)
    with pytest.raises(SystemExit):
        main(["--input_field", "a", "--input_moving", "b", "--output_warped", "c", "--order", "2"])


def test_there_is_no_cpu_path():
    import torch
    from convexadam_amd.geometry import Grid, resample_device
    from convexadam_amd.spline import spline_coefficients, warp_cubic
    z = torch.zeros(2, 3, 4)
    g = Grid((4, 3, 2), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0))
    for f in (lambda: spline_coefficients(z), lambda: warp_cubic(z, torch.zeros(2, 3, 4, 3)), lambda: warp_cubic(z.double(), torch.zeros(3, 2, 3, 4), True),
              lambda: resample_device(z, g, g, order=3)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()


def test_build_lists_the_source_and_the_header():
    from convexadam_amd.csrc import build
    assert "spline.hip" in build.SOURCES and "-ffp-contract=off" in build.FLAGS and "spline.hip" not in build.PER_FILE_FLAGS
    for f in ("spline.hip", "spline_core.h"):
        assert os.path.exists(os.path.join(build.HERE, f)), f
    assert "convexadam_spline.h" in open(os.path.join(build.HERE, "build.py")).read()
    core = open(os.path.join(build.HERE, "spline_core.h")).read()
    assert "__global__" not in core and "hip_runtime" not in core, "spline_core.h is plain C++ apart from the function qualifiers"
    assert "pow(" not in core.replace("spline_pole_power(", ""), "z^(n-1) is a sequential product"


SRC, COEF, FIELD, OUT, MAP = (k << 32 for k in (1, 2, 3, 4, 5))


def at(base, off=0):
    return C.c_void_p(base + off)


def test_refuses_bad_arguments_without_a_launch(L):
    H, W, D = 3, 5, 7
    V = H * W * D
    map12 = (C.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    ok = dict(src=at(SRC), sf64=0, coef=at(COEF), field=at(FIELD), f64=0, cs=V, vs=1, H=H, W=W, D=D, out=at(OUT), of64=1, oz=2, oy=3, ox=4, map=map12,
              dflt=0.0)

    def prefilter(**kw):
        a = dict(ok, **kw)
        return L.cvx_spline_prefilter_f64(a["src"], a["sf64"], a["H"], a["W"], a["D"], a["coef"], None)

    def warp(**kw):
        a = dict(ok, **kw)
        return L.cvx_map_coordinates_cubic_f64(a["coef"], a["field"], a["f64"], a["cs"], a["vs"], a["H"], a["W"], a["D"], a["out"], None)

    def resample(**kw):
        a = dict(ok, **kw)
        return L.cvx_resample_cubic_f64(a["coef"], a["H"], a["W"], a["D"], a["out"], a["of64"], a["oz"], a["oy"], a["ox"], a["map"], a["dflt"], None)

    calls = {"cvx_spline_prefilter_f64": prefilter, "cvx_map_coordinates_cubic_f64": warp, "cvx_resample_cubic_f64": resample}

    def refused(word, which, **kw):
        for name in which:
            assert calls[name](**kw) == -1, (name, kw)
            msg = L.cvx_last_error()
            assert word in msg and name.encode() in msg, (name, kw, msg)

    every = list(calls)
    refused(b"null", every, coef=None)
    refused(b"null", every[:1], src=None)
    refused(b"null", every[1:2], field=None)
    refused(b"null", every[1:], out=None)
    refused(b"null", every[2:], map=None)
    for axis in "HWD":
        refused(b"extent", every, **{axis: 0})
        refused(b"extent", every, **{axis: -2})
    for axis in ("oz", "oy", "ox"):
        refused(b"extent", every[2:], **{axis: 0})
    refused(b"2^31", every, H=1 << 11, W=1 << 10, D=1 << 10, cs=1 << 31)           # H W D = 2^31 exactly
    refused(b"2^31", every, H=1 << 16, W=1 << 16, D=1, cs=1 << 32)
    refused(b"2^31", every[2:], oz=1 << 11, oy=1 << 10, ox=1 << 10)
    # field strides, the rule of the field-carrying entry point of the main header: positive, and components not folded onto each other
    for cs, vs in ((0, 1), (V, 0), (-1, 3), (1, 2), (V - 1, 1), (2, 5), (1 << 40, 1), (1, 1 << 20)):
        refused(b"strides", every[1:2], cs=cs, vs=vs)
    refused(b"aligned", every[:1], src=at(SRC, 2))
    refused(b"aligned", every[:1], src=at(SRC, 4), sf64=1)
    refused(b"aligned", every, coef=at(COEF, 4))
    refused(b"aligned", every[1:2], field=at(FIELD, 2))
    refused(b"aligned", every[1:2], field=at(FIELD, 4), f64=1)
    refused(b"aligned", every[1:], out=at(OUT, 4))
    refused(b"aligned", every[2:], out=at(OUT, 2), of64=0)
    # an output overlapping an input; the one permitted overlap is src == coef with double samples
    refused(b"coef overlaps src", every[:1], coef=at(SRC, 8))
    refused(b"coef overlaps src", every[:1], coef=at(SRC, 4 * V - 4 - (4 * V - 4) % 8))
    refused(b"coef overlaps src", every[:1], coef=at(SRC, 8 * V - 8), sf64=1)
    refused(b"coef overlaps src", every[:1], coef=at(SRC, -8 * V + 8))
    refused(b"coef overlaps src", every[:1], coef=at(SRC))                           # the same address with float samples: 4-byte reads under 8-byte writes
    refused(b"out overlaps an input", every[1:], out=at(COEF, 8 * V - 8))
    refused(b"out overlaps an input", every[1:2], out=at(COEF, -8 * V + 8))
    refused(b"out overlaps an input", every[2:], out=at(COEF, -8 * 24 + 8))
    refused(b"out overlaps an input", every[1:2], out=at(FIELD, 4 * 3 * V - 4 - (4 * 3 * V - 4) % 8))
    refused(b"out overlaps an input", every[1:2], out=at(FIELD, 8 * 3 * V - 8), f64=1)
    refused(b"out overlaps an input", every[1:2], out=at(FIELD, 8 * 3 * V - 8), f64=1, cs=1, vs=3)
    for k in (0, 5, 11):
        for bad in (float("nan"), float("inf"), -float("inf")):
            m = (C.c_double * 12)(*[bad if i == k else float(i % 4 == 0) for i in range(12)])
            refused(b"non-finite", every[2:], map=m)
    for bad in (float("nan"), float("inf")):
        refused(b"non-finite", every[2:], dflt=bad)
