"""CPU checks of the field-operator entry points (include/convexadam_field.h): the header and the binding table list the same names, the
library exports them, none of them leaked into the main header or table, the ABI version is unchanged, and every bad argument is refused
with a message before anything touches a device (the pointers below are not memory: a launch would fault)."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "convexadam_field.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from abi_headers import header_functions  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _field
    return _field.lib()


def test_header_and_table_list_the_same_names(L):
    from convexadam_amd import _field, _lib
    names = header_functions(HEADER)
    assert names == ["cvx_field_compose_f64", "cvx_field_invert_f64"] and names == sorted(_field.FIELD_SIGNATURES)
    assert not set(names) & set(_lib.SIGNATURES), "the field operators have a table of their own"
    main = open(os.path.join(ROOT, "include", "convexadam_hip.h")).read()
    for n in names:
        assert hasattr(L, n), "libconvexadam_hip.so does not export %s" % n
        assert n not in main
        assert getattr(L, n).restype is _field.FIELD_SIGNATURES[n][0]
    # the argument counts of the declarations and of the table agree
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1)
        assert len(args.split(",")) == len(_field.FIELD_SIGNATURES[n][1]), n


def test_version_is_unchanged(L):
    from convexadam_amd import _lib
    assert L.cvx_version() == 2 == _lib.ABI_VERSION


def test_python_names_are_reexported():
    from convexadam_amd import convex_adam_utils, fieldops
    for n in ("invert_field", "compose_fields", "apply_convex_inverse"):
        assert getattr(convex_adam_utils, n) is getattr(fieldops, n)


U, VO, RES, IT, ST = (C.c_void_p(k << 24) for k in (1, 2, 3, 4, 5))
H, W, D = 6, 5, 7
V = H * W * D


def test_invert_refuses_bad_arguments_without_a_launch(L):
    ok = dict(u=U, u64=0, ucs=1, uvs=3, H=H, W=W, D=D, it=50, tol=1e-4, v=VO, v64=1, vcs=V, vvs=1, res=RES, iters=IT, stats=ST)

    def call(**kw):
        a = dict(ok, **kw)
        return L.cvx_field_invert_f64(a["u"], a["u64"], a["ucs"], a["uvs"], a["H"], a["W"], a["D"], a["it"], a["tol"], a["v"], a["v64"], a["vcs"],
                                      a["vvs"], a["res"], a["iters"], a["stats"], None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in L.cvx_last_error(), (kw, L.cvx_last_error())

    refused(b"null", u=None)
    refused(b"null", v=None)
    for axis in "HWD":
        refused(b"extent", **{axis: 0})
        refused(b"extent", **{axis: -3})
    refused(b"2^31", H=2048, W=2048, D=512)
    refused(b"2^31", H=1 << 16, W=1 << 16, D=1)
    refused(b"strides of u", ucs=1, uvs=2)                       # components fold onto the next voxel
    refused(b"strides of u", ucs=V - 1, uvs=1)                   # planes fold onto each other
    refused(b"strides of u", ucs=0)
    refused(b"strides of u", uvs=-3)
    refused(b"strides of v_out", vcs=1, vvs=1)
    refused(b"strides of v_out", vcs=V // 2, vvs=1)
    for it in (0, -1, 1001):
        refused(b"max_iters", it=it)
    for tol in (-1e-9, float("nan"), float("inf")):
        refused(b"tol", tol=tol)
    refused(b"aligned", u=C.c_void_p((1 << 24) + 2))
    refused(b"aligned", v=C.c_void_p((2 << 24) + 4))
    refused(b"aligned", res=C.c_void_p((3 << 24) + 4))
    refused(b"overlaps u", v=C.c_void_p((1 << 24) + 8))
    refused(b"overlaps u", v=U)
    refused(b"overlaps u", res=C.c_void_p((1 << 24) + 4 * 3 * V - 8))
    refused(b"overlaps u", iters=C.c_void_p((1 << 24) + 17))
    refused(b"overlaps u", stats=U)
    refused(b"outputs overlap", res=C.c_void_p((2 << 24) + 8 * 3 * V - 8))
    refused(b"outputs overlap", iters=C.c_void_p((3 << 24) + 8 * V - 1))
    refused(b"outputs overlap", stats=C.c_void_p((4 << 24) + V - 1 - (V - 1) % 8))
    refused(b"outputs overlap", stats=VO)


def test_compose_refuses_bad_arguments_without_a_launch(L):
    A, B, O = U, VO, RES
    ok = dict(a=A, a64=1, acs=1, avs=3, b=B, b64=0, bcs=V, bvs=1, H=H, W=W, D=D, out=O, o64=0, ocs=1, ovs=3)

    def call(**kw):
        a = dict(ok, **kw)
        return L.cvx_field_compose_f64(a["a"], a["a64"], a["acs"], a["avs"], a["b"], a["b64"], a["bcs"], a["bvs"], a["H"], a["W"], a["D"], a["out"],
                                       a["o64"], a["ocs"], a["ovs"], None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in L.cvx_last_error(), (kw, L.cvx_last_error())

    for k in ("a", "b", "out"):
        refused(b"null", **{k: None})
    for axis in "HWD":
        refused(b"extent", **{axis: 0})
    refused(b"2^31", H=2048, W=2048, D=512)
    refused(b"strides of a", acs=2, avs=3)
    refused(b"strides of b", bcs=V - 1)
    refused(b"strides of out", ocs=1, ovs=1)
    refused(b"aligned", a=C.c_void_p((1 << 24) + 4))
    refused(b"aligned", out=C.c_void_p((3 << 24) + 1))
    refused(b"overlaps", out=A)
    refused(b"overlaps", out=C.c_void_p((2 << 24) + 4 * 3 * V - 4))
