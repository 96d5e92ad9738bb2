"""CPU checks of the preprocessing entry points (include/convexadam_prep.h): the header and the binding table list the same names, the
library exports them, the ABI version is unchanged, and bad arguments are refused before anything touches a device."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "convexadam_prep.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from abi_headers import header_functions  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _prep
    return _prep.lib()


def test_header_and_table_list_the_same_names(L):
    from convexadam_amd import _lib, _prep
    names = header_functions(HEADER)
    assert len(names) == 6 and names == sorted(_prep.PREP_SIGNATURES)
    assert not set(names) & set(_lib.SIGNATURES), "the preprocessing entry points have a table of their own"
    main = open(os.path.join(ROOT, "include", "convexadam_hip.h")).read()
    for n in names:
        assert hasattr(L, n), "libconvexadam_hip.so does not export %s" % n
        assert n not in main
        assert getattr(L, n).restype is _prep.PREP_SIGNATURES[n][0]


def test_version_is_unchanged(L):
    from convexadam_amd import _lib
    assert L.cvx_version() == 2 == _lib.ABI_VERSION


def test_stats_refuses_bad_arguments_without_a_launch(L):
    d, big = C.c_void_p(1 << 20), 1 << 30
    ok = dict(x=d, n=1000, flags=1, lo=-1000.0, hi=1500.0, nq=2, q0=0.005, q1=0.995, params=C.c_void_p(2 << 20), mom=None, ws=C.c_void_p(3 << 20), nws=big)

    def call(**kw):
        a = dict(ok, **kw)
        return L.cvx_prep_stats_f32(a["x"], a["n"], a["flags"], a["lo"], a["hi"], a["nq"], a["q0"], a["q1"], a["params"], a["mom"], a["ws"], a["nws"], None)

    assert call(x=None) == -1 and b"null" in L.cvx_last_error()
    assert call(params=None) == -1 and b"null" in L.cvx_last_error()
    assert call(n=0) == -1 and b"extent" in L.cvx_last_error()
    assert call(n=1 << 31) == -1
    assert call(flags=4) == -1 and b"flag" in L.cvx_last_error()
    assert call(nq=1) == -1 and call(q0=-0.5) == -1 and call(q1=float("nan")) == -1
    assert call(flags=3) == -1 and b"positive" in L.cvx_last_error()
    assert call(lo=5.0, hi=1.0) == -1 and b"clamp" in L.cvx_last_error()
    assert call(params=d) == -1 and b"overlaps" in L.cvx_last_error()
    need = L.cvx_prep_stats_workspace_bytes(1000)
    assert need > 4 * (2048 + 4 * 2048 + 4 * 1024)                       # the three histogram sets
    assert call(nws=need - 1) == -2 and b"workspace" in L.cvx_last_error()
    assert call(ws=None) == -2
    assert L.cvx_prep_stats_workspace_bytes(0) == 0 and L.cvx_prep_stats_workspace_bytes(1 << 31) == 0
    # three arrays of 8 bytes per span of 4096 elements (sums, centred squares, counts), each carved at a multiple of 256 bytes:
    # 4096 spans take 3 * 32768 bytes, one span 256 + 256 + 8
    assert L.cvx_prep_stats_workspace_bytes(1 << 24) - need == 3 * 8 * 4096 - (256 + 256 + 8)


def test_normalise_refuses_bad_arguments_without_a_launch(L):
    d, o, p = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)
    hp = (C.c_float * 4)(0, 1, 0, 1)
    assert L.cvx_prep_normalise_f32(None, 10, p, None, 0, o, None) == -1 and b"null" in L.cvx_last_error()
    assert L.cvx_prep_normalise_f32(d, 10, p, None, 0, None, None) == -1
    assert L.cvx_prep_normalise_f32(d, 10, None, None, 0, o, None) == -1 and b"exactly one" in L.cvx_last_error()
    assert L.cvx_prep_normalise_f32(d, 10, p, hp, 0, o, None) == -1 and b"exactly one" in L.cvx_last_error()
    assert L.cvx_prep_normalise_f32(d, 0, p, None, 0, o, None) == -1 and b"extent" in L.cvx_last_error()
    assert L.cvx_prep_normalise_f32(d, 10, p, None, 2, o, None) == -1 and b"mode" in L.cvx_last_error()
    assert L.cvx_prep_normalise_f32(d, 10, p, None, 0, C.c_void_p((1 << 20) + 8), None) == -1 and b"overlaps" in L.cvx_last_error()
    assert L.cvx_prep_normalise_f32(d, 10, o, None, 0, o, None) == -1 and b"params" in L.cvx_last_error()


def test_mask_entry_points_refuse_bad_arguments_without_a_launch(L):
    d, m, b, w = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)
    big = 1 << 30
    assert L.cvx_prep_nonzero_mask_u8(None, 1, 4, 4, 4, 3, m, b, None, None, w, big, None) == -1 and b"null" in L.cvx_last_error()
    assert L.cvx_prep_nonzero_mask_u8(d, 1, 4, 4, 4, 3, m, None, None, None, w, big, None) == -1
    assert L.cvx_prep_nonzero_mask_u8(d, 0, 4, 4, 4, 3, m, b, None, None, w, big, None) == -1 and b"channels" in L.cvx_last_error()
    assert L.cvx_prep_nonzero_mask_u8(d, 1, 4, 0, 4, 3, m, b, None, None, w, big, None) == -1 and b"extent" in L.cvx_last_error()
    assert L.cvx_prep_nonzero_mask_u8(d, 1, 2048, 2048, 2048, 3, m, b, None, None, w, big, None) == -1 and b"2^31" in L.cvx_last_error()
    assert L.cvx_prep_nonzero_mask_u8(d, 1, 4, 4, 4, 2, m, b, None, None, w, big, None) == -1 and b"ndim" in L.cvx_last_error()
    assert L.cvx_prep_nonzero_mask_u8(d, 1, 4, 4, 4, 3, d, b, None, None, w, big, None) == -1 and b"overlaps" in L.cvx_last_error()
    need = L.cvx_prep_nonzero_mask_workspace_bytes(4, 4, 4)
    assert need >= 64 + 4
    assert L.cvx_prep_nonzero_mask_u8(d, 1, 4, 4, 4, 3, m, b, None, None, w, need - 1, None) == -2 and b"workspace" in L.cvx_last_error()
    assert L.cvx_prep_nonzero_mask_u8(d, 1, 4, 4, 4, 3, m, b, None, None, None, 0, None) == -2
    assert L.cvx_prep_nonzero_mask_workspace_bytes(4, 0, 4) == 0
    assert L.cvx_prep_mask_bbox_i32(None, 4, 4, 4, b, None, None) == -1 and b"null" in L.cvx_last_error()
    assert L.cvx_prep_mask_bbox_i32(m, 4, 4, 4, None, None, None) == -1
    assert L.cvx_prep_mask_bbox_i32(m, 4, 4, 0, b, None, None) == -1 and b"extent" in L.cvx_last_error()
    assert L.cvx_prep_mask_bbox_i32(m, 4, 4, 4, m, None, None) == -1 and b"overlaps" in L.cvx_last_error()
