"""CPU checks of the soft-statistics entry points (include/convexadam_soft.h): the header and the binding table list the same names, the
library exports them, none of them leaked into the other headers or tables, the ABI version is unchanged, the workspace query, and every
bad argument is refused with a message before anything touches a device (the pointers below are not memory: a launch would fault)."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "convexadam_soft.h")
NAMES = ["cvx_soft_stats_f32", "cvx_soft_stats_workspace_bytes"]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from abi_headers import header_functions, header_source  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _soft
    return _soft.lib()


def test_header_and_table_list_the_same_names(L):
    from convexadam_amd import _lib, _soft
    names = header_functions(HEADER)
    assert names == NAMES and names == sorted(_soft.SOFT_SIGNATURES) and _soft.SOFT_SIGNATURES is _lib.SOFT_SIGNATURES
    for table in (_lib.SIGNATURES, _lib.PREP_SIGNATURES, _lib.FIELD_SIGNATURES, _lib.AFFINE_SIGNATURES):
        assert not set(names) & set(table), "the soft-statistics entry points have a table of their own"
    src = header_source(HEADER)
    for other in ("convexadam_hip.h", "convexadam_prep.h", "convexadam_field.h", "convexadam_affine.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "cvx_soft" not in text, other
    for n in names:
        assert hasattr(L, n), "libconvexadam_hip.so does not export %s" % n
        assert getattr(L, n).restype is _soft.SOFT_SIGNATURES[n][0]
        assert getattr(L, n).argtypes == _soft.SOFT_SIGNATURES[n][1]
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1)
        assert len(args.split(",")) == len(_soft.SOFT_SIGNATURES[n][1]), n


def test_the_table_is_typed_on_the_shared_handle_and_a_missing_name_is_refused(L, monkeypatch):
    from convexadam_amd import _lib
    assert L is _lib.lib() and _lib.soft_lib() is L
    monkeypatch.setitem(_lib.SOFT_SIGNATURES, "cvx_soft_no_such_entry", (C.c_int, []))
    monkeypatch.setattr(_lib, "_soft_typed", None)
    with pytest.raises(RuntimeError, match="lacks the entry point cvx_soft_no_such_entry: rebuild with"):
        _lib.soft_lib()


def test_version_is_unchanged(L):
    from convexadam_amd import _lib
    assert L.cvx_version() == 2 == _lib.ABI_VERSION
    main = open(os.path.join(ROOT, "include", "convexadam_hip.h")).read()
    assert re.search(r"#define\s+CVX_ABI_VERSION\s+2\b", main)


def test_python_names_are_reexported():
    from convexadam_amd import confidence, convex_adam_utils
    for n in ("soft_stats", "soft_displacement", "soft_covariance", "soft_entropy", "soft_sigma", "convex_confidence", "Confidence"):
        assert getattr(convex_adam_utils, n) is getattr(confidence, n)


def test_there_is_no_cpu_path():
    import torch
    from convexadam_amd.confidence import soft_stats
    with pytest.raises(RuntimeError, match="no CPU path"):
        soft_stats(torch.zeros(27, 2, 2, 2), 1, 1.0)
    with pytest.raises(TypeError):
        soft_stats(torch.zeros(27, 2, 2, 2), 1)                  # beta has no default


def test_build_lists_the_source_and_the_header():
    from convexadam_amd.csrc import build
    assert "softstats.hip" in build.SOURCES
    for f in ("softstats.hip", "softstats_core.h"):
        assert os.path.exists(os.path.join(build.HERE, f)), f
    assert "convexadam_soft.h" in open(os.path.join(build.HERE, "build.py")).read()


def test_workspace_query(L):
    q = L.cvx_soft_stats_workspace_bytes
    for bad in ((0, 4, 4, 1), (4, -1, 4, 1), (4, 4, 0, 1), (4, 4, 4, -1), (4, 4, 4, 16), (64, 64, 64, 15), (1 << 16, 1 << 16, 1, 0)):
        assert q(*bad) == 0, bad
    # the minima of the n D-shift planes, one float per cell and plane, 256 bytes of slack behind them
    for h, w, d, hw in ((1, 1, 1, 0), (3, 5, 7, 2), (2, 3, 67, 1), (26, 32, 37, 6), (4, 9, 33, 5), (2, 2, 2, 15)):
        assert q(h, w, d, hw) == 4 * (2 * hw + 1) * h * w * d + 256, (h, w, d, hw)


SSD, FIELD, OUT, STATS, WS = (C.c_void_p(k << 32) for k in (1, 2, 3, 4, 5))


def test_refuses_bad_arguments_without_a_launch(L):
    h, w, d, hw = 3, 5, 7, 2
    V, K = h * w * d, 125
    ok = dict(ssd=SSD, half=0, field=FIELD, coupling=1.0, beta=2.0, h=h, w=w, d=d, hw=hw, out=OUT, stats=STATS, ws=WS,
              wsb=L.cvx_soft_stats_workspace_bytes(h, w, d, hw))

    def call(**kw):
        a = dict(ok, **kw)
        return L.cvx_soft_stats_f32(a["ssd"], a["half"], a["field"], a["coupling"], a["beta"], a["h"], a["w"], a["d"], a["hw"], a["out"], a["stats"],
                                    a["ws"], a["wsb"], None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in L.cvx_last_error(), (kw, L.cvx_last_error())

    for k in ("ssd", "out", "stats"):
        refused(b"null", **{k: None})
    for axis in "hwd":
        refused(b"extent", **{axis: 0})
        refused(b"extent", **{axis: -2})
    for bad in (-1, 16, 100):
        refused(b"hw", hw=bad)
    refused(b"2^31", h=64, w=64, d=64, hw=15)                      # 29791 x 262144
    refused(b"2^31", h=1 << 16, w=1 << 16, d=1, hw=0)
    refused(b"2^31", h=1 << 10, w=1 << 10, d=1 << 11, hw=0)        # K V = 2^31 exactly
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(b"beta", beta=bad)
    for bad in (-0.5, float("inf"), float("nan")):
        refused(b"coupling", coupling=bad)
    refused(b"needs a field", field=None)                          # coupling 1 without a field
    assert call(field=None, coupling=0.0, ssd=None) == -1 and b"null" in L.cvx_last_error()          # ... a zero coupling is fine without one
    refused(b"aligned", ssd=C.c_void_p((1 << 32) + 2))
    refused(b"aligned", ssd=C.c_void_p((1 << 32) + 1), half=1)
    refused(b"aligned", field=C.c_void_p((2 << 32) + 2))
    refused(b"aligned", out=C.c_void_p((3 << 32) + 1))
    refused(b"aligned", stats=C.c_void_p((4 << 32) + 4))
    refused(b"aligned", ws=C.c_void_p((5 << 32) + 4))
    refused(b"workspace", wsb=ok["wsb"] - 1)
    refused(b"workspace", wsb=0)
    refused(b"workspace", ws=None)
    refused(b"out overlaps an input", out=SSD)
    refused(b"out overlaps an input", out=C.c_void_p((1 << 32) + 4 * K * V - 4))
    refused(b"out overlaps an input", out=C.c_void_p((2 << 32) + 4 * 3 * V - 4))
    refused(b"out overlaps an input", out=C.c_void_p((1 << 32) + 2 * K * V + 2), half=0)
    refused(b"stats overlaps an input", stats=C.c_void_p((1 << 32) + 8))
    refused(b"the workspace overlaps an input", ws=C.c_void_p((2 << 32) + 8))
    refused(b"out overlaps stats", stats=C.c_void_p((3 << 32) + 48 * V - 8))
    refused(b"out overlaps the workspace", ws=C.c_void_p((3 << 32) + 8))
    refused(b"stats overlaps the workspace", stats=C.c_void_p((5 << 32) + 16))
    # a half volume ends after 2 K V bytes: an output right behind it is no overlap, and the call gets as far as the next check
    assert call(half=1, out=C.c_void_p((1 << 32) + 2 * K * V + 2), wsb=0) == -1 and b"workspace" in L.cvx_last_error()
