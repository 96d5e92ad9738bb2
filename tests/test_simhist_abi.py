"""CPU checks of the similarity entry points (include/convexadam_sim.h): the header and the binding table list the same names, the library
exports them, none of them leaked into the other five headers or tables, the ABI version is unchanged, the path query, and every bad
argument is refused with a message before anything touches a device (the pointers below are not memory: a launch would fault)."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "convexadam_sim.h")
NAMES = ["cvx_joint_hist_f32", "cvx_joint_hist_lds_bytes", "cvx_sim_range_f32"]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from abi_headers import header_functions, header_source  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _sim
    return _sim.lib()


def test_header_and_table_list_the_same_names(L):
    from convexadam_amd import _lib, _sim
    names = header_functions(HEADER)
    assert names == NAMES and names == sorted(_sim.SIM_SIGNATURES) and _sim.SIM_SIGNATURES is _lib.SIM_SIGNATURES
    for table in (_lib.SIGNATURES, _lib.PREP_SIGNATURES, _lib.FIELD_SIGNATURES, _lib.AFFINE_SIGNATURES, _lib.SOFT_SIGNATURES):
        assert not set(names) & set(table), "the similarity entry points have a table of their own"
    src = header_source(HEADER)
    for other in ("convexadam_hip.h", "convexadam_prep.h", "convexadam_field.h", "convexadam_affine.h", "convexadam_soft.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "cvx_sim" not in text and "cvx_joint_hist" not in text, other
    for n in names:
        assert hasattr(L, n), "libconvexadam_hip.so does not export %s" % n
        assert getattr(L, n).restype is _sim.SIM_SIGNATURES[n][0]
        assert getattr(L, n).argtypes == _sim.SIM_SIGNATURES[n][1]
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1)
        assert len(args.split(",")) == len(_sim.SIM_SIGNATURES[n][1]), n


def test_the_table_is_typed_on_the_shared_handle_and_a_missing_name_is_refused(L, monkeypatch):
    from convexadam_amd import _lib
    assert L is _lib.lib() and _lib.sim_lib() is L
    monkeypatch.setitem(_lib.SIM_SIGNATURES, "cvx_sim_no_such_entry", (C.c_int, []))
    monkeypatch.setattr(_lib, "_sim_typed", None)
    with pytest.raises(RuntimeError, match="lacks the entry point cvx_sim_no_such_entry: rebuild with"):
        _lib.sim_lib()


def test_version_is_unchanged(L):
    from convexadam_amd import _lib
    assert L.cvx_version() == 2 == _lib.ABI_VERSION
    main = open(os.path.join(ROOT, "include", "convexadam_hip.h")).read()
    assert re.search(r"#define\s+CVX_ABI_VERSION\s+2\b", main)


def test_python_names_are_reexported():
    from convexadam_amd import convex_adam_utils, similarity
    for n in ("joint_histogram", "value_range", "entropies", "mutual_information", "normalized_mutual_information", "registration_mi",
              "RegistrationMI"):
        assert getattr(convex_adam_utils, n) is getattr(similarity, n)
    assert similarity.RegistrationMI._fields == ("mi_before", "mi_after", "nmi_before", "nmi_after")


def test_there_is_no_cpu_path():
    import torch
    from convexadam_amd.similarity import joint_histogram, registration_mi, value_range
    z = torch.zeros(2, 3, 4)
    for f in (lambda: joint_histogram(z, z), lambda: value_range(z, z), lambda: registration_mi(z, z, torch.zeros(3, 2, 3, 4))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()


def test_build_lists_the_source_and_the_header():
    from convexadam_amd.csrc import build
    assert "simhist.hip" in build.SOURCES
    for f in ("simhist.hip", "simhist_core.h"):
        assert os.path.exists(os.path.join(build.HERE, f)), f
    assert "convexadam_sim.h" in open(os.path.join(build.HERE, "build.py")).read()


def test_the_path_query(L):
    q = L.cvx_joint_hist_lds_bytes
    for bad in ((1, 32), (32, 1), (0, 0), (257, 2), (2, 257), (-4, 8)):
        assert q(*bad) == -1, bad
    # copies = as many as fit 32 KiB, at most 4 (one per wavefront), at least 1; nothing above 64 KiB
    assert q(2, 2) == 4 * 16 and q(32, 32) == 4 * 4096 and q(64, 64) == 2 * 16384 and q(7, 130) == 4 * 3640
    assert q(128, 128) == 65536 and q(256, 64) == 65536 and q(91, 90) == 32760
    assert q(129, 128) == 0 and q(128, 129) == 0 and q(256, 256) == 0
    for ba in range(2, 257, 9):
        for bb in range(2, 257, 7):
            v = q(ba, bb)
            assert (v == 0) == (ba * bb * 4 > 65536) and v <= 65536 and v % (ba * bb * 4) == 0


FIXED, MOVING, FIELD, MASK, RANGE, HIST, STATS = (C.c_void_p(k << 32) for k in (1, 2, 3, 4, 5, 6, 7))


def at(base, off):
    return C.c_void_p((base << 32) + off)


def test_refuses_bad_arguments_without_a_launch(L):
    H, W, D = 3, 5, 7
    V = H * W * D
    ok = dict(fixed=FIXED, moving=MOVING, field=FIELD, f64=0, cs=V, vs=1, mask=MASK, H=H, W=W, D=D, ba=32, bb=16, range=RANGE, drop=0, hist=HIST,
              stats=STATS)

    def hist(**kw):
        a = dict(ok, **kw)
        return L.cvx_joint_hist_f32(a["fixed"], a["moving"], a["field"], a["f64"], a["cs"], a["vs"], a["mask"], a["H"], a["W"], a["D"], a["ba"], a["bb"],
                                    a["range"], a["drop"], a["hist"], a["stats"], None)

    def rng(**kw):
        a = dict(ok, **kw)
        return L.cvx_sim_range_f32(a["fixed"], a["moving"], a["field"], a["f64"], a["cs"], a["vs"], a["mask"], a["H"], a["W"], a["D"], a["drop"],
                                   a["range"], a["stats"], None)

    def refused(word, both=True, **kw):
        for name, f in (("cvx_joint_hist_f32", hist), ("cvx_sim_range_f32", rng))[:2 if both else 1]:
            assert f(**kw) == -1, (name, kw)
            msg = L.cvx_last_error()
            assert word in msg and name.encode() in msg, (name, kw, msg)

    for k in ("fixed", "moving", "range", "stats"):
        refused(b"null", **{k: None})
    refused(b"null", both=False, hist=None)
    for axis in "HWD":
        refused(b"extent", **{axis: 0})
        refused(b"extent", **{axis: -2})
    refused(b"2^31", H=1 << 11, W=1 << 10, D=1 << 10, field=None)          # H W D = 2^31 exactly
    refused(b"2^31", H=1 << 16, W=1 << 16, D=1, field=None)
    for bad in (1, 0, -3, 257, 1 << 20):
        refused(b"bins", both=False, ba=bad)
        refused(b"bins", both=False, bb=bad)
    # field strides, the rule of cvx_field_to_grid_f64: positive, and components not folded onto each other
    for cs, vs in ((0, 1), (V, 0), (-1, 3), (1, 2), (V - 1, 1), (2, 5), (1 << 40, 1), (1, 1 << 20)):
        refused(b"strides", cs=cs, vs=vs)
    assert hist(field=None, cs=0, vs=0, ba=1) == -1 and b"bins" in L.cvx_last_error()               # ... without a field they are not looked at: the next check answers
    refused(b"aligned", fixed=at(1, 2))
    refused(b"aligned", moving=at(2, 1))
    refused(b"aligned", field=at(3, 2))
    refused(b"aligned", field=at(3, 4), f64=1)
    refused(b"aligned", range=at(5, 2))
    refused(b"aligned", stats=at(7, 4))
    refused(b"aligned", both=False, hist=at(6, 4))
    # an output overlapping any other buffer
    for k, nbytes in (("fixed", 4 * V), ("moving", 4 * V), ("field", 4 * 3 * V), ("mask", V)):
        base = ok[k].value
        refused(b"stats overlaps an input", stats=C.c_void_p(base + (nbytes - 1) // 8 * 8))
        refused(b"hist overlaps an input", both=False, hist=C.c_void_p(base))
    assert rng(range=at(1, 4 * V - 4)) == -1 and b"range_out overlaps an input" in L.cvx_last_error()
    assert rng(range=at(4, V - 1 - (V - 1) % 4)) == -1 and b"range_out overlaps an input" in L.cvx_last_error()
    assert rng(range=at(7, 32)) == -1 and b"range_out overlaps stats" in L.cvx_last_error()
    assert rng(stats=at(5, 8)) == -1 and b"range_out overlaps stats" in L.cvx_last_error()
    refused(b"hist overlaps an input", both=False, hist=at(5, 8))                                    # the range is an input of the histogram
    refused(b"stats overlaps an input", both=False, stats=at(5, 8))
    refused(b"hist overlaps stats", both=False, stats=at(6, 8 * 32 * 16 - 8))
    refused(b"hist overlaps an input", both=False, hist=at(1, -8 * 32 * 16 + 8))
    # a float64 field spans 8 bytes per element, an interleaved one 3 V elements from its base
    refused(b"stats overlaps an input", f64=1, stats=at(3, 8 * 3 * V - 8))
    refused(b"stats overlaps an input", cs=1, vs=3, stats=at(3, 4 * 3 * V - 4 - (4 * 3 * V - 4) % 8))
