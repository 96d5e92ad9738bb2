"""The inputs of tests/mind_range_cases.py on the CPU: each case does what its name claims, and the oracle's MIND-SSC equals the reference's
on all of them -- live against the upstream MINDSSC where its tree is present (skipped elsewhere), and against its captures
(tests/golden/mind_range.npz, made by tests/golden/make_golden_mind_range.py) everywhere.  Never part of the `-m gpu` selection.

What the reference does at the edges:
  * any NaN or +-Inf voxel gives an all-NaN descriptor: the NaN reaches `mind_var.mean()` (an infinite voxel through 0 * Inf in the one-hot
    shift convolutions), and torch.clamp with a NaN bound returns NaN;
  * where V mean(variance) >= 2^128 torch's float32 sum is Inf, both bounds are Inf and every value is 1: the oracle reproduces that under
    set_mean_threads(T) and returns proper descriptors with its exactly rounded mean (the recorded deviation);
  * where 1000 mean exceeds float32 but the sum does not overflow (small volumes only) the reference raises; the oracle clamps with hi = Inf."""
import contextlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import mind_range_cases as MC  # noqa: E402
from make_golden_live import digest  # noqa: E402

EXP_ULP = 6e-8                    # MKL vsExp vs the expf restatement: <= 1 ulp of a value in (0.5, 1] (test_oracle_vs_reference_live.py)
F32_MAX = float(np.finfo(np.float32).max)


@contextlib.contextmanager
def reference_exp(orc, mkl, threads=8):
    """The oracle in reference-bits mode, as in test_oracle_vs_reference_live.py (a file that does not travel to every host): the capture
    host's MKL exp as a table and torch's `threads`-thread mean."""
    t = mkl.golden_tables()
    orc.set_exp_table(t["exp"], t["exp_first"], t["exp_count"])
    orc.set_mean_threads(threads)
    try:
        yield
    finally:
        orc.set_exp_table(None)
        orc.set_mean_threads(0)


@pytest.fixture(scope="module")
def ref(golden):
    return golden("mind_range")


@pytest.fixture(scope="module")
def exact(orc):
    """name -> (descriptor, mean) of the oracle with its exactly rounded mean, computed once"""
    out = {}
    for c in MC.CASES:
        m, gm = orc.mindssc(c.img, c.radius, c.dilation, return_mean=True)
        m.setflags(write=False)
        out[c.name] = m, gm
    return out


def log2_sum(c, gm):
    """log2 of V mean(variance), from the oracle's exactly rounded mean"""
    return float(np.log2(float(gm)) + np.log2(c.img.size)) if gm > 0 else -np.inf


def sum_overflows(c, gm):
    s = log2_sum(c, gm)
    assert not 127.9 < s < 128.1, "%s: V mean = 2^%.3f is too close to float32's end to say what torch's sum does" % (c.name, s)
    return s >= 128


def reference_raises(c, gm):
    """torch.clamp refuses a finite bound beyond float32: 1000 mean, where the sum itself did not overflow"""
    return np.isfinite(gm) and not sum_overflows(c, gm) and float(gm) * 1000.0 > F32_MAX


# ---- the table is the one the issue asks for ------------------------------------------------------------------------------------------------
def test_the_list_is_the_matrix_of_the_issue():
    names = set(MC.NAMES)
    kinds = ("base", "base@e-40", "base@e40", "base@e-62", "base@x1e-22", "base@x1e-23", "base@x1e-24", "top", "block@x1e17", "voxel_1e18",
             "nan_interior", "nan_first", "nan_last", "nan_face", "nan_all", "pos_inf", "neg_inf")
    for shape, r, d, _ in MC.SHAPES:
        for k in kinds:
            assert "%s/%s" % (k, MC.tag(shape)) in names, (k, shape)
        assert min(shape) >= 2 * d, "a voxel of %r that no shifted tap reads" % (shape,)
    assert [(s, r, d) for s, r, d, _ in MC.SHAPES] == [((12, 14, 64), 1, 2), ((13, 19, 92), 1, 2), ((7, 9, 15), 1, 2), ((6, 6, 6), 1, 2), ((9, 10, 12), 2, 2), ((9, 9, 33), 3, 4)]
    big = MC.tag(MC.OVERFLOW_ONLY[0])
    assert [n for n in MC.NAMES if n.endswith("/" + big)] == ["sum_overflow/" + big] and np.prod(MC.OVERFLOW_ONLY[0]) >= 32768
    # the sum-overflow case wherever the shape has the voxels for it: every radius-1 shape but the smallest
    assert {n.split("/")[1] for n in names if n.startswith("sum_overflow/")} == {"12x14x64", "13x19x92", "7x9x15", big}
    assert {c.cls for c in MC.CASES} == set(MC.CLASSES)
    for c in MC.CASES:
        assert c.img.shape == c.shape and c.img.dtype == np.float32 and c.img.flags.c_contiguous, c.name
        assert np.isfinite(c.img).all() == (c.cls != "nonfinite"), c.name
    assert np.array_equal(MC.base((12, 14, 16)), (np.random.default_rng(0).standard_normal((12, 14, 16)) * 10).astype(np.float32))


def test_scaled_inputs_are_what_they_claim():
    for shape, r, d, _ in MC.SHAPES:
        t = MC.tag(shape)
        b = MC.case("base/" + t).img.astype(np.float64)
        for e in (-40, 40, -62):
            assert np.array_equal(MC.case("base@e%d/%s" % (e, t)).img.astype(np.float64), b * 2.0 ** e), (e, t)
        # squared differences partly denormal at 2^-62, all of them below the normal range from 1e-22 down
        for kind, lo, hi in (("base@e-62", 0.001, 0.5), ("base@x1e-22", 1.0, 1.0), ("base@x1e-23", 1.0, 1.0)):
            img = MC.case("%s/%s" % (kind, t)).img.astype(np.float64)
            sq = np.diff(img, axis=2) ** 2
            frac = float(((sq > 0) & (sq < 2.0 ** -126)).mean())
            assert lo <= frac <= hi, (kind, t, frac)
        top = MC.case("top/" + t).img
        assert MC.CONTRACT_LOG2 - 1e-5 < MC.contract_log2(top, r) <= MC.CONTRACT_LOG2, t
        assert MC.contract_log2(MC.times(top, 1.0 + 2.0 ** -20), r) > MC.CONTRACT_LOG2          # (the check itself: one step beyond is outside)
    for c in MC.CASES:
        if c.cls in ("control", "pow2", "denormal", "zero_mean", "top"):
            assert MC.contract_log2(c.img, c.radius) <= MC.CONTRACT_LOG2, c.name
        if c.cls != "nonfinite":
            sums = MC.patch_sums(c.img, c.radius, c.dilation)
            assert float(sums.max()) < 2.0 ** 127.5, "%s: a patch sum at 2^%.2f" % (c.name, np.log2(sums.max()))
        if c.cls == "sum_overflow":
            got = np.log2(MC.mean_variance(sums, c.radius) * c.img.size)
            assert abs(got - MC.SUM_TARGET_LOG2) < 1e-3, (c.name, got)


def test_the_named_edges_are_in_the_list(exact):
    for c in MC.CASES:
        m, gm = exact[c.name]
        nan, ones = int(np.isnan(m).sum()), int((m == 1).sum())
        if c.cls == "nonfinite":
            assert nan == m.size and np.isnan(gm), c.name
        elif c.cls == "zero_mean":
            assert nan >= 0.999 * m.size and float(gm) * 0.001 < 2.0 ** -150, c.name             # lo rounds to 0
        else:
            assert nan == 0 or c.name == "base@x1e-23/9x9x33", c.name                            # (there 0 / 0 on a few voxels: lo is 0)
            assert ones < m.size, c.name
        if c.cls == "denormal" and "1e-2" in c.name:
            assert 0 < gm < 2.0 ** -126, c.name                                                  # the mean variance itself is denormal
        if c.cls == "clamp":
            # the float64 restatement's variances: the lower bound binds on a large part of the volume.  (The upper one cannot at these sizes:
            # one large voxel reaches some 160 variances, a thousand times their mean needs a volume of 10^5 voxels and more -- the `sparse`
            # input of test_gpu_mind_single.py is that case)
            ssd = MC.patch_sums(c.img, c.radius, c.dilation) / float((2 * c.radius + 1) ** 3)
            var = (ssd - ssd.min(0)).mean(0)
            assert (var < 0.001 * var.mean()).mean() > 0.3 or c.name == "block@x1e17/6x6x6", c.name   # (6x6x6: the block's patches reach every voxel)
        if c.cls == "sum_overflow":
            assert sum_overflows(c, gm) and nan == 0 and ones == m.size // 12, c.name            # exact mean: proper descriptors (one channel is the minimum)
    assert [c.name for c in MC.CASES if c.cls != "nonfinite" and reference_raises(c, exact[c.name][1])] == ["block@x1e17/6x6x6"]
    assert sorted(c.name for c in MC.CASES if c.cls == "top" and sum_overflows(c, exact[c.name][1])) == ["top/12x14x64", "top/13x19x92"]


def test_power_of_two_scales_give_the_same_bits(exact):
    for c in MC.CASES:
        if c.cls == "pow2":
            assert exact[c.name][0].tobytes() == exact[MC.base_name(c.name)][0].tobytes(), c.name


# ---- the oracle against the reference ---------------------------------------------------------------------------------------------------------
def check_against_reference(c, r, bits, mine, gm, tag):
    """r: the reference's descriptor (None: it raised); bits: the oracle in reference-bits mode; mine, gm: the oracle with its own expf and mean"""
    if r is None:
        assert reference_raises(c, gm), "%s %s: the reference raised" % (c.name, tag)
        assert np.isfinite(mine).all() and np.isfinite(bits).all()
        return
    assert not reference_raises(c, gm), "%s %s: the reference should have raised" % (c.name, tag)
    assert np.array_equal(np.isnan(bits), np.isnan(r)), "%s %s: NaN masks differ (%d vs %d NaNs)" % (c.name, tag, np.isnan(bits).sum(), np.isnan(r).sum())
    assert np.array_equal(bits, r, equal_nan=True), "%s %s: %d values differ in reference-bits mode" % (c.name, tag, int((bits != r).sum()))
    if c.cls == "nonfinite":
        assert np.isnan(r).all() and np.isnan(mine).all(), c.name
    elif sum_overflows(c, gm):
        assert (r == 1).all() and np.isfinite(mine).all() and not (mine == 1).all(), c.name
    else:
        assert np.array_equal(np.isnan(mine), np.isnan(r)), c.name
        if not np.isnan(r).all():
            assert np.nanmax(np.abs(mine - r)) <= EXP_ULP, c.name


@pytest.fixture(scope="module")
def upstream():
    try:
        from _ref_import import import_reference, reference_available
    except ImportError:
        pytest.skip("the import harness of the upstream reference is not on this host")
    if not reference_available():
        pytest.skip("the upstream reference tree is not on this host")
    # the repository's own `convexAdam` package (the drop-in front end of the device operators) may be imported already: the reference's
    # package of the same name is imported in its place and both the module table and the path are put back
    mine = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "convexAdam" or k.startswith("convexAdam.")}
    path = list(sys.path)
    try:
        utils = import_reference()[0]
        assert not utils.__file__.startswith(os.path.dirname(HERE)), utils.__file__
    finally:
        for k in [k for k in sys.modules if k == "convexAdam" or k.startswith("convexAdam.")]:
            del sys.modules[k]
        sys.modules.update(mine)
        sys.path[:] = path
    return utils.MINDSSC


@pytest.mark.parametrize("threads", [1, 8])
def test_oracle_equals_the_live_reference(upstream, orc, mkl, exact, threads):
    import torch
    from make_golden_mind_range import reference_descriptor
    if not mkl.host_tables(orc)["matches_golden_host"]:
        pytest.skip("this host's MKL code path differs from the one the exp table was recorded on")
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        for c in MC.CASES:
            r = reference_descriptor(upstream, c)
            with reference_exp(orc, mkl, threads):
                bits = orc.mindssc(c.img, c.radius, c.dilation)
            check_against_reference(c, r, bits, *exact[c.name], tag="%d threads" % threads)
    finally:
        torch.set_num_threads(old)


def test_oracle_equals_the_captures(ref, orc, mkl, exact):
    assert {k.split(":")[0] for k in ref} == set(MC.NAMES), "tests/golden/mind_range.npz was made for another list: run make_golden_mind_range.py"
    arrays = 0
    for c in MC.CASES:
        mine, gm = exact[c.name]
        with reference_exp(orc, mkl, 8):
            bits = orc.mindssc(c.img, c.radius, c.dilation)
        if c.name + ":raises" in ref:
            check_against_reference(c, None, bits, mine, gm, "capture")
            continue
        assert (int(np.isnan(bits).sum()), int((bits == 1).sum())) == (int(ref[c.name + ":nan"]), int(ref[c.name + ":ones"])), c.name
        assert digest(bits) == str(ref[c.name + ":digest"]), c.name
        if c.name + ":out" in ref:
            arrays += 1
            check_against_reference(c, ref[c.name + ":out"], bits, mine, gm, "capture")
        elif c.cls == "nonfinite":
            assert int(ref[c.name + ":nan"]) == bits.size and np.isnan(mine).all(), c.name
        elif sum_overflows(c, gm):
            assert int(ref[c.name + ":ones"]) == bits.size and np.isfinite(mine).all() and not (mine == 1).all(), c.name
        else:
            assert np.array_equal(np.isnan(mine), np.isnan(bits)) and (np.isnan(bits).all() or np.nanmax(np.abs(mine - bits)) <= EXP_ULP), c.name
    assert arrays >= 15, arrays


def test_sum_overflow_under_torchs_mean(orc, exact):
    """set_mean_threads(T), the oracle's own expf: all ones, whatever T; the exact mean: finite, not all ones"""
    for c in MC.CASES:
        if c.cls != "nonfinite" and sum_overflows(c, exact[c.name][1]):
            for T in (1, 8):
                orc.set_mean_threads(T)
                try:
                    assert (orc.mindssc(c.img, c.radius, c.dilation) == 1).all(), (c.name, T)
                finally:
                    orc.set_mean_threads(0)
            mine = exact[c.name][0]
            assert np.isfinite(mine).all() and not (mine == 1).all(), c.name
