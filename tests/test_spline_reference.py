"""CPU checks of the cubic B-spline arithmetic, no device needed: the numpy restatement (tests/spline_restatement.py) against
scipy.ndimage's spline_filter and map_coordinates, order 3 with the defaults apply_convex uses, inside the bound the restatement module
states; and the header the kernels compile (csrc/spline_core.h) run on the host under AddressSanitizer and UndefinedBehaviorSanitizer -- a
stand-alone program, tools/spline_host.cpp, with the sanitizer runtimes linked in and started as a child process, so that no library has
to be preloaded anywhere -- against the restatement bit for bit on every case."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spline_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_list_is_the_one_the_kernels_need():
    assert len(R.SHAPES) == 11 and (3, 5, 131) in R.SHAPES and (1, 1, 1) in R.SHAPES
    assert {min(s) for s in R.SHAPES} >= {1, 2, 3} and max(s[2] for s in R.SHAPES) > 64 + 32 and max(s[0] for s in R.SHAPES) > 64
    for shape in R.SHAPES:
        c = R.coordinates(shape)
        assert c.shape[1] == 3 and len(c) >= R.N_RANDOM + 20 and c.dtype == np.float64
        inside = R.is_inside(shape, c)
        assert 2 * int(inside.sum()) >= len(c), shape
        assert np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any() and (c == 1e300).any()
        for a, n in enumerate(shape):
            assert (c[:, a] == -1e-9).any() and (c[:, a] == n - 1 + 1e-9).any()
            if n == 1:
                assert (c[:R.N_RANDOM * 3 // 4, a] == 0.0).all()
        assert (np.abs(R.volume(shape)) >= 0.25 * R.MAGNITUDE).all()


def test_restatement_equals_scipy_inside_the_stated_bound():
    worst_c = worst_v = 0.0
    for k, shape in enumerate(R.SHAPES):
        for dtype in (np.float64, np.float32):
            vol = R.volume(shape, k, dtype)
            scale = float(np.abs(vol).max())
            coef = R.prefilter(vol)
            assert coef.dtype == np.float64
            want_c = ndimage.spline_filter(vol.astype(np.float64), order=3, mode="constant", output=np.float64)
            dc = float(np.abs(coef - want_c).max()) / scale
            c = R.coordinates(shape, k)
            got = R.map_cubic(coef, c)
            want = ndimage.map_coordinates(vol.astype(np.float64), c.T, order=3, mode="constant", cval=0.0, prefilter=True)
            dv = float(np.abs(got - want).max()) / scale
            print("%-12s %s: coefficients %.3e, values %.3e of max|volume|" % (shape, np.dtype(dtype).name, dc, dv))
            worst_c, worst_v = max(worst_c, dc), max(worst_v, dv)
            assert dc <= R.SCIPY_BOUND_COEF and dv <= R.SCIPY_BOUND_VALUE, (shape, dc, dv)
            # the same points are outside for both, and inside both answer: a kernel that says 0 everywhere cannot pass
            inside = R.is_inside(shape, c)
            assert 2 * int(inside.sum()) >= len(c)
            assert (got[~inside] == 0.0).all() and (want[~inside] == 0.0).all()
            assert (got[inside] != 0.0).all() and (want[inside] != 0.0).all(), shape
    print("restatement against scipy: coefficients %.3e, values %.3e of max|volume| (stated: %.1e, %.1e)"
          % (worst_c, worst_v, R.MEASURED_COEF, R.MEASURED_VALUE))
    assert R.MEASURED_COEF < 1e-12 and R.MEASURED_VALUE < 1e-12, "a figure this large says the statement is wrong, not the tolerance"
    assert R.SCIPY_BOUND_COEF == 64 * R.MEASURED_COEF and R.SCIPY_BOUND_VALUE == 64 * R.MEASURED_VALUE


def test_restatement_known_answers():
    # a constant volume has constant coefficients and interpolates to the constant; integer coordinates return the samples
    for shape in ((5, 6, 7), (1, 4, 5), (2, 3, 4)):
        const = np.full(shape, 7.25)
        coef = R.prefilter(const)
        assert np.abs(coef - 7.25).max() <= R.SCIPY_BOUND_COEF * 7.25
        c = R.coordinates(shape)
        inside = R.is_inside(shape, c)
        assert np.abs(R.map_cubic(coef, c)[inside] - 7.25).max() <= R.SCIPY_BOUND_VALUE * 7.25
        vol = R.volume(shape, 3)
        grid = R.warp_coordinates(shape, np.zeros(shape + (3,)))
        assert np.abs(R.map_cubic(R.prefilter(vol), grid) - vol.reshape(-1)).max() <= R.SCIPY_BOUND_VALUE * np.abs(vol).max()
    # the ITK rule: the half voxel beyond the last sample is inside and clamped onto it, everything further out is the default
    vol = R.volume((5, 6, 7), 4)
    coef = R.prefilter(vol)
    pts = np.array([[-0.5, 0, 0], [4.5, 5.5, 6.5], [-0.5000001, 0, 0], [0, 5.5000001, 0], [np.nan, 0, 0], [0, 0, np.inf], [1e300, 0, 0]])
    got = R.itk_cubic(coef, pts, default=-3.0)
    assert got[2:].tolist() == [-3.0] * 5
    assert abs(got[0] - vol[0, 0, 0]) <= R.SCIPY_BOUND_VALUE * R.MAGNITUDE and abs(got[1] - vol[4, 5, 6]) <= R.SCIPY_BOUND_VALUE * R.MAGNITUDE
    assert R.mirror(np.array([-1, 0, 3, 4, 5, -2]), 4).tolist() == [1, 0, 3, 2, 1, 2] and R.mirror(np.array([-1, 2, 3]), 2).tolist() == [1, 0, 1]
    assert R.mirror(np.array([-1, 0, 2]), 1).tolist() == [0, 0, 0]
    w = R.weights(np.array([0.0, 0.25, 0.5]))
    assert [float(x[0]) for x in w][:3] == [1.0 / 6.0, 4.0 / 6.0, 1.0 / 6.0] and np.abs(sum(w) - 1.0).max() <= 2.3e-16


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the host-arithmetic test needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("spline_host") / "spline_host")
    header = os.path.join(ROOT, "convexadam_amd", "csrc", "spline_core.h")
    assert os.path.exists(header), "csrc/spline_core.h: the spline arithmetic as a plain-C++ header"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.dirname(header), os.path.join(ROOT, "tools", "spline_host.cpp"), "-o", exe]
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run(cmd + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode == 0:
            return exe
    raise AssertionError("%s\n%s" % (" ".join(cmd), r.stdout))


def host_run(exe, tmp, vol, coords, default):
    src, pts, out = (os.path.join(tmp, n) for n in ("src.bin", "pts.bin", "out.bin"))
    vol.tofile(src)
    np.ascontiguousarray(coords, np.float64).tofile(pts)
    args = [exe] + [str(s) for s in vol.shape] + ["2" if vol.dtype == np.float64 else "1", str(len(coords)), repr(float(default)), src, pts, out]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "", "spline_host %s: exit %d\n%s" % (args[1:7], r.returncode, r.stderr[-4000:])
    raw = np.fromfile(out, np.float64)
    assert raw.size == vol.size + 2 * len(coords)
    return raw[:vol.size].reshape(vol.shape), raw[vol.size:vol.size + len(coords)], raw[vol.size + len(coords):]


def test_host_arithmetic_under_sanitizers_equals_the_restatement(host_program, tmp_path):
    n = 0
    for k, shape in enumerate(R.SHAPES):
        for dtype in (np.float64, np.float32):
            vol = R.volume(shape, k, dtype)
            c = R.coordinates(shape, k)
            coef, mapped, itk = host_run(host_program, str(tmp_path), vol, c, -2.5)
            want = R.prefilter(vol)
            assert np.array_equal(coef, want), (shape, dtype)
            assert np.array_equal(mapped, R.map_cubic(want, c)), (shape, dtype)
            assert np.array_equal(itk, R.itk_cubic(want, c, -2.5)), (shape, dtype)
            inside = R.is_inside(shape, c)
            assert (mapped[inside] != 0.0).all() and (mapped[~inside] == 0.0).all() and (itk != 0.0).all()
            n += 1
    assert n == 22


def test_host_arithmetic_on_non_finite_samples(host_program, tmp_path):
    """a NaN or an infinite sample poisons its lines and never becomes an index; the program ends clean"""
    vol = R.volume((5, 6, 7), 9)
    vol[2, 3, 4] = np.nan
    vol[0, 0, 0] = np.inf
    c = R.coordinates(vol.shape, 9)
    coef, mapped, itk = host_run(host_program, str(tmp_path), vol, c, 0.0)
    want = R.prefilter(vol)
    assert np.isnan(want).any() and np.array_equal(coef, want, equal_nan=True)
    assert np.array_equal(mapped, R.map_cubic(want, c), equal_nan=True) and np.array_equal(itk, R.itk_cubic(want, c), equal_nan=True)
    assert (mapped[~R.is_inside(vol.shape, c)] == 0.0).all()
