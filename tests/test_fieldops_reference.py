"""CPU checks of the field-operator arithmetic, no device needed: the numpy restatement against closed forms, and the
header the kernels compile (csrc/fieldops_core.h) run on the host under AddressSanitizer and UndefinedBehaviorSanitizer -- a stand-alone
program, tools/fieldops_host.cpp, with the sanitizer runtimes linked in and started as a child process, so that no library has to be
preloaded anywhere -- against the restatement bit for bit."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldops_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_constant_field_inverts_to_its_negative_in_one_iteration():
    u = np.zeros((4, 5, 6, 3)) + np.array([1.25, -0.5, 2.0])
    for tol in (0.0, 1e-4):
        w = R.invert(u, max_iters=1 if tol == 0.0 else 50, tol=tol)
        assert same_bits(w["v"], -u) and float(w["residual"].max()) == 0.0
        assert int(w["iters"].max()) == 1 and w["stats"].tolist() == [0, 0, 0]


def test_affine_field_reaches_the_true_inverse_inside():
    u, v_true, inside, L = R.affine_field()
    k = 60
    w = R.invert(u, max_iters=k, tol=0.0)
    err = np.abs(w["v"] - v_true).max(-1)
    bound = R.affine_bound(u, L, k)
    print("affine field: L = %.4f, %.1f %% inside, error inside %.3g, bound %.3g" % (L, 100 * inside.mean(), err[inside].max(), bound))
    assert L < 0.5 and inside.mean() > 0.5 and bound < 1e-12
    assert float(err[inside].max()) <= bound


def test_compose_is_the_residual_vector():
    for u in R.smooth_set()[:3] + (R.folded_field(), R.affine_field()[0]):
        w = R.invert(u, max_iters=12, tol=0.0)
        c = R.compose(u, w["v"])
        assert same_bits(np.abs(c).max(-1), w["residual"])


def test_folded_field_does_not_converge():
    w = R.invert(R.folded_field(), max_iters=40, tol=0.0)
    assert float((w["residual"] > 1e-3).mean()) == 0.375 and float(w["residual"].max()) == 5.0


def test_non_finite_coordinates_never_become_an_index():
    u = np.array(R.smooth_set()[1])
    u[3, 4, 5, 1] = np.nan
    u[1, 2, 3, 0] = np.inf
    w = R.invert(u, max_iters=8, tol=1e-6)
    bad = np.isnan(w["residual"])
    assert bad[3, 4, 5] and bad[1, 2, 3] and int(w["stats"][1]) == int(bad.sum()) >= 2
    assert np.isnan(w["v"][bad]).all() and np.isfinite(w["v"][~bad]).all()


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the host-arithmetic test needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("fieldops_host") / "fieldops_host")
    header = os.path.join(ROOT, "convexadam_amd", "csrc", "fieldops_core.h")
    assert os.path.exists(header), "csrc/fieldops_core.h: the per-voxel arithmetic as a plain-C++ header"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.dirname(header), os.path.join(ROOT, "tools", "fieldops_host.cpp"), "-o", exe]
    # the sanitizer runtimes linked into the program where the compiler offers that (GCC's default is a shared runtime, which insists on
    # being the first library of the process)
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run(cmd + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode == 0:
            return exe
    raise AssertionError("%s\n%s" % (" ".join(cmd), r.stdout))


def _run(exe, args, tmp, inputs, nbytes):
    paths = []
    for i, a in enumerate(inputs):
        paths.append(os.path.join(tmp, "in%d.bin" % i))
        a.tofile(paths[-1])
    out = os.path.join(tmp, "out.bin")
    r = subprocess.run([exe] + [str(a) for a in args] + paths + [out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "", "fieldops_host %s: exit %d\n%s" % (args, r.returncode, r.stderr[-4000:])
    raw = open(out, "rb").read()
    assert len(raw) == nbytes
    return raw


def test_host_arithmetic_under_sanitizers_equals_the_restatement(host_program, tmp_path):
    cases = list(R.smooth_set()) + [R.folded_field()]
    for i, u in enumerate(cases):
        H, W, D = u.shape[:3]
        V = H * W * D
        for f64 in (1, 0):
            planar = (i + f64) % 2
            uu = u.astype(np.float64 if f64 else np.float32)
            for max_iters, tol in ((40, 0.0), (60, 1e-6)):
                raw = _run(host_program, ["invert", H, W, D, f64, planar, max_iters, repr(tol)], str(tmp_path), [R.layouts(uu, uu.dtype, planar)],
                           33 * V + 24)
                want = R.invert(uu, max_iters, tol)
                assert same_bits(np.frombuffer(raw, np.float64, 3 * V).reshape(H, W, D, 3), want["v"]), (u.shape, f64, tol)
                assert same_bits(np.frombuffer(raw, np.float64, V, 24 * V).reshape(H, W, D), want["residual"]), (u.shape, f64, tol)
                assert same_bits(np.frombuffer(raw, np.int64, 3, 32 * V), want["stats"]), (u.shape, f64, tol)
                assert same_bits(np.frombuffer(raw, np.uint8, V, 32 * V + 24).reshape(H, W, D), want["iters"]), (u.shape, f64, tol)
            b = R.invert(uu, 3, 0.0)["v"].astype(uu.dtype)
            raw = _run(host_program, ["compose", H, W, D, f64, planar], str(tmp_path), [R.layouts(uu, uu.dtype, planar), R.layouts(b, uu.dtype, planar)],
                       24 * V)
            assert same_bits(np.frombuffer(raw, np.float64, 3 * V).reshape(H, W, D, 3), R.compose(uu, b)), (u.shape, f64)
    # a NaN and an Inf in the field: the sanitizers see no out-of-range conversion or index
    u = np.array(cases[1])
    u[3, 4, 5, 1], u[1, 2, 3, 0] = np.nan, -np.inf
    H, W, D = u.shape[:3]
    V = H * W * D
    raw = _run(host_program, ["invert", H, W, D, 1, 0, 8, repr(1e-6)], str(tmp_path), [u], 33 * V + 24)
    want = R.invert(u, 8, 1e-6)
    assert same_bits(np.frombuffer(raw, np.float64, 3 * V).reshape(H, W, D, 3), want["v"]) and int(want["stats"][1]) >= 2
    assert same_bits(np.frombuffer(raw, np.int64, 3, 32 * V), want["stats"])
