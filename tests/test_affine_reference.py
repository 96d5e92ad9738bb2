"""CPU checks of the affine arithmetic, no device needed: the numpy restatement against closed forms, the header the kernels
compile (csrc/affine_core.h) run on the host under AddressSanitizer and UndefinedBehaviorSanitizer -- a stand-alone program,
tools/affine_host.cpp, with the sanitizer runtimes linked in and started as a child process, so that no library has to be preloaded
anywhere -- against the restatement bit for bit for the field, and the capture of the reference's own least_trimmed_squares
(tests/golden/affine_lts.npz, written by tests/golden/make_golden_affine.py) against the restatement's float64 loop."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "affine_lts.npz")
IDENTITY = np.eye(4, dtype=np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normal", [0, 1])
def test_an_exact_affine_pair_is_recovered(normal):
    g = np.random.default_rng(1)
    F = np.c_[g.uniform(-1, 1, (50, 3)), np.ones(50)]
    M = F @ R.X_TRUE
    X, cond = R.fit64(F, M, normal)
    assert cond < 1e3 and np.abs(X - R.X_TRUE).max() <= 64 * cond * R.EPS64
    assert np.abs(R.lts64(F, M, 4, normal) - R.X_TRUE).max() <= 64 * 1e3 * R.EPS64
    if not normal:
        assert np.abs(X - np.linalg.lstsq(F, M, rcond=None)[0]).max() <= 64 * cond * R.EPS64


def test_the_two_equations_differ_on_noisy_points():
    f, m, _ = R.points(501, seed=12, noise=1e-2)
    X0, X1 = R.fit64(f, m, 0)[0], R.fit64(f, m, 1)[0]
    assert 1e-6 < np.abs(X0 - X1).max() < 1e-2           # the reference's equation is not the least-squares one; both are near X_TRUE
    assert np.abs(X0 - R.X_TRUE).max() < 5e-3 and np.abs(X1 - R.X_TRUE).max() < 5e-3


def test_a_pure_translation_gives_a_constant_field():
    shape = (6, 4, 8)
    theta = IDENTITY.copy()
    theta[:3, 3] = (2.0 * 4 / 8, -2.0 * 1 / 4, 2.0 * 3 / 6)                  # x along D, y along W, z along H: 4, -1 and 3 voxels (exact floats)
    out = R.field(theta, shape)
    assert np.abs(out - np.array([3.0, -1.0, 4.0])).max() <= R.identity_bound(shape)


@pytest.mark.parametrize("shape", R.FIELD_SHAPES)
def test_the_identity_gives_u_back(shape):
    u = R.smooth_field(shape)
    bound = R.identity_bound(shape)
    assert bound == 16.0 * max(shape) * 2.0 ** -53
    assert np.abs(R.field(IDENTITY, shape, u) - u).max() <= bound
    assert np.abs(R.field(IDENTITY, shape)).max() <= bound


def test_a_non_finite_displacement_stays_in_its_voxel():
    shape = (4, 5, 6)
    u = np.array(R.smooth_field(shape))
    u[1, 2, 3, 0], u[2, 0, 5, 2] = np.nan, np.inf
    out, clean = R.field(R.THETA, shape, u), R.field(R.THETA, shape, R.smooth_field(shape))
    bad = ~np.isfinite(out).all(-1)
    assert bad.sum() == 2 and bad[1, 2, 3] and bad[2, 0, 5]
    assert same_bits(out[~bad], clean[~bad])


def test_the_field_is_the_affine_grid_map():
    """affine_grid's own coordinates (torch, CPU, float64), un-normalised, minus the voxel index"""
    import torch
    shape = (5, 4, 7)
    grid = torch.nn.functional.affine_grid(torch.from_numpy(R.THETA.astype(np.float64))[None], (1, 1) + shape, align_corners=False)[0].numpy()
    q = np.stack([((grid[..., 2 - a] + 1.0) * shape[a] - 1.0) / 2.0 for a in range(3)], -1)
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)
    assert np.abs(R.field(R.THETA, shape) - (q - x)).max() <= 16 * R.identity_bound(shape)


# ---- the reference's own function --------------------------------------------------------------------------------------------------
def test_golden_capture_is_the_equation_the_restatement_states():
    z = np.load(GOLDEN)
    tags = sorted({k.split("_")[0] for k in z.files})
    assert tags == ["clean", "noisy"]
    for tag in tags:
        f, m = z[tag + "_fixed"], z[tag + "_moving"]
        assert f.dtype == m.dtype == np.float32 and f.shape == m.shape and f.shape[1] == 4
        for key in [k for k in z.files if k.startswith(tag + "_ref")]:
            k = int(key[len(tag) + 4:])
            ref, f64 = z[key], z["%s_f64_%d" % (tag, k)]
            assert ref.dtype == np.float32 and f64.dtype == np.float64 and ref.shape == f64.shape == (4, 4)
            mine = R.lts64(f, m, k, 1)
            # the same equation on the same rows: numpy's and torch's float64 LU differ by rounding only
            assert np.abs(mine - f64).max() <= 1e-11, (tag, k)
            assert np.abs(ref - f64).max() <= 1e-4, (tag, k)       # and the float32 run is a float32 run of it


# ---- the header on the host, under sanitizers --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the host-arithmetic test needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("affine_host") / "affine_host")
    header = os.path.join(ROOT, "convexadam_amd", "csrc", "affine_core.h")
    assert os.path.exists(header), "csrc/affine_core.h: the affine arithmetic as a plain-C++ header"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.dirname(header), os.path.join(ROOT, "tools", "affine_host.cpp"), "-o", exe]
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
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "", "affine_host %s: exit %d\n%s" % (args, r.returncode, r.stderr[-4000:])
    raw = open(out, "rb").read()
    assert len(raw) == nbytes
    return raw


def test_host_field_under_sanitizers_equals_the_restatement(host_program, tmp_path):
    for i, shape in enumerate(R.FIELD_SHAPES):
        H, W, D = shape
        V = H * W * D
        raw = _run(host_program, ["field", H, W, D, 1, 0, 0], str(tmp_path), [R.THETA], 24 * V)
        assert same_bits(np.frombuffer(raw, np.float64).reshape(shape + (3,)), R.field(R.THETA, shape)), shape
        for f64 in (1, 0):
            planar = (i + f64) % 2
            u = R.smooth_field(shape).astype(np.float64 if f64 else np.float32)
            raw = _run(host_program, ["field", H, W, D, f64, planar, 1], str(tmp_path), [R.THETA, R.layouts(u, u.dtype, planar)], 24 * V)
            assert same_bits(np.frombuffer(raw, np.float64).reshape(shape + (3,)), R.field(R.THETA, shape, u)), (shape, f64)
    # a NaN and an Inf in the field: the sanitizers see no out-of-range conversion or index
    shape = (4, 5, 6)
    u = np.array(R.smooth_field(shape))
    u[1, 2, 3, 0], u[2, 0, 5, 2] = np.nan, -np.inf
    raw = _run(host_program, ["field", 4, 5, 6, 1, 0, 1], str(tmp_path), [R.THETA, u], 24 * 120)
    got, want = np.frombuffer(raw, np.float64).reshape(shape + (3,)), R.field(R.THETA, shape, u)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and same_bits(np.nan_to_num(got, nan=7.0), np.nan_to_num(want, nan=7.0))


def test_host_solve_under_sanitizers(host_program, tmp_path):
    f, m, _ = R.points(65, seed=2)
    for normal, nrhs in ((0, 3), (1, 4)):
        A, B = R.system(R.homogeneous(f), R.homogeneous(m), normal)
        raw = _run(host_program, ["solve", nrhs], str(tmp_path), [np.ascontiguousarray(np.c_[A, B])], 136)
        X, status = np.frombuffer(raw, np.float64, 16).reshape(4, 4), int(np.frombuffer(raw, np.int64, 1, 128)[0])
        want, cond = R.fit64(f, m, normal)
        assert status == 0 and cond < 1e3
        assert np.abs(X[:, :nrhs] - want[:, :nrhs]).max() <= 64 * cond * R.EPS64 * np.abs(want).max()
    # an exact zero pivot (a plane at integer coordinates), a NaN moment, a needed row exchange
    g = np.random.default_rng(3)
    P = np.c_[g.integers(-5, 6, (40, 2)).astype(np.float64), np.zeros(40), np.ones(40)]
    raw = _run(host_program, ["solve", 3], str(tmp_path), [np.ascontiguousarray(np.c_[P.T @ P, P.T @ P])], 136)
    assert int(np.frombuffer(raw, np.int64, 1, 128)[0]) == 2 and not np.frombuffer(raw, np.float64, 16).any()
    bad = np.c_[np.eye(4), np.eye(4)]
    bad[2, 5] = np.nan
    raw = _run(host_program, ["solve", 4], str(tmp_path), [bad], 136)
    assert int(np.frombuffer(raw, np.int64, 1, 128)[0]) == 1
    perm = np.eye(4)[[2, 0, 3, 1]] * np.array([3.0, -2.0, 0.5, 7.0])
    rhs = g.standard_normal((4, 4))
    raw = _run(host_program, ["solve", 4], str(tmp_path), [np.ascontiguousarray(np.c_[perm, rhs])], 136)
    assert int(np.frombuffer(raw, np.int64, 1, 128)[0]) == 0
    assert np.abs(np.frombuffer(raw, np.float64, 16).reshape(4, 4) - np.linalg.solve(perm, rhs)).max() <= 1e-14
