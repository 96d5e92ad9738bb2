"""The field operators of csrc/fieldops.hip on the device against the numpy restatement, bit for bit (run on the MI355X box with `-m gpu`).

Inputs (tests/fieldops_restatement.py): seven smooth fields whose offset pushes most coordinates through the border clamp -- shapes with
extents of 1, a row of 131 and one shape that exceeds the workgroup footprint on every axis by a non-multiple --, a folded field on which
the iteration cannot converge, and an affine field with a closed-form inverse.  Every restatement is computed once per module."""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldops_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SETTINGS = ((40, 0.0), (60, 1e-6))                 # (max_iters, tol)
FIELDS = ["smooth%d-%s" % (i, "x".join(map(str, s))) for i, s in enumerate(R.SMOOTH_SHAPES)] + ["folded"]


def field(name):
    return R.folded_field() if name == "folded" else R.smooth_set()[int(name[6:name.index("-")])]


@functools.lru_cache(maxsize=None)
def restated(name, f64, max_iters, tol):
    return R.invert(field(name).astype(np.float64 if f64 else np.float32), max_iters, tol)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _field
    return _field.lib()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def strides(shape, planar):
    return (shape[0] * shape[1] * shape[2], 1) if planar else (1, 3)


def as_hwd3(t, planar):
    a = t.cpu().numpy()
    return np.ascontiguousarray(np.moveaxis(a, 0, -1)) if planar else a


def run_invert(L, u, u64, u_planar, v64, v_planar, max_iters, tol, optional=True):
    """u (H, W, D, 3) numpy -> dict(v (H, W, D, 3) in the output type, residual, iters, stats), the status checked"""
    shape = u.shape[:3]
    ut = torch.from_numpy(R.layouts(u, np.float64 if u64 else np.float32, u_planar)).to(DEV)
    vt = torch.empty((3,) + shape if v_planar else shape + (3,), dtype=torch.float64 if v64 else torch.float32, device=DEV)
    res = torch.empty(shape, dtype=torch.float64, device=DEV) if optional else None
    it = torch.empty(shape, dtype=torch.uint8, device=DEV) if optional else None
    st = torch.full((3,), -7, dtype=torch.int64, device=DEV) if optional else None
    rc = L.cvx_field_invert_f64(p(ut), int(u64), *strides(shape, u_planar), *shape, max_iters, tol, p(vt), int(v64), *strides(shape, v_planar),
                                p(res), p(it), p(st), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, L.cvx_last_error()
    out = dict(v=as_hwd3(vt, v_planar))
    if optional:
        out.update(residual=res.cpu().numpy(), iters=it.cpu().numpy(), stats=st.cpu().numpy())
    return out


def run_compose(L, a, b, a64, a_planar, b64, b_planar, o64, o_planar):
    shape = a.shape[:3]
    at = torch.from_numpy(R.layouts(a, np.float64 if a64 else np.float32, a_planar)).to(DEV)
    bt = torch.from_numpy(R.layouts(b, np.float64 if b64 else np.float32, b_planar)).to(DEV)
    ot = torch.empty((3,) + shape if o_planar else shape + (3,), dtype=torch.float64 if o64 else torch.float32, device=DEV)
    rc = L.cvx_field_compose_f64(p(at), int(a64), *strides(shape, a_planar), p(bt), int(b64), *strides(shape, b_planar), *shape, p(ot), int(o64),
                                 *strides(shape, o_planar), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, L.cvx_last_error()
    return as_hwd3(ot, o_planar)


@pytest.mark.parametrize("name", FIELDS)
def test_invert_equals_the_restatement_bit_for_bit(L, name):
    u = field(name)
    for max_iters, tol in SETTINGS:
        for u64, u_planar, v64, v_planar in itertools.product((0, 1), repeat=4):
            want = restated(name, u64, max_iters, tol)
            got = run_invert(L, u, u64, u_planar, v64, v_planar, max_iters, tol)
            tag = (name, max_iters, tol, u64, u_planar, v64, v_planar)
            assert same_bits(got["v"], want["v"].astype(np.float64 if v64 else np.float32)), tag
            assert same_bits(got["residual"], want["residual"]), tag
            assert same_bits(got["iters"], want["iters"]), tag
            assert same_bits(got["stats"], want["stats"]), tag


@pytest.mark.parametrize("name", FIELDS)
def test_convergence_counts(L, name):
    got = run_invert(L, field(name), 1, 0, 1, 0, 60, 1e-6)
    want = restated(name, 1, 60, 1e-6)
    print("%s: not converged %d, non-finite %d, max residual %.3g, iterations up to %d" %
          (name, got["stats"][0], got["stats"][1], got["stats"][2:].view(np.float64)[0], got["iters"].max()))
    if name == "folded":
        assert int(got["stats"][0]) == int(want["stats"][0]) == 180          # 37.5 % of 6 x 5 x 16
    else:
        assert int(got["stats"][0]) == 0, "a smooth field (neighbour differences of 0.25 voxel) must converge to 1e-6 within 60 iterations"
    assert int(got["stats"][1]) == 0
    assert run_invert(L, field(name), 1, 0, 1, 0, 40, 0.0)["stats"][0] == 0, "tol = 0 counts nothing as not converged"


def test_one_iteration_and_one_voxel(L):
    for name in (FIELDS[0], FIELDS[5], "folded"):
        for u_planar, v_planar in ((0, 1), (1, 0)):
            got = run_invert(L, field(name), 1, u_planar, 1, v_planar, 1, 0.0)
            want = restated(name, 1, 1, 0.0)
            assert all(same_bits(got[k], want[k]) for k in ("v", "residual", "iters", "stats")), name
            assert int(got["iters"].max()) == 1
    u = field(FIELDS[5])
    assert u.shape == (1, 1, 1, 3)
    got = run_invert(L, u, 0, 0, 0, 0, 60, 1e-6)
    assert same_bits(got["v"], (-u).astype(np.float32)) and float(got["residual"][0, 0, 0]) == 0.0 and int(got["iters"][0, 0, 0]) == 1


def test_optional_outputs_may_be_null(L):
    for name in (FIELDS[2], "folded"):
        got = run_invert(L, field(name), 0, 1, 1, 0, 60, 1e-6, optional=False)
        assert same_bits(got["v"], restated(name, 0, 60, 1e-6)["v"])


def test_two_runs_give_identical_bytes(L):
    for name in (FIELDS[2], FIELDS[6], "folded"):
        a = run_invert(L, field(name), 0, 0, 0, 1, 60, 1e-6)
        b = run_invert(L, field(name), 0, 0, 0, 1, 60, 1e-6)
        assert all(same_bits(a[k], b[k]) for k in a), name


def test_planted_nan_and_inf_stay_local(L):
    clean = np.array(field(FIELDS[0]))
    plants = ((1, 1, 2), (2, 1, 1))
    u = clean.copy()
    u[plants[0]][1] = np.nan
    u[plants[1]][0] = np.inf
    reach = float(np.abs(clean).max()) + 2.0
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in clean.shape[:3]], indexing="ij"), -1)
    far = np.ones(clean.shape[:3], bool)
    for q in plants:
        far &= np.abs(idx - np.array(q)).max(-1) > reach
    assert far.sum() > 200
    for max_iters, tol in SETTINGS:
        got = run_invert(L, u, 1, 0, 1, 0, max_iters, tol)                    # run_invert asserts CVX_OK
        ref = run_invert(L, clean, 1, 0, 1, 0, max_iters, tol)
        assert int(got["stats"][1]) >= 1 and np.isnan(got["residual"][plants[0]]) and np.isnan(got["residual"][plants[1]])
        for k in ("v", "residual", "iters"):
            assert same_bits(got[k][far], ref[k][far]), k
        want = R.invert(u, max_iters, tol)
        assert all(same_bits(got[k], want[k]) for k in ("v", "residual", "iters", "stats"))
        bad = np.isnan(got["residual"])
        assert int(got["stats"][1]) == int(bad.sum()) and np.isnan(got["v"][bad]).all() and np.isfinite(got["v"][~bad]).all()


def test_affine_field_reaches_the_true_inverse_inside(L):
    u, v_true, inside, Lip = R.affine_field()
    k = 60
    got = run_invert(L, u, 1, 0, 1, 0, k, 0.0)
    err = np.abs(got["v"] - v_true).max(-1)
    bound = R.affine_bound(u, Lip, k)
    print("affine field on the device: error inside %.3g, bound %.3g" % (err[inside].max(), bound))
    assert float(err[inside].max()) <= bound


def test_compose_equals_the_restatement_and_the_residual(L):
    for name in (FIELDS[1], FIELDS[2], FIELDS[6], "folded"):
        u = field(name)
        w = restated(name, 1, 40, 0.0)
        for a64, a_planar, b64, b_planar, o64, o_planar in itertools.product((0, 1), repeat=6):
            a = u.astype(np.float64 if a64 else np.float32)
            b = w["v"].astype(np.float64 if b64 else np.float32)
            got = run_compose(L, a, b, a64, a_planar, b64, b_planar, o64, o_planar)
            assert same_bits(got, R.compose(a, b).astype(np.float64 if o64 else np.float32)), (name, a64, a_planar, b64, b_planar, o64, o_planar)
        got = run_compose(L, u, w["v"], 1, 0, 1, 1, 1, 0)
        assert same_bits(np.abs(got).max(-1), w["residual"]), "compose(u, v) is the vector whose max-norm the inverter reports"
    u = np.array(field(FIELDS[1]))
    u[2, 3, 4, 2] = np.nan
    got = run_compose(L, field(FIELDS[1]), u, 1, 0, 1, 0, 1, 0)
    assert same_bits(got, R.compose(field(FIELDS[1]), u)) and np.isnan(got[2, 3, 4]).all()


def test_python_functions_host_and_device():
    from convexadam_amd.apply_convex import apply_convex
    from convexadam_amd.convex_adam_utils import apply_convex_inverse, compose_fields, invert_field
    u = field(FIELDS[0])
    want = R.invert(u, 50, 1e-4)
    # host array in, float64 array out
    v, info = invert_field(u, return_info=True)
    assert isinstance(v, np.ndarray) and same_bits(v, want["v"])
    assert same_bits(info["residual"], want["residual"]) and same_bits(info["iters"], want["iters"])
    assert (info["not_converged"], info["non_finite"]) == (0, 0) and info["max_residual"] == float(want["residual"].max())
    assert same_bits(invert_field(u, max_iters=7, tol=0.0), R.invert(u, 7, 0.0)["v"])
    # a float32 host tensor is computed in float64 like every host input
    u32 = u.astype(np.float32)
    assert same_bits(invert_field(torch.from_numpy(u32)), R.invert(u32, 50, 1e-4)["v"])
    # device tensors keep layout and dtype and stay on the device
    want32 = R.invert(u32, 50, 1e-4)
    for planar in (False, True):
        t = torch.from_numpy(R.layouts(u32, np.float32, planar)).to(DEV)
        r, info = invert_field(t, return_info=True)
        assert r.is_cuda and r.dtype == torch.float32 and r.shape == t.shape and info["residual"].is_cuda and info["iters"].is_cuda
        assert same_bits(as_hwd3(r, planar), want32["v"].astype(np.float32))
        assert same_bits(info["residual"].cpu().numpy(), want32["residual"])
        c = compose_fields(t, r)
        assert c.is_cuda and c.dtype == torch.float32 and c.shape == t.shape
        assert same_bits(as_hwd3(c, planar), R.compose(u32, want32["v"].astype(np.float32)).astype(np.float32))
    t64 = torch.from_numpy(np.array(u)).to(DEV)
    assert same_bits(invert_field(t64).cpu().numpy(), want["v"])
    # composition through host arrays: the residual vector
    c = compose_fields(u, v)
    assert isinstance(c, np.ndarray) and same_bits(c, R.compose(u, want["v"])) and float(np.abs(c).max()) <= 1e-4
    # the fixed image in the moving frame
    fixed = np.random.default_rng(11).random(u.shape[:3])
    assert same_bits(apply_convex_inverse(u, fixed), apply_convex(want["v"], fixed))
    assert same_bits(apply_convex_inverse(t64, fixed, max_iters=9, tol=0.0), apply_convex(R.invert(u, 9, 0.0)["v"], fixed))
    tp = torch.from_numpy(R.layouts(u, np.float64, True)).to(DEV)
    assert same_bits(apply_convex_inverse(tp, fixed), apply_convex(want["v"], fixed))
    with pytest.raises(ValueError):
        invert_field(np.zeros((4, 5, 6)))
    with pytest.raises(ValueError):
        compose_fields(u, np.zeros((3, 3, 3, 3)))


def test_command_line_inverts_a_nifti_field(tmp_path, capsys):
    from convexadam_amd import fieldops, nifti_io
    u = field(FIELDS[1]).astype(np.float32)
    src, dst = str(tmp_path / "disp.nii.gz"), str(tmp_path / "inv.nii.gz")
    nifti_io.save_image(u, np.diag([1.5, 1.5, 2.0, 1.0]), src)
    assert fieldops.main(["--input_field", src, "--output_inverse", dst, "--max_iters", "30", "--tol", "1e-5"]) == 0
    line = capsys.readouterr().out
    want = R.invert(u, 30, 1e-5)
    assert "0 of 693 voxels not converged" in line and ("max residual %.6g" % want["residual"].max()) in line
    assert same_bits(nifti_io.load_fdata(dst).astype(np.float32), want["v"].astype(np.float32))
    assert np.array_equal(nifti_io.load_affine(dst), nifti_io.load_affine(src))
