"""Least-trimmed affine fit and affine displacement field on the GPU (csrc/affine.hip, convexadam_amd/affine.py) against the numpy
restatement (tests/affine_restatement.py) and the capture of the reference's own function (tests/golden/affine_lts.npz).

Criteria:
  fit         acceptance without any tie sensitivity: the returned inlier mask has exactly n // 2 ones (all ones for one fit), and X lies
              within x_bound() -- one float32 ulp plus the float64 solve's own error -- of the float64 solution of the same equation
              over the points of the RETURNED mask, whose condition number is asserted to be below 1e6 first.
  selection   gross outliers never survive; duplicated points split at the threshold in favour of the lower index; a NaN residual is
              never selected; degenerate sets are refused with X and the mask untouched; repeated calls give the same bits.
  golden      the kernel's X is no farther from the float64 evaluation of the reference's equation than the reference's own float32 X.
  field       bit-identical to the restatement, for both layouts, both element types, strided views, with and without u.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "affine_lts.npz")
DEV = "cuda"
SENTINEL = 0xA5
FIT_N = (8, 9, 63, 64, 65, 1023, 1024, 1025, 2049, 70001)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _affine
    return _affine.lib()


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)            # (a copy: the shared inputs are read-only)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def abi_fit(L, f, m, iters, normal, want_mask=True):
    """-> (return code, X (4, 4) float32 numpy, mask (n,) uint8 numpy or None); X and the mask start as SENTINEL bytes"""
    f, m = dev(f), dev(m)
    n = f.shape[0]
    X = torch.full((64,), SENTINEL, dtype=torch.uint8, device=DEV)
    mask = torch.full((n,), SENTINEL, dtype=torch.uint8, device=DEV) if want_mask else None
    nws = L.cvx_affine_lts_workspace_bytes(n)
    ws = torch.full((nws,), 0x5A, dtype=torch.uint8, device=DEV)            # a stale workspace
    rc = L.cvx_affine_lts_f32(p(f), f.shape[1], p(m), m.shape[1], n, iters, normal, p(X), p(mask), p(ws), nws, stream())
    torch.cuda.synchronize()
    return rc, X.cpu().numpy().view(np.float32).reshape(4, 4), (mask.cpu().numpy() if want_mask else None)


def check_solution(X, f, m, mask, normal):
    want, cond = R.fit64(f[mask], m[mask], normal)
    assert cond < 1e6, "the system of the returned set is badly conditioned (%g): the inputs of this case are badly chosen" % cond
    err = np.abs(X.astype(np.float64) - want)
    assert (err <= R.x_bound(want, cond)).all(), (err.max(), cond)
    if not normal:
        assert same_bits(X[:, 3], np.array([0, 0, 0, 1], np.float32))


# ---- fit: sizes, leading dimensions, iteration counts, both equations -----------------------------------------------------------------
@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("iters", [1, 2, 15])
@pytest.mark.parametrize("ld", [3, 4, 7])
@pytest.mark.parametrize("n", FIT_N)
def test_fit_is_the_float64_solution_on_the_returned_set(L, n, ld, iters, normal):
    f, m, _ = R.points(n, ld=ld)
    rc, X, mask = abi_fit(L, f, m, iters, normal)
    if ld == 3 and (iters > 1 or normal):
        assert rc == -1 and b"ld" in L.cvx_last_error()                    # three columns: a single least-squares fit only
        assert (X.view(np.uint8) == SENTINEL).all() and (mask == SENTINEL).all()
        return
    assert rc == 0, L.cvx_last_error()
    assert set(np.unique(mask)) <= {0, 1} and int(mask.sum()) == (n if iters == 1 else n // 2)
    check_solution(X, f, m, mask.astype(bool), normal)


@pytest.mark.parametrize("normal", [0, 1])
def test_gross_outliers_never_survive(L, normal):
    f, m, good = R.points(2049, seed=1, noise=0.0, outliers=0.4)
    rc, X, mask = abi_fit(L, f, m, 15, normal)
    assert rc == 0 and int(mask.sum()) == 1024
    assert good[mask.astype(bool)].all(), "%d outliers among the returned inliers" % int((~good[mask.astype(bool)]).sum())
    check_solution(X, f, m, mask.astype(bool), normal)
    assert np.abs(X - R.X_TRUE).max() <= 1e-5                               # exact inliers: the true map up to float32 rounding of the points


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("half", [33, 1025])
def test_ties_at_the_threshold_go_to_the_lowest_index(L, half, normal):
    """n = 2 m with m odd and point m + i a copy of point i: equal residuals in pairs, n // 2 = m is odd, so exactly one pair is split --
    and it must keep its lower index.  No residual arithmetic is restated."""
    f, m, _ = R.points(half, seed=2, noise=5e-2)
    f, m = np.r_[f, f], np.r_[m, m]
    rc, X, mask = abi_fit(L, f, m, 2, normal)
    assert rc == 0 and int(mask.sum()) == half
    lo, hi = mask[:half], mask[half:]
    assert (lo >= hi).all() and int((lo != hi).sum()) == 1


@pytest.mark.parametrize("iters", [2, 15])
def test_a_nan_row_is_never_selected(L, iters):
    """NaN in column 3 of three moving rows: the least-squares fit never reads that column, the residual does and sorts last"""
    f, m, _ = R.points(1025, seed=3)
    m = np.array(m)
    rows = [0, 511, 1024]
    m[rows, 3] = np.nan
    rc, X, mask = abi_fit(L, f, m, iters, 0)
    assert rc == 0 and int(mask.sum()) == 512 and not mask[rows].any()
    check_solution(X, f, m, mask.astype(bool), 0)


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("case", ["plane", "nan"])
def test_degenerate_sets_are_refused_and_nothing_is_written(L, case, normal):
    from convexadam_amd._lib import CvxError
    from convexadam_amd.affine import least_trimmed_affine, least_trimmed_squares
    if case == "plane":                                                     # z = 0 at integer coordinates: an exact zero pivot
        g = np.random.default_rng(4)
        f = np.c_[g.integers(-9, 10, (64, 2)), np.zeros(64), np.ones(64)].astype(np.float32)
        m = np.c_[f[:, :2] + g.integers(-1, 2, (64, 2)), np.zeros(64), np.ones(64)].astype(np.float32)
        word = b"singular"
    else:
        f, m, _ = R.points(65, seed=5)
        f = np.array(f)
        f[5, 0] = np.nan
        word = b"non-finite"
    rc, X, mask = abi_fit(L, f, m, 3, normal)
    assert rc == -1 and word in L.cvx_last_error(), (rc, L.cvx_last_error())
    assert (X.view(np.uint8) == SENTINEL).all() and (mask == SENTINEL).all()
    with pytest.raises(CvxError):
        (least_trimmed_squares if normal else least_trimmed_affine)(dev(f), dev(m), 3)


def test_repeated_calls_are_bit_identical(L):
    f, m, _ = R.points(70001, seed=6, outliers=0.3)
    for normal in (0, 1):
        a = abi_fit(L, f, m, 15, normal)
        b = abi_fit(L, f, m, 15, normal)
        assert a[0] == b[0] == 0 and same_bits(a[1], b[1]) and same_bits(a[2], b[2])


def test_python_orientations(L):
    from convexadam_amd.affine import find_affine_3d, least_trimmed_affine, least_trimmed_squares
    f, m, _ = R.points(1023, seed=7, outliers=0.2)
    X0 = abi_fit(L, f, m, 5, 0)
    T, inl = least_trimmed_affine(dev(f), dev(m), 5, return_inliers=True)
    assert T.dtype == torch.float32 and T.is_cuda and inl.dtype == torch.bool
    assert same_bits(T.cpu().numpy(), X0[1].T) and same_bits(inl.cpu().numpy(), X0[2].astype(bool))
    assert same_bits(least_trimmed_affine(dev(f), dev(m), 5).cpu().numpy(), X0[1].T)
    assert same_bits(least_trimmed_squares(dev(f), dev(m), 5).cpu().numpy(), abi_fit(L, f, m, 5, 1)[1])      # X, not transposed
    T3 = find_affine_3d(dev(f[:, :3]), dev(m[:, :3])).cpu().numpy()
    assert same_bits(T3, find_affine_3d(dev(f), dev(m)).cpu().numpy()) and same_bits(T3, abi_fit(L, f[:, :3], m[:, :3], 1, 0)[1].T)
    want, cond = R.fit64(f, m, 0)
    assert (np.abs(T3.T - want) <= R.x_bound(want, cond)).all()              # moving_i^T ~ T fixed_i^T
    for bad in (lambda: least_trimmed_affine(dev(f[:, :3]), dev(m[:, :3])), lambda: least_trimmed_affine(dev(f[:7]), dev(m[:7])),
                lambda: least_trimmed_affine(dev(f), dev(m[:-1])), lambda: least_trimmed_squares(dev(f), dev(m), 0),
                lambda: find_affine_3d(dev(f[:3]), dev(m[:3]))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        least_trimmed_affine(torch.from_numpy(np.array(f)), torch.from_numpy(np.array(m)))


def test_against_reference_golden(L):
    from convexadam_amd.affine import least_trimmed_squares
    z = np.load(GOLDEN)
    seen = 0
    for key in sorted(k for k in z.files if "_ref" in k):
        tag, k = key.split("_ref")
        f, m, ref, f64 = z[tag + "_fixed"], z[tag + "_moving"], z[key], z["%s_f64_%s" % (tag, k)]
        X = least_trimmed_squares(dev(f), dev(m), int(k)).cpu().numpy()
        mine, theirs = np.abs(X - f64).max(), np.abs(ref - f64).max()
        print("golden %s iter %s: kernel %.3g, reference float32 %.3g from the float64 evaluation" % (tag, k, mine, theirs))
        assert mine <= theirs, (tag, k, mine, theirs)
        seen += 1
    assert seen == 4


# ---- field ----------------------------------------------------------------------------------------------------------------------------
def abi_field(L, theta, shape, u, u_view, out_buf, out_view_strides, o64):
    """u: None or (tensor, f64, cs, vs); out_buf: the allocation, out_view_strides: (offset elements, cs, vs)"""
    th = dev(np.asarray(theta, np.float32).reshape(-1, 4)[:3])
    off, ocs, ovs = out_view_strides
    item = 8 if o64 else 4
    ua = (p(u_view[0]), u_view[1], u_view[2], u_view[3]) if u is not None else (None, 0, 0, 0)
    rc = L.cvx_affine_field_f64(p(th), *shape, *ua, C.c_void_p(out_buf.data_ptr() + off * item), o64, ocs, ovs, stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("with_u", [False, True])
@pytest.mark.parametrize("planar", [0, 1])
@pytest.mark.parametrize("shape", R.FIELD_SHAPES, ids=["x".join(map(str, s)) for s in R.FIELD_SHAPES])
def test_field_is_bit_identical_to_the_restatement(L, shape, planar, with_u):
    V = int(np.prod(shape))
    for u64 in ((0, 1) if with_u else (0,)):
        u = R.smooth_field(shape).astype(np.float64 if u64 else np.float32) if with_u else None
        for o64 in (1, 0):
            want = R.field(R.THETA, shape, u).astype(np.float64 if o64 else np.float32)
            ut = dev(R.layouts(u, u.dtype, planar)) if with_u else None
            out = torch.full((3 * V,), float("nan"), dtype=torch.float64 if o64 else torch.float32, device=DEV)
            # input in one layout, output in the other
            rc = abi_field(L, R.THETA, shape, u, (ut, u64) + ((V, 1) if planar else (1, 3)), out, (0,) + ((1, 3) if planar else (V, 1)), o64)
            assert rc == 0, L.cvx_last_error()
            got = out.cpu().numpy().reshape(shape + (3,)) if planar else np.moveaxis(out.cpu().numpy().reshape((3,) + shape), 0, -1)
            assert same_bits(got, want), (shape, planar, with_u, u64, o64)


def test_field_without_u_ignores_its_element_flag(L):
    """u = NULL with u_f64 = 1, the one pairing of flags the cases above leave out: no displacement is read, whatever the flag says.  A
    (5, 4, 7) grid: three distinct extents, one partial block"""
    shape = (5, 4, 7)
    V = int(np.prod(shape))
    th = dev(R.THETA)
    for o64 in (1, 0):
        want = R.field(R.THETA, shape, None).astype(np.float64 if o64 else np.float32)
        for planar in (0, 1):
            out = torch.full((3 * V,), float("nan"), dtype=torch.float64 if o64 else torch.float32, device=DEV)
            rc = L.cvx_affine_field_f64(p(th), *shape, None, 1, 0, 0, p(out), o64, *((V, 1) if planar else (1, 3)), stream())
            torch.cuda.synchronize()
            assert rc == 0, L.cvx_last_error()
            got = np.moveaxis(out.cpu().numpy().reshape((3,) + shape), 0, -1) if planar else out.cpu().numpy().reshape(shape + (3,))
            assert same_bits(got, want), (o64, planar)


def test_field_on_non_contiguous_views(L):
    """u is the [..., 1:4] part of an (H, W, D, 5) tensor, out the [..., :3] part of an (H, W, D, 4) one: voxel strides 5 and 4; what lies
    between the components' columns is never read (NaN) and never written (a sentinel)"""
    shape = (7, 1, 9)
    V = int(np.prod(shape))
    u = R.smooth_field(shape)
    big = np.full(shape + (5,), np.nan)
    big[..., 1:4] = u
    bt = dev(big)
    out = torch.full(shape + (4,), -77.0, dtype=torch.float64, device=DEV)
    th = dev(R.THETA)
    rc = L.cvx_affine_field_f64(p(th), *shape, C.c_void_p(bt.data_ptr() + 8), 1, 1, 5, p(out), 1, 1, 4, stream())
    torch.cuda.synchronize()
    assert rc == 0, L.cvx_last_error()
    o = out.cpu().numpy()
    assert same_bits(o[..., :3], R.field(R.THETA, shape, u)) and (o[..., 3] == -77.0).all()
    # planar with padded planes: component stride V + 3
    pl = torch.full((3, V + 3), -77.0, dtype=torch.float32, device=DEV)
    rc = L.cvx_affine_field_f64(p(th), *shape, C.c_void_p(bt.data_ptr() + 8), 1, 1, 5, p(pl), 0, V + 3, 1, stream())
    torch.cuda.synchronize()
    assert rc == 0, L.cvx_last_error()
    o = pl.cpu().numpy()
    assert same_bits(np.moveaxis(o[:, :V].reshape((3,) + shape), 0, -1), R.field(R.THETA, shape, u).astype(np.float32)) and (o[:, V:] == -77.0).all()


def test_a_non_finite_displacement_stays_in_its_voxel(L):
    from convexadam_amd.affine import affine_to_field
    shape = (33, 17, 65)
    u = np.array(R.smooth_field(shape))
    u[1, 2, 3, 0], u[32, 16, 64, 2], u[20, 0, 5, 1] = np.nan, np.inf, -np.inf
    got = affine_to_field(dev(R.THETA), shape, field=dev(u)).cpu().numpy()
    want, clean = R.field(R.THETA, shape, u), R.field(R.THETA, shape, R.smooth_field(shape))
    bad = ~np.isfinite(got).all(-1)
    assert int(bad.sum()) == 3 and bad[1, 2, 3] and bad[32, 16, 64] and bad[20, 0, 5]
    assert same_bits(got[~bad], clean[~bad])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and same_bits(np.nan_to_num(got, nan=7.0), np.nan_to_num(want, nan=7.0))


def test_affine_to_field_layouts_and_inputs():
    from convexadam_amd.affine import affine_to_field
    shape = (7, 1, 9)
    u = R.smooth_field(shape)
    T = np.eye(4, dtype=np.float32)
    T[:3] = R.THETA
    want = R.field(R.THETA, shape, u)
    pure = affine_to_field(dev(T), shape)
    assert pure.is_cuda and pure.dtype == torch.float64 and tuple(pure.shape) == shape + (3,)
    assert same_bits(pure.cpu().numpy(), R.field(R.THETA, shape))
    for th in (dev(T), dev(R.THETA), dev(R.THETA[None])):
        assert same_bits(affine_to_field(th, shape, field=u).cpu().numpy(), want)                            # a numpy field goes up
    a = affine_to_field(dev(T), shape, field=dev(u))
    b = affine_to_field(dev(T), shape, field=dev(R.layouts(u, np.float64, 1)))
    assert tuple(b.shape) == (3,) + shape and same_bits(a.cpu().numpy(), want) and same_bits(b.permute(1, 2, 3, 0).contiguous().cpu().numpy(), want)
    u32 = u.astype(np.float32)
    c = affine_to_field(dev(T), shape, field=dev(u32))
    assert c.dtype == torch.float64 and same_bits(c.cpu().numpy(), R.field(R.THETA, shape, u32))
    # the identity gives u back within the bound computed from the extent
    ident = affine_to_field(torch.eye(4, device=DEV), shape, field=dev(u)).cpu().numpy()
    assert np.abs(ident - u).max() <= R.identity_bound(shape)
    for bad in (lambda: affine_to_field(dev(T[:2]), shape), lambda: affine_to_field(dev(T), (7, 0, 9)),
                lambda: affine_to_field(dev(T), (7, 2, 9), field=dev(u))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        affine_to_field(torch.eye(4), shape)
