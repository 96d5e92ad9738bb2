"""Thin-plate-spline densification on the GPU (csrc/tps.hip, convexadam_amd/tps.py) against float64 restatements of the reference's
expressions (l2r_2021_convexAdam_task1_docker.py:198-262,365-387).

Criteria (u = 2^-24, gamma_k = k u / (1 - k u)):
  evaluation  per output |HIP - f64| <= gamma_{n+8} * S + 16 u * sum_j |w_j| (|U_j| + r_j^2), S = |a0| + |a1 x| + |a2 y| + |a3 z| +
              sum_j |w_j U_j|: the order-free bound of the sum, plus the error of forming each term in float32 -- r^2 from rounded
              differences (<= 3 u relative), sqrtf / logf (<= 1 ulp each; an absolute log error of ~ u reaches r^2 through r^2 log(.)).
  fit         normwise backward error ||A theta - v||_inf / (||A||_inf ||theta||_inf) <= 4 (n + 4) u, A and v the float64 system;
              values (at the centres, on a lattice) no further from the float64 spline than 4x those of the reference's own float32
              arithmetic (CPU torch float32 assembly + torch.linalg.solve + evaluation) plus an absolute floor of 1e-5 max|f|.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tps.npz")
U32 = 2.0 ** -24
DEV = "cuda"


def gamma(k):
    return k * U32 / (1 - k * U32)


# ---- float64 restatement (the reference's expressions) -------------------------------------------------------------------------------
def d64(a, b):
    ra = (a ** 2).sum(1)[:, None]
    rb = (b ** 2).sum(1)[None, :]
    return np.sqrt(np.maximum(ra + rb - 2.0 * a @ b.T, 0.0))


def u64(r):
    return r ** 2 * np.log(r + 1e-6)


def system64(c, f, lambd):
    c, f = np.asarray(c, np.float64), np.asarray(f, np.float64)
    n = c.shape[0]
    A = np.zeros((n + 4, n + 4))
    A[:n, :n] = u64(d64(c, c)) + lambd * np.eye(n)
    P = np.concatenate([np.ones((n, 1)), c], 1)
    A[:n, n:] = P
    A[n:, :n] = P.T
    v = np.zeros((n + 4, f.shape[1]))
    v[:n] = f
    return A, v


def fit64(c, f, lambd):
    A, v = system64(c, f, lambd)
    return np.linalg.solve(A, v)


def z64(x, c, theta, chunk=4096):
    x, c, theta = np.asarray(x, np.float64), np.asarray(c, np.float64), np.asarray(theta, np.float64)
    w, a = theta[:-4], theta[-4:]
    out = np.empty((x.shape[0], theta.shape[1]))
    for i in range(0, x.shape[0], chunk):
        xs = x[i:i + chunk]
        out[i:i + chunk] = a[0] + xs[:, :1] * a[1] + xs[:, 1:2] * a[2] + xs[:, 2:3] * a[3] + u64(d64(xs, c)) @ w
    return out


def eval_bound(x, c, theta):
    x, c, theta = np.asarray(x, np.float64), np.asarray(c, np.float64), np.asarray(theta, np.float64)
    n = c.shape[0]
    w, a = np.abs(theta[:-4]), np.abs(theta[-4:])
    r = d64(x, c)
    U = np.abs(u64(r))
    S = a[0] + np.abs(x[:, :1]) * a[1] + np.abs(x[:, 1:2]) * a[2] + np.abs(x[:, 2:3]) * a[3] + U @ w
    return gamma(n + 8) * S + 16 * U32 * ((U + r ** 2) @ w)


# ---- the reference's own float32 arithmetic on CPU (the yardstick of the fit criterion) -------------------------------------------
def fit32(c, f, lambd):
    c, f = torch.as_tensor(c, dtype=torch.float32), torch.as_tensor(f, dtype=torch.float32)
    n = c.shape[0]
    ra = (c ** 2).sum(1).view(-1, 1)
    dist = (ra + ra.view(1, -1) - 2.0 * c @ c.t()).clamp(0.0)
    r = torch.sqrt(dist)
    A = torch.zeros(n + 4, n + 4)
    A[:n, :n] = r ** 2 * torch.log(r + 1e-6) + lambd * torch.eye(n)
    P = torch.ones(n, 4)
    P[:, 1:] = c
    A[:n, n:] = P
    A[n:, :n] = P.t()
    v = torch.zeros(n + 4, f.shape[1])
    v[:n] = f
    return torch.linalg.solve(A, v)


def z32(x, c, theta):
    x, c = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(c, dtype=torch.float32)
    ra, rb = (x ** 2).sum(1).view(-1, 1), (c ** 2).sum(1).view(1, -1)
    r = torch.sqrt((ra + rb - 2.0 * x @ c.t()).clamp(0.0))
    w, a = theta[:-4], theta[-4:].unsqueeze(2)
    b = (r ** 2 * torch.log(r + 1e-6)) @ w
    return (a[0] + a[1] * x[:, 0] + a[2] * x[:, 1] + a[3] * x[:, 2] + b.t()).t()


def lattice(size):
    return F.affine_grid(torch.eye(3, 4).unsqueeze(0), (1, 1) + tuple(size), align_corners=True).view(-1, 3)


def masked_centres(n, seed, size=(32, 32, 32)):
    """task1-like centres: a random subset of the masked align_corners=True lattice in [-1, 1]^3."""
    g = torch.Generator().manual_seed(seed)
    pts = lattice(size)
    pts = pts[(pts ** 2).sum(1) < 0.9]
    return pts[torch.randperm(pts.shape[0], generator=g)[:n]].contiguous()


def smooth_values(c, seed, k=3):
    """(n, k) smooth values plus noise (k = 3 draws what it always drew)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(k, 3, generator=g) * 3 + 1
    f = torch.stack([sum(0.02 * torch.sin(a[j, i] * c[:, i] + j) for i in range(3)) for j in range(k)], 1)
    return (f + 0.002 * torch.randn(c.shape[0], k, generator=g)).contiguous()


def assert_no_worse(hip, ref32, exact, fmax, what):
    e_hip = float(np.abs(np.asarray(hip, np.float64) - exact).max())
    e_ref = float(np.abs(np.asarray(ref32, np.float64) - exact).max())
    floor = 1e-5 * fmax
    assert e_hip <= 4 * e_ref + floor, "%s: HIP error %.3g > 4 x float32-reference error %.3g + floor %.3g" % (what, e_hip, e_ref, floor)


# ---- 1. evaluation against a fixed theta -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 64, 1000, 4096])
def test_eval_fixed_theta(n):
    from convexadam_amd.convex_adam_utils import TPS
    g = torch.Generator().manual_seed(n)
    c = torch.rand(n, 3, generator=g) * 2 - 1
    x = torch.rand(3000, 3, generator=g) * 2.2 - 1.1
    x[:5] = c[:5] if n >= 5 else x[:5]                      # points on centres (r = 0) too
    theta = torch.randn(n + 4, 3, generator=g) * 0.1
    out = TPS.z(x.to(DEV), c.to(DEV), theta.to(DEV)).cpu().numpy()
    assert out.shape == (3000, 3)
    err = np.abs(out - z64(x.numpy(), c.numpy(), theta.numpy()))
    bound = eval_bound(x.numpy(), c.numpy(), theta.numpy())
    assert np.all(err <= bound), "max err/bound %.3g" % float((err / bound).max())


@pytest.mark.parametrize("size", [(37 // 3, 41 // 3, 29 // 3), (1, 6, 5), (4, 1, 7), (3, 5, 1), (1, 1, 1)])
def test_dense_lattice_matches_restatement(size):
    from convexadam_amd.tps import tps_dense
    n = 300
    g = torch.Generator().manual_seed(7)
    c = torch.rand(n, 3, generator=g) * 2 - 1
    theta = torch.randn(n + 4, 3, generator=g) * 0.1
    out = tps_dense(c.to(DEV), theta.to(DEV), size).cpu().numpy()
    assert out.shape == (3,) + tuple(size)
    x = lattice(size).numpy()                               # torch's float32 lattice: the kernel generates the same points
    err = np.abs(out.reshape(3, -1).T - z64(x, c.numpy(), theta.numpy()))
    assert np.all(err <= eval_bound(x, c.numpy(), theta.numpy()))


# ---- 2. fit ----------------------------------------------------------------------------------------------------------------------
def backward_error_ok(c, f, lambd, theta):
    """theta finite and the normwise backward error on the float64 system <= 4 (n+4) u; returns theta as float64."""
    n = c.shape[0]
    th = theta.cpu().numpy().astype(np.float64)
    assert np.isfinite(th).all()
    A, v = system64(c.numpy(), f.numpy(), lambd)
    be = np.abs(A @ th - v).max() / (np.abs(A).sum(1).max() * np.abs(th).max())
    assert be <= 4 * (n + 4) * U32, "backward error %.3g > %.3g" % (be, 4 * (n + 4) * U32)
    return th


def check_fit(c, f, lambd):
    """The fit criteria of the header: backward error, values at the centres and on a lattice against the float32 reference."""
    from convexadam_amd.convex_adam_utils import TPS
    n = c.shape[0]
    theta = TPS.fit(c.to(DEV), f.to(DEV), lambd)
    assert theta.shape == (n + 4, f.shape[1])
    backward_error_ok(c, f, lambd, theta)
    t64 = fit64(c.numpy(), f.numpy(), lambd)
    t32 = fit32(c, f, lambd)
    fmax = float(np.abs(f.numpy()).max())
    assert_no_worse(TPS.z(c.to(DEV), c.to(DEV), theta).cpu().numpy(), z32(c, c, t32).numpy(), z64(c.numpy(), c.numpy(), t64), fmax,
                    "values at the centres")
    x = lattice((11, 12, 10))
    assert_no_worse(TPS.z(x.to(DEV), c.to(DEV), theta).cpu().numpy(), z32(x, c, t32).numpy(), z64(x.numpy(), c.numpy(), t64), fmax,
                    "values on a lattice")
    return theta


@pytest.mark.parametrize("lambd", [0.0, 0.1])
@pytest.mark.parametrize("n", [5, 17, 64, 300, 1000, 4096])
def test_fit_backward_error_and_values(n, lambd):
    c = masked_centres(n, seed=n)
    check_fit(c, smooth_values(c, seed=n + 1), lambd)


# ---- 3. known answer: an affine f is reproduced -------------------------------------------------------------------------------------
def test_affine_field_is_reproduced():
    from convexadam_amd.convex_adam_utils import thin_plate_dense
    c = masked_centres(500, seed=3)
    M = torch.tensor([[0.03, -0.01, 0.02], [0.01, 0.05, -0.02], [-0.04, 0.02, 0.01]])
    b = torch.tensor([0.01, -0.02, 0.03])
    f = c @ M + b
    shape = (37, 41, 29)
    out = thin_plate_dense(c.unsqueeze(0).to(DEV), f.unsqueeze(0).to(DEV), shape, 3)
    assert out.shape == (1,) + shape + (3,)
    exact = lattice(shape).double().numpy() @ M.double().numpy() + b.double().numpy()
    # the float32 reference on the same input (fit + evaluation on the coarse lattice + align_corners=True up-sampling)
    t32 = fit32(c, f, 0.0)
    s1 = tuple(s // 3 for s in shape)
    y2 = z32(lattice(s1), c, t32).view(1, *s1, 3).permute(0, 4, 1, 2, 3)
    ref32 = F.interpolate(y2, shape, mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1).reshape(-1, 3)
    assert_no_worse(out.reshape(-1, 3).cpu().numpy(), ref32.numpy(), exact, float(np.abs(f.numpy()).max()), "affine field")


# ---- 4. resize with align_corners=True ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [((5, 6, 7), (9, 11, 13)), ((40, 48, 56), (160, 192, 224)), ((12, 10, 14), (48, 40, 56)),
                                     ((9, 10, 7), (37, 41, 29)), ((1, 5, 1), (4, 1, 9)), ((7, 7, 7), (3, 2, 5)), ((13, 1, 6), (13, 8, 6)),
                                     ((3, 4, 5), (3, 4, 5)), ((2, 3, 4), (17, 19, 23)), ((30, 20, 10), (11, 31, 4))])
def test_resize_align_corners_bit_identical(src, dst):
    from convexadam_amd.tps import resize_trilinear_ac
    g = torch.Generator().manual_seed(sum(src) + sum(dst))
    x = torch.randn(1, 3, *src, generator=g)
    ref = F.interpolate(x, dst, mode="trilinear", align_corners=True)
    out = resize_trilinear_ac(x.to(DEV), dst).cpu()
    assert np.array_equal(out.numpy(), ref.numpy())


# ---- 5. the reference's own thin_plate_dense (golden) -------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["small", "large"])
def test_thin_plate_dense_against_reference_golden(tag):
    from convexadam_amd.convex_adam_utils import thin_plate_dense
    z = np.load(GOLDEN)
    x1, y1, shape, idx = z[tag + "_x1"], z[tag + "_y1"], tuple(int(s) for s in z[tag + "_shape"]), z[tag + "_idx"].astype(np.int64)
    out = thin_plate_dense(torch.from_numpy(x1).unsqueeze(0).to(DEV), torch.from_numpy(y1).unsqueeze(0).to(DEV), shape, 4, 0.)
    assert out.shape == (1,) + shape + (3,)
    hip = out[0].reshape(-1, 3)[torch.from_numpy(idx).to(DEV)].cpu().numpy()      # the golden holds the reference's output at these voxels
    # float64 restatement: the spline on the coarse lattice, up-sampled (align_corners=True) in float64
    s1 = tuple(s // 4 for s in shape)
    y2 = z64(lattice(s1).numpy(), x1, fit64(x1, y1, 0.0)).reshape(1, *s1, 3).transpose(0, 4, 1, 2, 3)
    exact = F.interpolate(torch.from_numpy(y2), shape, mode="trilinear", align_corners=True)[0].permute(1, 2, 3, 0).reshape(-1, 3)
    exact = exact[torch.from_numpy(idx)].numpy()
    assert_no_worse(hip, z[tag + "_dense"], exact, float(np.abs(y1).max()), "thin_plate_dense " + tag)


# ---- 6. tps_densify end to end --------------------------------------------------------------------------------------------------------
def _densify64(disp_hr, mask, n_points, seed, step=4):
    """task1:365-387 in float64 on CPU (the same randperm draw)."""
    _, _, H, W, D = disp_hr.shape
    ident = F.affine_grid(torch.eye(3, 4).unsqueeze(0), (1, 1, H // 3, W // 3, D // 3), align_corners=True)
    disp = (disp_hr.double().permute(0, 2, 3, 4, 1) / torch.tensor([H - 1, W - 1, D - 1]).double().view(1, 1, 1, 1, 3) * 2).flip(4)
    mask3 = mask[1::3, 1::3, 1::3][:ident.shape[1], :ident.shape[2], :ident.shape[3]]
    ident1 = ident.view(-1, 3)[mask3.reshape(-1) > 0, :]
    ident_mask = ident1[torch.randperm(int((mask3 > 0).sum()), generator=torch.Generator().manual_seed(seed))[:n_points]]
    sampled = F.grid_sample(disp.permute(0, 4, 1, 2, 3), ident_mask.double().view(1, -1, 1, 1, 3)).squeeze(3).squeeze(3).permute(0, 2, 1)
    s1 = (H // step, W // step, D // step)
    x1 = ident_mask.double().numpy()
    y2 = z64(lattice(s1).numpy(), x1, fit64(x1, sampled[0].numpy(), 0.0)).reshape(1, *s1, 3).transpose(0, 4, 1, 2, 3)
    dense = F.interpolate(torch.from_numpy(y2), (H, W, D), mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1)
    flow = dense.flip(4).permute(0, 4, 1, 2, 3) * torch.tensor([H - 1, W - 1, D - 1]).double().view(1, 3, 1, 1, 1) / 2
    for _ in range(3):
        flow = F.avg_pool3d(flow, 3, padding=1, stride=1)
    return flow, sampled.float(), ident_mask


def test_tps_densify_end_to_end_and_deterministic():
    from convexadam_amd.convex_adam_MIND import convex_adam_pt
    from convexadam_amd.convex_adam_utils import tps_densify
    from convexadam_amd.phantom import phantom
    shape = (48, 44, 52)
    fix = phantom(shape, 1, 10)
    mov = torch.roll(phantom(shape, 1, 11), (2, -1, 1), (0, 1, 2))
    out = convex_adam_pt(fix, mov, dtype=torch.float32, device=torch.device(DEV), grid_sp=4, disp_hw=3, selected_niter=20, grid_sp_adam=2)
    disp_hr = torch.from_numpy(np.ascontiguousarray(out)).float().permute(3, 0, 1, 2).unsqueeze(0).contiguous()
    mask = (fix > float(fix.median())).float()
    n_points, seed = 1024, 5
    a = tps_densify(disp_hr.to(DEV), mask, n_points=n_points, generator=torch.Generator().manual_seed(seed))
    b = tps_densify(disp_hr.to(DEV), mask, n_points=n_points, generator=torch.Generator().manual_seed(seed))
    assert a.shape == (1, 3) + shape
    assert torch.equal(a, b), "two calls differ"
    assert torch.isfinite(a).all()
    exact, sampled32, pts = _densify64(disp_hr, mask, n_points, seed)
    # the float32 reference chain: same points, float32 samples, float32 fit / evaluation / up-sampling / pooling
    H, W, D = shape
    s1 = (H // 4, W // 4, D // 4)
    y2 = z32(lattice(s1), pts, fit32(pts, sampled32[0], 0.0)).view(1, *s1, 3).permute(0, 4, 1, 2, 3)
    dense = F.interpolate(y2, shape, mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1)
    ref32 = dense.flip(4).permute(0, 4, 1, 2, 3) * torch.tensor([H - 1, W - 1, D - 1]).float().view(1, 3, 1, 1, 1) / 2
    for _ in range(3):
        ref32 = F.avg_pool3d(ref32, 3, padding=1, stride=1)
    assert_no_worse(a.cpu().numpy(), ref32.numpy(), exact.numpy(), float(exact.abs().max()), "tps_densify")


# ---- 7. error path ----------------------------------------------------------------------------------------------------------------
def test_duplicate_centres_raise_and_write_nothing():
    from convexadam_amd import _lib
    from convexadam_amd.convex_adam_utils import TPS
    c = masked_centres(40, seed=9)
    c[17] = c[3]
    f = smooth_values(c, seed=2)
    with pytest.raises(_lib.CvxError, match="singular system"):
        TPS.fit(c.to(DEV), f.to(DEV), 0.0)
    # through the ABI: theta keeps what it held
    cd, fd = c.to(DEV), f.to(DEV)
    theta = torch.zeros(44, 3, device=DEV)
    nws = _lib.lib().cvx_tps_fit_workspace_bytes(40, 3)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    rc = _lib.lib().cvx_tps_fit_f32(_lib.ptr(cd), _lib.ptr(fd), 40, 3, 0.0, _lib.ptr(theta), _lib.ptr(ws), nws, _lib.stream_ptr())
    assert rc == _lib.CVX_ERR_INVALID_ARG and b"singular" in _lib.lib().cvx_last_error()
    assert torch.equal(theta, torch.zeros_like(theta))
    # lambda > 0 makes the same centres solvable, and the device is fine for the next call
    theta = TPS.fit(cd, fd, 0.1)
    assert torch.isfinite(theta).all()
    torch.cuda.synchronize()


# ---- 8. exact invariants (the build has no contraction and no atomics in the arithmetic: these hold bit for bit) -----------------
F_DIMS = [1, 2, 3, 4, 5, 8]           # every k_tps_eval<NR> instantiation, and the groups of 4 plus a remainder of tps._columns


@pytest.mark.parametrize("n", [70, 125])  # N = 74: three panels, a GEMM, two back-substitution blocks; N = 129: a last block of 1 row
def test_fit_columns_are_independent(n):
    """The pivots depend only on the matrix columns, and every right-hand side goes through the same swaps, triangular solve, GEMM
    element and back substitution in the same order, whatever its neighbours."""
    from convexadam_amd.convex_adam_utils import TPS
    c = masked_centres(n, seed=21).to(DEV)
    f = smooth_values(c.cpu(), seed=22, k=max(F_DIMS)).to(DEV)
    single = [TPS.fit(c, f[:, k:k + 1]) for k in range(f.shape[1])]
    for fd in F_DIMS:
        theta = TPS.fit(c, f[:, :fd])
        assert theta.shape == (n + 4, fd)
        for k in range(fd):
            assert torch.equal(theta[:, k], single[k][:, 0]), "f_dim %d, column %d" % (fd, k)


def test_nan_in_one_value_column_poisons_only_that_column():
    from convexadam_amd.convex_adam_utils import TPS
    c = masked_centres(100, seed=23).to(DEV)
    f = smooth_values(c.cpu(), seed=24, k=5).to(DEV)
    clean = TPS.fit(c, f)
    f[37, 1] = float("nan")
    theta = TPS.fit(c, f)                                    # the pivots never look at the right-hand sides: no error
    assert torch.isnan(theta[:, 1]).all()
    for k in (0, 2, 3, 4):
        assert torch.equal(theta[:, k], clean[:, k]), "column %d" % k


def test_eval_columns_are_independent_and_bounded():
    from convexadam_amd.convex_adam_utils import TPS
    n, m = 300, 1500
    g = torch.Generator().manual_seed(25)
    c = torch.rand(n, 3, generator=g) * 2 - 1
    x = torch.rand(m, 3, generator=g) * 2.2 - 1.1
    x[:5] = c[:5]
    theta = torch.randn(n + 4, max(F_DIMS), generator=g) * 0.1
    xd, cd, td = x.to(DEV), c.to(DEV), theta.to(DEV)
    single = [TPS.z(xd, cd, td[:, k:k + 1]) for k in range(theta.shape[1])]
    for fd in F_DIMS:
        out = TPS.z(xd, cd, td[:, :fd])
        assert out.shape == (m, fd)
        for k in range(fd):
            assert torch.equal(out[:, k], single[k][:, 0]), "f_dim %d, column %d" % (fd, k)
        err = np.abs(out.cpu().numpy() - z64(x.numpy(), c.numpy(), theta[:, :fd].numpy()))
        assert np.all(err <= eval_bound(x.numpy(), c.numpy(), theta[:, :fd].numpy())), "f_dim %d" % fd


@pytest.mark.parametrize("size", [(40, 48, 56), (37, 41, 29), (2, 3, 2), (1, 6, 5), (5, 1, 1), (1, 1, 1)])
def test_dense_lattice_is_the_evaluated_lattice(size):
    """tps_dense generates torch's float32 affine_grid lattice in the kernel: every bit of it, so the same spline values."""
    from convexadam_amd.convex_adam_utils import TPS
    from convexadam_amd.tps import tps_dense
    n, fd = 300, 5
    g = torch.Generator().manual_seed(26)
    c = (torch.rand(n, 3, generator=g) * 2 - 1).to(DEV)
    theta = (torch.randn(n + 4, fd, generator=g) * 0.1).to(DEV)
    out = tps_dense(c, theta, size)
    assert out.shape == (fd,) + size
    ref = TPS.z(lattice(size).to(DEV), c, theta)
    assert torch.equal(out, ref.t().reshape((fd,) + size))


def _abi_fit(c, f, lambd, theta, ws):
    from convexadam_amd import _lib
    L = _lib.lib()
    n, nr = int(c.shape[0]), int(f.shape[1])
    rc = L.cvx_tps_fit_f32(_lib.ptr(c), _lib.ptr(f), n, nr, float(lambd), _lib.ptr(theta), _lib.ptr(ws), int(ws.numel()), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, L.cvx_last_error()


def test_fit_is_deterministic_and_ignores_the_workspace_contents():
    from convexadam_amd import _lib
    n = 200
    c = masked_centres(n, seed=27).to(DEV)
    f = smooth_values(c.cpu(), seed=28).to(DEV)
    nws = _lib.lib().cvx_tps_fit_workspace_bytes(n, 3)

    def fit(ws):
        theta = torch.zeros(n + 4, 3, device=DEV)
        rc, msg = _abi_fit(c, f, 0.0, theta, ws)
        assert rc == _lib.CVX_OK, msg
        return theta

    a = fit(torch.zeros(nws, dtype=torch.uint8, device=DEV))
    assert torch.equal(a, fit(torch.zeros(nws, dtype=torch.uint8, device=DEV)))
    assert torch.equal(a, fit(torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)))
    # a fit that stops at a singular pivot leaves its workspace half factorised; the next fit in it does not see that
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    cz = c.clone()
    cz[:, 2] = 0.0
    rc, msg = _abi_fit(cz, f, 0.0, torch.zeros(n + 4, 3, device=DEV), ws)
    assert rc == _lib.CVX_ERR_INVALID_ARG and b"singular" in msg
    assert torch.equal(a, fit(ws))


# ---- 9. batched and wide resize -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [(2, 3), (3, 1), (2, 4)])
def test_resize_batched_bit_identical(nc):
    from convexadam_amd.tps import resize_trilinear_ac
    g = torch.Generator().manual_seed(30 + sum(nc))
    x = torch.randn(*nc, 5, 6, 7, generator=g)
    ref = F.interpolate(x, (9, 11, 13), mode="trilinear", align_corners=True)
    out = resize_trilinear_ac(x.to(DEV), (9, 11, 13)).cpu()
    assert out.shape == ref.shape
    assert np.array_equal(out.numpy(), ref.numpy())


@pytest.mark.parametrize("D", [257, 300])                    # D > 256: several x-blocks at the widest block size
@pytest.mark.parametrize("C", [1, 4, 7])
def test_resize_wide_rows_bit_identical(C, D):
    from convexadam_amd.tps import resize_trilinear_ac
    g = torch.Generator().manual_seed(C * D)
    x = torch.randn(1, C, 3, 4, 9, generator=g)
    ref = F.interpolate(x, (5, 6, D), mode="trilinear", align_corners=True)
    assert np.array_equal(resize_trilinear_ac(x.to(DEV), (5, 6, D)).cpu().numpy(), ref.numpy())


def test_resize_refuses_an_output_beyond_the_grid_limit():
    from convexadam_amd import _lib
    from convexadam_amd.tps import resize_trilinear_ac
    x = torch.rand(1, 1, 2, 2, 2, device=DEV)
    with pytest.raises(_lib.CvxError, match="grid limits"):
        resize_trilinear_ac(x, (65536, 1, 1))                 # refused on the host: a 256 KB output, nothing launched
    torch.cuda.synchronize()


# ---- 10. LU block edges and evaluation chunk edges against the float64 restatement -----------------------------------------------
NB = 32                               # panel width of the LU (csrc/tps.hip); the GEMM tiles are 64 x 64, the back substitution 64 rows
LU_EDGE_N = [27, 28, 29, 60, 61, 91, 124, 1020, 1021, 2045]     # N = n + 4 = 31, 32, 33, 64, 65, 95, 128, 1024, 1025, 2049
LU_EDGES = [(n, fd) for n in LU_EDGE_N for fd in (1, 4)] + [(29, 2), (61, 2)]


def _lu_launches(N, nrhs):
    """(nb, right, rows) of every panel step of cvx_tps_fit_f32: GEMM launched iff rows > 0, `right` columns wide."""
    ncol = N + nrhs
    return [(min(NB, N - k0), ncol - k0 - min(NB, N - k0), N - k0 - min(NB, N - k0)) for k0 in range(0, N, NB)]


def test_lu_edge_cases_sit_on_the_block_edges():
    Ns = {n + 4 for n, _ in LU_EDGES}
    for r in (0, 1):
        assert any(N % NB == r for N in Ns) and any(N % 64 == r for N in Ns)   # full / 1-column last panel, 64 / 1-row backsub block
    assert {1024, 1025} <= Ns                                                  # the 1024-thread panel loop wraps
    assert (27, 1) in LU_EDGES and (27 + 5) % NB == 0                        # ncol = N + nrhs at 0 and 1 mod 32
    assert (28, 1) in LU_EDGES and (28 + 5) % NB == 1
    steps = [s for n, fd in LU_EDGES for s in _lu_launches(n + 4, fd)]
    assert any(rows == 1 for _, _, rows in steps)                              # the 1-row trailing GEMM
    for r in (0, 1):                                                           # GEMM width on, and one past, its 64-column tile edge
        assert any(rows > 0 and right % 64 == r for _, right, rows in steps)


@pytest.mark.parametrize("lambd", [0.0, 0.1])
@pytest.mark.parametrize("n,fd", LU_EDGES)
def test_fit_lu_block_edges(n, fd, lambd):
    c = masked_centres(n, seed=100 + n)
    check_fit(c, smooth_values(c, seed=200 + n, k=fd), lambd)


EVAL_M = [1, 255, 256, 257, 511, 512, 513, 1025]


@pytest.mark.parametrize("fd", [1, 2, 4])
@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513])   # centres staged 256 at a time
def test_eval_chunk_edges(n, fd):
    """m at the edges of the 512-point blocks: the full evaluation is graded, every shorter prefix must equal its head bit for bit."""
    from convexadam_amd.convex_adam_utils import TPS
    g = torch.Generator().manual_seed(300 + n)
    c = torch.rand(n, 3, generator=g) * 2 - 1
    x = torch.rand(max(EVAL_M), 3, generator=g) * 2.2 - 1.1
    for i, j in ((0, 0), (255, 255), (256, n - 1), (511, 256), (512, n // 2), (1024, n - 256)):
        x[i] = c[j % n]                                        # points on centres (r = 0), at the block edges, from either chunk
    theta = torch.randn(n + 4, fd, generator=g) * 0.1
    xd, cd, td = x.to(DEV), c.to(DEV), theta.to(DEV)
    full = TPS.z(xd, cd, td)
    err = np.abs(full.cpu().numpy() - z64(x.numpy(), c.numpy(), theta.numpy()))
    assert np.all(err <= eval_bound(x.numpy(), c.numpy(), theta.numpy())), "max err/bound %.3g" % float(
        (err / eval_bound(x.numpy(), c.numpy(), theta.numpy())).max())
    for m in EVAL_M[:-1]:
        assert torch.equal(TPS.z(xd[:m], cd, td), full[:m]), "m = %d" % m


# ---- 11. ill-conditioned but regular, and the affine known answer for every lambda -------------------------------------------------
def test_fit_close_partner_centres():
    """lambda = 0, 500 masked centres, 100 with a partner at 1e-3 and 20 with one at 2e-5 (distinct in float32): a regular system
    with tiny pivots; the backward error keeps its bound."""
    from convexadam_amd.convex_adam_utils import TPS
    base = masked_centres(500, seed=31)
    g = torch.Generator().manual_seed(32)
    d = torch.randn(120, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    dist = torch.cat([torch.full((100, 1), 1e-3), torch.full((20, 1), 2e-5)])
    c = torch.cat([base, base[:120] + dist * d]).contiguous()
    assert (c[500:] != base[:120]).any(1).all()
    f = smooth_values(c, seed=33)
    backward_error_ok(c, f, 0.0, TPS.fit(c.to(DEV), f.to(DEV), 0.0))


@pytest.mark.parametrize("lambd", [0.0, 0.1, 10.0])
def test_affine_known_answer_every_lambda(lambd):
    """f = c M + b exactly (dyadic centres on the 33^3 lattice, M and b in 1/64ths): the solution is w = 0 and affine rows (b, M) for
    every lambda.  Values on a lattice, the weights and the affine rows are graded against the float32 reference."""
    from convexadam_amd.convex_adam_utils import TPS
    n = 500
    c = masked_centres(n, seed=34, size=(33, 33, 33))
    M = torch.tensor([[2.0, -1.0, 1.0], [1.0, 3.0, -1.0], [-3.0, 1.0, 1.0]]) / 64
    b = torch.tensor([1.0, -1.0, 2.0]) / 64
    f = (c @ M + b).contiguous()
    assert torch.equal(f.double(), c.double() @ M.double() + b.double())
    theta = TPS.fit(c.to(DEV), f.to(DEV), lambd)
    th = theta.cpu().numpy()
    t32 = fit32(c, f, lambd)
    fmax = float(np.abs(f.numpy()).max())
    x = lattice((11, 12, 10))
    exact = x.double().numpy() @ M.double().numpy() + b.double().numpy()
    assert_no_worse(TPS.z(x.to(DEV), c.to(DEV), theta).cpu().numpy(), z32(x, c, t32).numpy(), exact, fmax, "values on a lattice")
    assert_no_worse(th[:n], t32[:n].numpy(), 0.0, fmax, "weights")
    assert_no_worse(th[n:], t32[n:].numpy(), np.concatenate([b[None].double().numpy(), M.double().numpy()]), fmax, "affine rows")


# ---- 12. error paths: zero and non-finite pivots ---------------------------------------------------------------------------------
def _check_refused_then_recovers(c, f, lambd, what):
    """Through the ABI: the fit refuses with `what` in the message and leaves theta as it was; the next good fit in the same
    workspace gives what a fresh workspace gives."""
    from convexadam_amd import _lib
    n = int(c.shape[0])
    nws = _lib.lib().cvx_tps_fit_workspace_bytes(n, 3)
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    sentinel = torch.arange((n + 4) * 3, dtype=torch.float32, device=DEV).view(n + 4, 3)
    theta = sentinel.clone()
    rc, msg = _abi_fit(c.to(DEV), f.to(DEV), lambd, theta, ws)
    assert rc == _lib.CVX_ERR_INVALID_ARG and what in msg, msg
    assert torch.equal(theta, sentinel)
    good = masked_centres(n, seed=40).to(DEV)
    fg = smooth_values(good.cpu(), seed=41).to(DEV)
    fresh = torch.zeros(n + 4, 3, device=DEV)
    assert _abi_fit(good, fg, lambd, fresh, torch.zeros(nws, dtype=torch.uint8, device=DEV))[0] == _lib.CVX_OK
    theta = torch.zeros(n + 4, 3, device=DEV)
    assert _abi_fit(good, fg, lambd, theta, ws)[0] == _lib.CVX_OK
    assert torch.equal(theta, fresh)


@pytest.mark.parametrize("lambd", [0.0, 0.1])
def test_planar_centres_give_a_zero_pivot(lambd):
    """All centres at z = 0.0: row and column n+3 of the system are exactly zero through every update, so column n+3 has a zero pivot
    (not the coincident-centre path: the centres are distinct)."""
    from convexadam_amd import _lib
    from convexadam_amd.convex_adam_utils import TPS
    n = 60
    g = torch.Generator().manual_seed(42)
    c = torch.rand(n, 3, generator=g) * 2 - 1
    c[:, 2] = 0.0
    f = smooth_values(c, seed=43)
    with pytest.raises(_lib.CvxError, match="zero or non-finite pivot in column %d of %d" % (n + 3, n + 4)):
        TPS.fit(c.to(DEV), f.to(DEV), lambd)
    _check_refused_then_recovers(c, f, lambd, b"zero or non-finite pivot")


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_centre_gives_a_non_finite_pivot(bad):
    from convexadam_amd import _lib
    from convexadam_amd.convex_adam_utils import TPS
    n = 60
    c = masked_centres(n, seed=44)
    f = smooth_values(c, seed=45)
    c[7, 1] = bad
    with pytest.raises(_lib.CvxError, match="zero or non-finite pivot"):
        TPS.fit(c.to(DEV), f.to(DEV), 0.0)
    _check_refused_then_recovers(c, f, 0.0, b"zero or non-finite pivot")
