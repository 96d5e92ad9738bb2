"""Least-trimmed rigid fit and fused affine warp on the GPU (csrc/rigid.hip, convexadam_amd/rigid.py) against float64 restatements of the
reference's expressions (convex_adam_utils.py:173-193, l2r_2020_convexAdam_CuRIOUS.py:349-390) and torch's CPU affine_grid / grid_sample.

Criteria:
  solver      T equals the float64 Kabsch fit (SVD, diag(1, 1, det(V U^T))) on exactly the returned point set within 2e-6; R is
              orthonormal to 1e-6 with det +1 (collinear points: the objective instead of R).
  selection   the n // 2 points chosen after fit k have float64 residuals (under the returned T_k) no larger than any unchosen one's plus
              a float32 allowance, and they are exactly the n // 2 smallest float32 residuals of the kernel's expression (emulated here bit
              for bit), ties to the lowest index.
  golden      max|T_hip - T_64| <= 4 max|T_ref32 - T_64| + 2e-6, T_64 the float64 restatement of the whole trimmed fit, T_ref32 the
              reference's own float32 result (tests/golden/rigid.npz).
  warp        bit-identical to torch's CPU F.grid_sample and the oracle's grid_sample on the affine_grid chain emulated here, to a numpy
              rint restatement (nearest), and to torch's CPU F.affine_grid + F.grid_sample wherever that host's affine_grid (a BLAS
              bmm) rounds like the chain -- it does on AVX2 hosts; an AVX-512 MKL path can differ in the last bit of a coordinate.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rigid.npz")
DEV = "cuda"
TAGS = ("clean", "outliers", "reflection", "planar", "field")


# ---- float64 restatements ------------------------------------------------------------------------------------------------------------
def kabsch64(x, y):
    x, y = np.asarray(x, np.float64)[:, :3], np.asarray(y, np.float64)[:, :3]
    xm, ym = x.mean(0), y.mean(0)
    u, _, vt = np.linalg.svd((x - xm).T @ (y - ym))
    v = vt.T
    m = np.eye(3)
    m[2, 2] = np.linalg.det(v @ u.T)
    R = v @ m @ u.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, ym - R @ xm
    return T


def resid64(T, f, m):
    f, m = np.asarray(f, np.float64), np.asarray(m, np.float64)
    return np.sqrt(((m - f @ np.asarray(T, np.float64).T) ** 2).sum(1))


def lts64(f, m, iters):
    idx = np.arange(f.shape[0])
    for _ in range(iters):
        T = kabsch64(f[idx], m[idx])
        idx = np.argsort(resid64(T, f, m), kind="stable")[:f.shape[0] // 2]
    return T


def fmaf(a, b, c):
    """float32 fused multiply-add, exactly: the product is exact in float64; a float64 sum that lands on a float32 midpoint is resolved
    with the exact error of that sum (TwoSum)."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    other = np.where(s > r64, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf)))
    mid = (r64 + other.astype(np.float64)) / 2
    fix = (s == mid) & (s != r64) & (((s > r64) & (err > 0)) | ((s < r64) & (err < 0)))
    return np.where(fix, other, r).astype(np.float32)


def resid32(T, f, m):
    """The kernel's float32 residual expression (rigid.hip::residual_bits), emulated bit for bit."""
    T, f, m = np.asarray(T, np.float32), np.asarray(f, np.float32), np.asarray(m, np.float32)
    s = np.zeros(f.shape[0], np.float32)
    for a in range(3):
        p = f[:, 0] * T[a, 0]
        for k in (1, 2, 3):
            p = fmaf(f[:, k], T[a, k], p)
        e = m[:, a] - p
        s = s + e * e
    e3 = m[:, 3] - f[:, 3]
    s = s + e3 * e3
    return np.sqrt(s)


def check_rotation(T):
    R = np.asarray(T, np.float64)[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6
    assert abs(np.linalg.det(R) - 1.0) <= 1e-6
    assert np.array_equal(np.asarray(T)[3], [0, 0, 0, 1])


def golden():
    return np.load(GOLDEN)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


# ---- solver ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("k", [1, 2, 5, 15])
def test_solver_is_the_float64_fit_on_the_returned_set(tag, k):
    from convexadam_amd.rigid import least_trimmed_rigid
    z = golden()
    f, m = z[tag + "_fixed"], z[tag + "_moving"]
    T, mask = least_trimmed_rigid(dev(f), dev(m), k, return_inliers=True)
    T, mask = T.cpu().numpy(), mask.cpu().numpy()
    assert T.dtype == np.float32 and mask.dtype == bool
    assert mask.sum() == (f.shape[0] if k == 1 else f.shape[0] // 2)
    assert np.abs(T - kabsch64(f[mask], m[mask])).max() <= 2e-6
    check_rotation(T)


@pytest.mark.parametrize("tag", TAGS)
def test_find_rigid_3d_on_three_and_four_columns(tag):
    from convexadam_amd.rigid import find_rigid_3d
    z = golden()
    f, m = z[tag + "_fixed"], z[tag + "_moving"]
    T4 = find_rigid_3d(dev(f), dev(m)).cpu().numpy()
    T3 = find_rigid_3d(dev(f[:, :3]), dev(m[:, :3])).cpu().numpy()
    assert np.array_equal(T3, T4)
    assert np.abs(T4 - kabsch64(f, m)).max() <= 2e-6
    check_rotation(T4)


def test_reflection_gives_a_proper_rotation():
    from convexadam_amd.rigid import find_rigid_3d
    g = np.random.default_rng(3)
    x = (g.normal(size=(500, 3)) * [0.5, 0.3, 0.1]).astype(np.float32)
    y = (x * [1, -1, 1]).astype(np.float32)                         # an exact mirror: no rotation fits it
    T = find_rigid_3d(dev(x), dev(y)).cpu().numpy()
    check_rotation(T)
    assert np.abs(T - kabsch64(x, y)).max() <= 2e-6


def test_collinear_points_reach_the_optimal_objective():
    from convexadam_amd.rigid import find_rigid_3d
    g = np.random.default_rng(4)
    x = (np.outer(g.normal(size=400), [0.3, -0.5, 0.8]) + [0.1, 0.2, 0.3]).astype(np.float32)
    y = (x[:, [1, 2, 0]] + 1e-3 * g.normal(size=(400, 3))).astype(np.float32)
    T = find_rigid_3d(dev(x), dev(y)).cpu().numpy()
    check_rotation(T)
    T64 = kabsch64(x, y)
    obj = lambda T_: float((resid64(T_, np.c_[x, np.ones(400)], np.c_[y, np.ones(400)]) ** 2).sum())  # noqa: E731
    assert obj(T) <= obj(T64) * (1 + 1e-5) + 1e-9


# ---- selection --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["outliers", "field", "planar"])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_selection_is_the_half_with_the_smallest_residuals(tag, k):
    from convexadam_amd.rigid import least_trimmed_rigid
    z = golden()
    f, m = z[tag + "_fixed"], z[tag + "_moving"]
    n = f.shape[0]
    Tk = least_trimmed_rigid(dev(f), dev(m), k).cpu().numpy()
    _, mask = least_trimmed_rigid(dev(f), dev(m), k + 1, return_inliers=True)
    mask = mask.cpu().numpy()
    assert mask.sum() == n // 2
    r64 = resid64(Tk, f, m)
    allow = 16 * 2.0 ** -24 * (np.abs(m).max() + 4 * np.abs(f).max() * np.abs(Tk).max())
    assert r64[mask].max() <= r64[~mask].min() + allow
    # prefix consistency: fit k of the (k + 1)-fit run is the k-fit result bit for bit, so its selection is exactly the n // 2 smallest
    # float32 residuals under T_k, ties to the lowest index
    expect = np.zeros(n, bool)
    expect[np.argsort(resid32(Tk, f, m), kind="stable")[:n // 2]] = True
    assert np.array_equal(mask, expect)


def test_ties_at_the_threshold_go_to_the_lowest_index():
    from convexadam_amd.rigid import least_trimmed_rigid
    g = np.random.default_rng(5)
    base = np.c_[g.normal(size=(5, 3)) * 0.5, np.ones(5)].astype(np.float32)
    moved = base.copy()
    moved[:, :3] += (g.normal(size=(5, 3)) * 0.05).astype(np.float32)
    n = 4000                                                        # five classes of 800 exact duplicates, n // 2 = 2000
    f, m = base[np.arange(n) % 5], moved[np.arange(n) % 5]
    T1 = least_trimmed_rigid(dev(f), dev(m), 1).cpu().numpy()
    r = resid32(T1, f, m)
    order = np.argsort(r[:5], kind="stable")
    assert np.diff(r[:5][order]).min() > 0                           # five distinct residual values
    _, mask = least_trimmed_rigid(dev(f), dev(m), 2, return_inliers=True)
    mask = mask.cpu().numpy()
    expect = np.zeros(n, bool)
    expect[np.argsort(r, kind="stable")[:n // 2]] = True           # classes order[0], order[1] whole, the first 400 of order[2]
    assert np.array_equal(mask, expect)
    assert mask[np.arange(n) % 5 == order[2]].sum() == 400
    assert mask[order[2]] and not mask[n - 5 + order[2]]


def test_repeated_calls_are_bit_identical():
    from convexadam_amd.rigid import least_trimmed_rigid
    z = golden()
    f, m = dev(z["outliers_fixed"]), dev(z["outliers_moving"])
    a, ma = least_trimmed_rigid(f, m, 15, return_inliers=True)
    b, mb = least_trimmed_rigid(f, m, 15, return_inliers=True)
    assert torch.equal(a, b) and torch.equal(ma, mb)


# ---- against the reference's own float32 result -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("k", ["find", 1, 2, 5, 15])
def test_against_reference_golden(tag, k):
    from convexadam_amd.rigid import find_rigid_3d, least_trimmed_rigid
    z = golden()
    f, m = z[tag + "_fixed"], z[tag + "_moving"]
    if k == "find":
        hip, ref, t64 = find_rigid_3d(dev(f), dev(m)), z[tag + "_find"], kabsch64(f, m)
    else:
        hip, ref, t64 = least_trimmed_rigid(dev(f), dev(m), k), z["%s_lts%d" % (tag, k)], lts64(f, m, k)
    err = np.abs(hip.cpu().numpy() - t64).max()
    assert err <= 4 * np.abs(ref - t64).max() + 2e-6, (err, np.abs(ref - t64).max())


def test_large_trimmed_fit_recovers_the_motion():
    from convexadam_amd.rigid import least_trimmed_rigid
    g = np.random.default_rng(6)
    n = 85000
    x = g.normal(size=(n, 3)) * [0.6, 0.4, 0.3]
    ang = np.deg2rad(5.0)
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    y = x @ R.T + [0.02, -0.01, 0.03] + 1e-4 * g.normal(size=(n, 3))
    bad = g.permutation(n)[:n // 4]
    y[bad] += g.normal(size=(bad.size, 3))
    f, m = np.c_[x, np.ones(n)].astype(np.float32), np.c_[y, np.ones(n)].astype(np.float32)
    T, mask = least_trimmed_rigid(dev(f), dev(m), 15, return_inliers=True)
    T, mask = T.cpu().numpy(), mask.cpu().numpy()
    assert np.abs(T[:3, :3] - R).max() <= 1e-4 and np.abs(T[:3, 3] - [0.02, -0.01, 0.03]).max() <= 1e-4
    assert np.abs(T - kabsch64(f[mask], m[mask])).max() <= 2e-6
    assert not mask[bad].any() or mask[bad].mean() < 0.01


# ---- warp -----------------------------------------------------------------------------------------------------------------------
def grid_fma(theta, size):
    from convexadam_amd.convex_adam_utils import affine_base
    ho, wo, do_ = size
    th = np.asarray(theta, np.float32)
    full = (ho, wo, do_)
    bx = np.broadcast_to(affine_base(do_)[None, None, :], full)
    by = np.broadcast_to(affine_base(wo)[None, :, None], full)
    bz = np.broadcast_to(affine_base(ho)[:, None, None], full)
    out = []
    for i in range(3):
        a = (bx * th[i, 0]).astype(np.float32)
        a = fmaf(by, th[i, 1], a)
        a = fmaf(bz, th[i, 2], a)
        out.append((a + th[i, 3]).astype(np.float32))
    return np.stack(out, -1)


def nearest64(vol, grid):
    """grid_sample nearest / zeros / align_corners=False restated: ATen's float32 unnormalisation, rint (half to even)."""
    C, h, w, d = vol.shape
    S = np.array([d, w, h], np.float32)
    ix = ((grid + np.float32(1)) * S - np.float32(1)) * np.float32(0.5)
    r = np.rint(ix)
    inb = (r >= 0).all(-1) & (r[..., 0] <= d - 1) & (r[..., 1] <= w - 1) & (r[..., 2] <= h - 1)
    rr = np.where(inb[..., None], r, 0).astype(np.int64)
    return np.where(inb[None], vol[:, rr[..., 2], rr[..., 1], rr[..., 0]], np.float32(0)).astype(np.float32)


def torch_warp(vol, theta, size, mode):
    C = vol.shape[0]
    grid = F.affine_grid(torch.as_tensor(np.asarray(theta, np.float32))[:3].unsqueeze(0), (1, C) + tuple(size), align_corners=False)
    return F.grid_sample(torch.as_tensor(vol).unsqueeze(0), grid, mode=mode, padding_mode="zeros", align_corners=False)[0].numpy()


def rot(g, deg, shift=(0.0, 0.0, 0.0)):
    axis = g.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.deg2rad(deg)
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    return np.c_[R, shift].astype(np.float32)


WARP_CASES = {
    "identity": (3, (20, 24, 28), None, lambda g: np.eye(3, 4, dtype=np.float32)),
    "rotation": (1, (30, 26, 34), None, lambda g: rot(g, 12.0, (0.05, -0.03, 0.02))),
    "rotation_c3": (3, (30, 26, 34), None, lambda g: rot(g, -20.0, (0.1, 0.0, -0.05))),
    "resized": (2, (24, 20, 28), (31, 17, 40), lambda g: rot(g, 7.0, (0.0, 0.02, 0.0))),
    "out_of_bounds": (1, (16, 18, 20), None, lambda g: rot(g, 30.0, (0.9, -0.7, 0.5))),
    "all_outside": (1, (16, 18, 20), None, lambda g: rot(g, 0.0, (3.0, 0.0, 0.0))),
    "ragged": (1, (37, 41, 43), None, lambda g: rot(g, 9.0, (0.01, 0.02, -0.03))),
    "ragged_c3": (3, (37, 41, 43), (43, 37, 41), lambda g: rot(g, 33.0, (-0.05, 0.02, 0.01))),
}


def torch_affine_grid_is_the_chain(theta, size):
    """torch's CPU affine_grid is a bmm: its rounding follows the host's BLAS kernel.  On an AVX2 host it equals the FMA chain the warp
    kernel computes bit for bit; on others it may differ in the last bit.  Returns (chain grid, whether torch's grid equals it)."""
    grid = grid_fma(theta, size)
    tg = F.affine_grid(torch.as_tensor(np.asarray(theta, np.float32))[:3].unsqueeze(0), (1, 1) + tuple(size), align_corners=False)[0].numpy()
    assert np.abs(grid - tg).max() <= 4 * 2.0 ** -24 * (np.abs(theta).sum(1).max() + 1)
    return grid, np.array_equal(grid, tg)


@pytest.mark.parametrize("case", sorted(WARP_CASES))
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_affine_warp_bit_identical(case, mode):
    from oracle import oracle
    from convexadam_amd.rigid import affine_warp
    C, shape, size, make = WARP_CASES[case]
    g = np.random.default_rng(sum(map(ord, case)))
    vol = g.normal(size=(C,) + shape).astype(np.float32)
    theta = make(g)
    out_size = size or shape
    hip = affine_warp(dev(vol), dev(theta), size=size, mode=mode).cpu().numpy()
    assert hip.shape == (C,) + tuple(out_size) and hip.dtype == np.float32
    grid, torch_grid_is_chain = torch_affine_grid_is_the_chain(theta, out_size)
    ref = F.grid_sample(torch.as_tensor(vol)[None], torch.as_tensor(grid)[None], mode=mode, align_corners=False)[0].numpy()
    assert np.array_equal(hip.view(np.uint32), ref.view(np.uint32))
    restated = oracle.grid_sample(vol, grid) if mode == "bilinear" else nearest64(vol, grid)
    assert np.array_equal(hip.view(np.uint32), restated.view(np.uint32))
    if torch_grid_is_chain:                                         # the whole torch chain, where this host's affine_grid rounds like it
        assert np.array_equal(hip.view(np.uint32), torch_warp(vol, theta, out_size, mode).view(np.uint32))
    if case == "identity" and mode == "nearest":
        assert np.array_equal(hip, vol)
    if case == "all_outside":
        assert not hip.any()


def test_affine_warp_ranks_and_theta_forms():
    from convexadam_amd.rigid import affine_warp
    g = np.random.default_rng(8)
    vol = dev(g.normal(size=(2, 12, 14, 16)).astype(np.float32))
    th = rot(g, 15.0, (0.1, 0.0, 0.0))
    T4 = np.r_[th, [[0, 0, 0, 1]]].astype(np.float32)
    a = affine_warp(vol, dev(th))
    assert torch.equal(a, affine_warp(vol, dev(T4)))
    assert torch.equal(a, affine_warp(vol, dev(th[None])))
    b = affine_warp(vol.unsqueeze(0), dev(th))
    assert b.shape == (1, 2, 12, 14, 16) and torch.equal(a, b[0])


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def field_samples_torch(disp_hr, mask, g):
    """CuRIOUS:349-365 on torch CPU (float32)."""
    _, _, H, W, D = disp_hr.shape
    affine = F.affine_grid(torch.eye(3, 4).unsqueeze(0), (1, 1, H, W, D), align_corners=False)
    disp0 = (disp_hr.float().permute(0, 2, 3, 4, 1) / torch.tensor([H - 1, W - 1, D - 1]).view(1, 1, 1, 1, 3) * 2).flip(4)
    sp = F.affine_grid(torch.eye(3, 4).unsqueeze(0), (1, 1, H // g, W // g, D // g), align_corners=False)
    sp = sp.reshape(-1, 3)[torch.nonzero(mask.reshape(-1)), :]
    T1 = F.grid_sample(affine.permute(0, 4, 1, 2, 3), sp.reshape(1, -1, 1, 1, 3), align_corners=False)
    T2 = F.grid_sample((affine + disp0).permute(0, 4, 1, 2, 3), sp.reshape(1, -1, 1, 1, 3), align_corners=False)
    T1 = torch.cat((T1.squeeze().t(), torch.ones(sp.shape[0], 1)), 1)
    T2 = torch.cat((T2.squeeze().t(), torch.ones(sp.shape[0], 1)), 1)
    return T1, T2


def test_field_samples_bit_identical_to_torch():
    from convexadam_amd.rigid import _field_samples
    gen = torch.Generator().manual_seed(9)
    H, W, D, g = 40, 36, 44, 4
    disp_hr = F.interpolate(torch.randn(1, 3, 5, 5, 6, generator=gen) * 3, (H, W, D), mode="trilinear", align_corners=False)
    mask = torch.rand(1, 1, H // g, W // g, D // g, generator=gen) > 0.4
    T1, T2 = _field_samples(disp_hr.to(DEV), mask.to(DEV), g)
    R1, R2 = field_samples_torch(disp_hr, mask, g)
    assert torch.equal(T1.cpu(), R1) and torch.equal(T2.cpu(), R2)


def test_rigid_motion_field_is_recovered():
    from convexadam_amd.rigid import rigid_from_field
    g = np.random.default_rng(10)
    H, W, D, sp = 48, 44, 52, 4
    R = rot(g, 4.0, (0.03, -0.02, 0.015)).astype(np.float64)
    ident = F.affine_grid(torch.eye(3, 4, dtype=torch.float64).unsqueeze(0), (1, 1, H, W, D), align_corners=False)[0].numpy()
    disp0 = ident @ R[:, :3].T + R[:, 3] - ident                    # (H, W, D, 3) in (x, y, z)
    disp_hr = np.stack([disp0[..., 2] * (H - 1) / 2, disp0[..., 1] * (W - 1) / 2, disp0[..., 0] * (D - 1) / 2])
    mask = np.zeros((H // sp, W // sp, D // sp), bool)
    mask[1:-1, 1:-1, 1:-1] = True
    cells = np.argwhere(mask)
    bad = cells[g.permutation(len(cells))[:len(cells) // 5]]
    for (a, b, c) in bad:                                           # corrupt 20 % of the masked cells' blocks
        disp_hr[:, a * sp:(a + 1) * sp, b * sp:(b + 1) * sp, c * sp:(c + 1) * sp] += g.normal(size=3)[:, None, None, None] * 4
    T = rigid_from_field(dev(disp_hr.astype(np.float32)), torch.as_tensor(mask), sp, 15).cpu().numpy()
    assert np.abs(T[:3] - R).max() <= 1e-4, np.abs(T[:3] - R).max()
    check_rotation(T)


def test_phantom_label_warp_matches_torch():
    from convexadam_amd.convex_adam_MIND import convex_adam_pt
    from convexadam_amd.phantom import phantom
    from convexadam_amd.rigid import _field_samples, affine_warp, least_trimmed_rigid, rigid_from_field
    shape, sp = (48, 44, 52), 4
    fix = phantom(shape, 1, 10)
    mov = torch.roll(phantom(shape, 1, 11), (2, -1, 1), (0, 1, 2))
    out = convex_adam_pt(fix, mov, dtype=torch.float32, device=torch.device(DEV), grid_sp=sp, disp_hw=3, selected_niter=20, grid_sp_adam=2)
    disp_hr = torch.from_numpy(np.ascontiguousarray(out)).float().permute(3, 0, 1, 2).unsqueeze(0).contiguous()
    mask = F.avg_pool3d((fix > float(fix.median())).float()[None, None], sp, stride=sp) > 0.5
    R = rigid_from_field(disp_hr.to(DEV), mask.to(DEV), sp, 15)
    assert torch.equal(R, least_trimmed_rigid(*_field_samples(disp_hr.to(DEV), mask.to(DEV), sp), 15))
    check_rotation(R.cpu().numpy())
    seg = torch.bucketize(mov, torch.tensor([-0.5, 0.0, 0.5])).float()
    warped = affine_warp(seg.view(1, 1, *shape).to(DEV), R, mode="nearest").cpu()
    grid, torch_grid_is_chain = torch_affine_grid_is_the_chain(R.cpu().numpy(), shape)
    ref = F.grid_sample(seg.view(1, 1, *shape), torch.as_tensor(grid)[None], mode="nearest", align_corners=False)
    assert torch.equal(warped, ref)
    if torch_grid_is_chain:
        ref = F.grid_sample(seg.view(1, 1, *shape), F.affine_grid(R[:3].cpu().unsqueeze(0), (1, 1) + shape, align_corners=False),
                            mode="nearest", align_corners=False)
        assert torch.equal(warped, ref)


# ---- errors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_point_raises_and_writes_nothing(bad):
    import ctypes as C
    from convexadam_amd import _lib
    from convexadam_amd.rigid import least_trimmed_rigid
    z = golden()
    f, m = z["outliers_fixed"].copy(), z["outliers_moving"]
    f[17, 1] = bad
    L = _lib.lib()
    n = f.shape[0]
    nws = L.cvx_rigid_lts_workspace_bytes(n)
    ws = torch.full((nws,), 7, dtype=torch.uint8, device=DEV)
    T = torch.full((4, 4), -5.0, device=DEV)
    mask = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    fd, md = dev(f), dev(m)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = _lib.stream_ptr(fd.device)
    rc = L.cvx_rigid_lts_f32(p(fd), 4, p(md), 4, n, 5, p(T), p(mask), p(ws), nws, stream)
    assert rc == _lib.CVX_ERR_INVALID_ARG and b"non-finite" in L.cvx_last_error()
    assert (T == -5.0).all() and (mask == 9).all()
    with pytest.raises(_lib.CvxError, match="non-finite"):
        least_trimmed_rigid(fd, md, 5)
    # the workspace stays usable: the same buffers on good points give the fresh result
    good = dev(z["outliers_fixed"])
    assert L.cvx_rigid_lts_f32(p(good), 4, p(md), 4, n, 5, p(T), p(mask), p(ws), nws, stream) == 0
    ref, ref_mask = least_trimmed_rigid(good, md, 5, return_inliers=True)
    assert torch.equal(T, ref) and torch.equal(mask.bool(), ref_mask)


def test_nan_in_a_trimmed_away_point_is_not_an_error():
    from convexadam_amd.rigid import least_trimmed_rigid
    z = golden()
    f, m = z["outliers_fixed"], z["outliers_moving"].copy()
    m[5, 3] = np.nan                                                # column 3 only: the fits never read it, its residual sorts last
    T, mask = least_trimmed_rigid(dev(f), dev(m), 5, return_inliers=True)
    assert not mask[5].item()
    check_rotation(T.cpu().numpy())
