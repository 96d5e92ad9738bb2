"""Least-trimmed rigid fit and fused affine warp (convex_adam_utils.py:173-193; l2r_2020_convexAdam_CuRIOUS.py:349-390).

`find_rigid_3d` and `least_trimmed_rigid` keep the reference's names, positional signatures and (4, 4) float32 results; the whole fit --
every trimming iteration -- is one launch of csrc/rigid.hip.  `affine_warp` is F.grid_sample(vol, F.affine_grid(theta, ...)) with the
grid computed in the kernel.  `rigid_from_field` is the CuRIOUS script's rigid step after its convex stage.
"""
import torch

from ._lib import check, f32c, lib, ptr, require_device_tensor, stream_ptr, workspace
from .tps import _shape

_MODES = {"bilinear": 0, "nearest": 1}


def _points(t, name, exact_cols=None):
    s = _shape(t, name)
    if len(s) != 2 or s[0] < 2 or (s[1] != exact_cols if exact_cols else s[1] < 3):
        want = "(N, %d)" % exact_cols if exact_cols else "(N, k) with k >= 3"
        raise ValueError("%s must be %s and N >= 2, got %s" % (name, want, s))
    return s


def _fit(fixed, moving, iters, want_inliers):
    f = f32c(require_device_tensor(fixed, "fixed"))
    m = f32c(require_device_tensor(moving, "moving"))
    if m.device != f.device:
        raise ValueError("both point sets must live on one device (%s, %s)" % (f.device, m.device))
    n = int(f.shape[0])
    T = torch.empty((4, 4), dtype=torch.float32, device=f.device)
    mask = torch.empty(n, dtype=torch.uint8, device=f.device) if want_inliers else None
    with torch.cuda.device(f.device):
        nws = lib().cvx_rigid_lts_workspace_bytes(n)
        ws = workspace(nws, f.device)
        check(lib().cvx_rigid_lts_f32(ptr(f), int(f.shape[1]), ptr(m), int(m.shape[1]), n, int(iters), ptr(T), ptr(mask), ptr(ws), nws,
                                      stream_ptr(f.device)))
    return (T, mask.bool()) if want_inliers else T


def find_rigid_3d(x, y):
    """(4, 4) T = [R t; 0 0 0 1] with y[:, :3] ~ x[:, :3] R^T + t, R the optimal proper rotation (convex_adam_utils.py:173-184).
    x, y: (N, k >= 3) device tensors, N >= 2.  Raises CvxError on a non-finite coordinate (the reference's torch.svd raises too)."""
    sx, sy = _points(x, "x"), _points(y, "y")
    if sx[0] != sy[0]:
        raise ValueError("x and y must have the same number of points, got %d and %d" % (sx[0], sy[0]))
    return _fit(x, y, 1, False)


def least_trimmed_rigid(fixed_pts, moving_pts, iter=5, return_inliers=False):
    """least_trimmed_rigid of convex_adam_utils.py:187-193: `iter` rigid fits, the first on all N points, each later one on the N // 2
    points with the smallest residuals ||moving - fixed T^T|| under the previous fit (ties: lowest index first).  fixed_pts, moving_pts:
    (N, 4) device tensors (homogeneous points).  Returns T (4, 4) float32, and with return_inliers=True also the (N,) bool mask of the
    points the returned fit used."""
    sf, sm = _points(fixed_pts, "fixed_pts", 4), _points(moving_pts, "moving_pts", 4)
    if sf[0] != sm[0]:
        raise ValueError("fixed_pts and moving_pts must have the same number of points, got %d and %d" % (sf[0], sm[0]))
    if int(iter) < 1:
        raise ValueError("iter must be >= 1, got %r" % (iter,))
    return _fit(fixed_pts, moving_pts, int(iter), bool(return_inliers))


def affine_warp(vol, theta, size=None, mode="bilinear"):
    """F.grid_sample(vol, F.affine_grid(theta[:3], (1, C) + size, align_corners=False), mode=mode, padding_mode='zeros',
    align_corners=False) without the (size, 3) grid.  vol (C, h, w, d) or (1, C, h, w, d) (returned in the same rank, float32);
    theta (3, 4), (1, 3, 4) or (4, 4) on vol's device (read there by the kernel); size (ho, wo, do), default (h, w, d)."""
    vs = _shape(vol, "vol")
    if len(vs) == 5 and vs[0] == 1:
        Cn, h, w, d = vs[1:]
    elif len(vs) == 4:
        Cn, h, w, d = vs
    else:
        raise ValueError("vol must be (C, h, w, d) or (1, C, h, w, d), got %s" % (vs,))
    ts = _shape(theta, "theta")
    if ts not in ((3, 4), (4, 4), (1, 3, 4)):
        raise ValueError("theta must be (3, 4), (1, 3, 4) or (4, 4), got %s" % (ts,))
    if mode not in _MODES:
        raise ValueError("mode must be 'bilinear' or 'nearest', got %r" % (mode,))
    try:
        ho, wo, do_ = (h, w, d) if size is None else [int(s) for s in size]
    except (TypeError, ValueError):
        raise ValueError("size must be three positive ints, got %r" % (size,)) from None
    if min(ho, wo, do_) < 1 or min(Cn, h, w, d) < 1:
        raise ValueError("empty volume or size: vol %s, size %r" % (vs, size))
    a = f32c(require_device_tensor(vol, "vol"))
    th = f32c(require_device_tensor(theta, "theta").reshape(-1, 4)[:3])
    if th.device != a.device:
        raise ValueError("theta must live on vol's device (%s, %s)" % (th.device, a.device))
    out = torch.empty((Cn, ho, wo, do_), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        check(lib().cvx_affine_warp_f32(ptr(a), Cn, h, w, d, ptr(th), ho, wo, do_, _MODES[mode], ptr(out), stream_ptr(a.device)))
    return out.unsqueeze(0) if len(vs) == 5 else out


def _field_samples(disp_hr, mask_coarse, grid_sp):
    """T1, T2 of CuRIOUS:360-365 as (M, 4) float32: the identity and identity + disp0 volumes (float32, formed as the reference forms
    them) sampled by cvx_grid_sample_f32 at the F.affine_grid(eye, coarse, align_corners=False) coordinates of the masked coarse cells in
    torch.nonzero order, with a ones column appended."""
    from .convex_adam_utils import _base_tables
    ds = _shape(disp_hr, "disp_hr")
    if len(ds) == 5 and ds[0] == 1:
        ds = ds[1:]
    if len(ds) != 4 or ds[0] != 3:
        raise ValueError("disp_hr must be (3, H, W, D) or (1, 3, H, W, D), got %s" % (_shape(disp_hr, "disp_hr"),))
    H, W, D = ds[1:]
    g = int(grid_sp)
    if g < 1 or min(H // g, W // g, D // g) < 1 or min(H, W, D) < 2:
        raise ValueError("grid_sp = %r does not fit the field extent %s" % (grid_sp, (H, W, D)))
    Hc, Wc, Dc = H // g, W // g, D // g
    ms = _shape(mask_coarse, "mask_coarse")
    if len(ms) < 3 or ms[-3:] != (Hc, Wc, Dc) or any(s != 1 for s in ms[:-3]):
        raise ValueError("mask_coarse must be (%d, %d, %d) (optionally with leading 1s), got %s" % (Hc, Wc, Dc, ms))
    disp = f32c(require_device_tensor(disp_hr, "disp_hr")).reshape(3, H, W, D)
    dev = disp.device
    with torch.cuda.device(dev):
        bh, bw, bd = _base_tables(H, W, D, dev)
        ident = torch.stack([bd.view(1, 1, D).expand(H, W, D), bw.view(1, W, 1).expand(H, W, D), bh.view(H, 1, 1).expand(H, W, D)])
        # disp_hr / (size - 1) * 2 flipped to (x, y, z), divided by a DEVICE tensor as the reference does (true division; a Python
        # scalar divisor would be applied as a multiplication by its reciprocal on the device)
        scale = torch.tensor([D - 1, W - 1, H - 1], dtype=torch.float32, device=dev).view(3, 1, 1, 1)
        moved = ident + disp.flip(0) / scale * 2
        idx = torch.nonzero(torch.as_tensor(mask_coarse).to(dev).reshape(-1)).reshape(-1)
        M = int(idx.numel())
        if M < 2:
            raise ValueError("mask_coarse selects %d cells; the fit needs at least 2" % M)
        ch, cw, cd = _base_tables(Hc, Wc, Dc, dev)
        pts = torch.stack([cd[idx % Dc], cw[(idx // Dc) % Wc], ch[idx // (Wc * Dc)]], 1).contiguous()
        out = []
        for v in (ident, moved):
            s = torch.empty((3, M), dtype=torch.float32, device=dev)
            check(lib().cvx_grid_sample_f32(ptr(v), 3, H, W, D, ptr(pts), M, 1, 1, ptr(s), stream_ptr(dev)))
            out.append(torch.cat([s.t(), torch.ones((M, 1), dtype=torch.float32, device=dev)], 1).contiguous())
    return out[0], out[1]


def rigid_from_field(disp_hr, mask_coarse, grid_sp, iter=15):
    """The rigid step of CuRIOUS:349-367 on a registered field: least_trimmed_rigid(T1, T2, iter) with T1 the identity coordinates and
    T2 the displaced ones (normalised, x/y/z order) of the masked coarse cells.

    disp_hr     (1, 3, H, W, D) or (3, H, W, D) device tensor, displacement in voxels (channel a along array axis a)
    mask_coarse (H // grid_sp, W // grid_sp, D // grid_sp) tensor (any device, optionally with leading 1s), nonzero = use the cell
    Returns R (4, 4) float32: F.affine_grid(R[:3], ...) / affine_warp(vol, R) warp the moving image rigidly."""
    if int(iter) < 1:
        raise ValueError("iter must be >= 1, got %r" % (iter,))
    T1, T2 = _field_samples(disp_hr, mask_coarse, grid_sp)
    return least_trimmed_rigid(T1, T2, int(iter))
