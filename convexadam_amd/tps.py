"""Thin-plate-spline densification of a field known at sparse points (l2r_2021_convexAdam_task1_docker.py:198-262,365-387).

`TPS` and `thin_plate_dense` keep the reference's names, signatures and return layouts; the work runs in csrc/tps.hip (system assembly,
blocked LU with partial pivoting, spline evaluation, align_corners=True up-sampling).  `tps_densify` is the composition the 2021 lung-CT
script runs on the registered field after its Adam stage.
"""
import torch

from ._lib import _shape, call, f32c, ptr, require_device_tensor, scratch

_MAX_RHS = 4


def _centres(c, name="c"):
    """n of a (n, 3) centre array, n >= 1."""
    s = _shape(c, name)
    if len(s) != 2 or s[1] != 3 or s[0] < 1:
        raise ValueError("%s must be (n, 3) with n >= 1, got %s" % (name, s))
    return s[0]


def _theta(theta, n):
    s = _shape(theta, "theta")
    if len(s) != 2 or s[0] != n + 4 or s[1] < 1:
        raise ValueError("theta must be (n+4, f_dim) with n = %d and f_dim >= 1, got %s" % (n, s))


def _columns(t, name):
    """(k, d) float32 device tensor, shape already checked -> list of contiguous (k, <=4) column groups (the library takes at most 4
    right-hand sides)."""
    t = f32c(require_device_tensor(t, name))
    return [t[:, i:i + _MAX_RHS].contiguous() for i in range(0, t.shape[1], _MAX_RHS)]


class TPS:
    @staticmethod
    def fit(c, f, lambd=0.):
        """theta (n+4, f_dim) of the spline through f at the centres c (n, 3): solves [U(d(c,c)) + lambd I, P; P^T, 0] theta = [f; 0]
        (task1:200-222).  Raises CvxError ("singular system") on a zero or non-finite pivot, e.g. duplicate centres with lambd = 0."""
        n = _centres(c)
        fs = _shape(f, "f")
        if len(fs) != 2 or fs[0] != n or fs[1] < 1:
            raise ValueError("f must be (n, f_dim) with n = %d and f_dim >= 1, got %s" % (n, fs))
        c = f32c(require_device_tensor(c, "c"))
        parts = []
        for fk in _columns(f, "f"):
            nr = int(fk.shape[1])
            theta = torch.zeros((n + 4, nr), dtype=torch.float32, device=c.device)
            ws = scratch(c.device, "cvx_tps_fit_workspace_bytes", n, nr)
            if ws[1] == 0:
                raise ValueError("TPS.fit: n = %d centres is outside what the library supports" % n)
            call(c.device, "cvx_tps_fit_f32", ptr(c), ptr(fk), n, nr, float(lambd), ptr(theta), *ws)
            parts.append(theta)
        return parts[0] if len(parts) == 1 else torch.cat(parts, 1)

    @staticmethod
    def d(a, b):
        """Pairwise distances (n, m) of a (n, 3) and b (m, 3): d(a, b) of the reference (task1:224-230) from direct differences."""
        a, b = f32c(require_device_tensor(a, "a")), f32c(require_device_tensor(b, "b"))
        # the spline kernel evaluates U, not d: d is a tiny O(nm) helper, kept for the reference's interface
        return torch.cdist(a.unsqueeze(0), b.unsqueeze(0), compute_mode="donot_use_mm_for_euclid_dist")[0]

    @staticmethod
    def u(r):
        """U(r) = r^2 log(r + 1e-6) (task1:232-234)."""
        return (r ** 2) * torch.log(r + 1e-6)

    @staticmethod
    def z(x, c, theta):
        """Spline value (m, f_dim) at the points x (m, 3) (task1:236-241)."""
        xs = _shape(x, "x")
        if len(xs) != 2 or xs[1] != 3:
            raise ValueError("x must be (m, 3), got %s" % (xs,))
        n, m = _centres(c), xs[0]
        _theta(theta, n)
        x = f32c(require_device_tensor(x, "x"))
        c = f32c(require_device_tensor(c, "c"))
        parts = []
        for th in _columns(theta, "theta"):
            nr = int(th.shape[1])
            out = torch.empty((m, nr), dtype=torch.float32, device=x.device)
            call(x.device, "cvx_tps_eval_f32", ptr(x), m, ptr(c), ptr(th), n, nr, ptr(out))
            parts.append(out)
        return parts[0] if len(parts) == 1 else torch.cat(parts, 1)


def tps_dense(c, theta, size):
    """The spline at the F.affine_grid(eye, (1,1)+size, align_corners=True) lattice, generated in the kernel: (f_dim,) + size."""
    n = _centres(c)
    _theta(theta, n)
    try:
        s0, s1, s2 = [int(s) for s in size]
    except (TypeError, ValueError):
        raise ValueError("size must be three positive ints, got %r" % (size,)) from None
    if min(s0, s1, s2) < 1:
        raise ValueError("size must be three positive ints, got %r" % (size,))
    c = f32c(require_device_tensor(c, "c"))
    parts = []
    for th in _columns(theta, "theta"):
        nr = int(th.shape[1])
        out = torch.empty((nr, s0, s1, s2), dtype=torch.float32, device=c.device)
        call(c.device, "cvx_tps_dense_f32", s0, s1, s2, ptr(c), ptr(th), n, nr, ptr(out))
        parts.append(out)
    return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def resize_trilinear_ac(x, size):
    """F.interpolate(x, size=size, mode='trilinear', align_corners=True) for (N,C,h,w,d) (task1:260).  The contiguous (N, C, h, w, d)
    input is the (1, N*C, h, w, d) one, so the batch rides along as channels."""
    xs = _shape(x, "x")
    if len(xs) != 5:
        raise ValueError("x must be (N, C, h, w, d), got %s" % (xs,))
    Nb, Cn, h, w, d = xs
    H, W, D = [int(s) for s in size]
    a = f32c(require_device_tensor(x, "x"))
    out = torch.empty((Nb, Cn, H, W, D), dtype=torch.float32, device=a.device)
    call(a.device, "cvx_resize_trilinear_ac_f32", ptr(a), Nb * Cn, h, w, d, ptr(out), H, W, D)
    return out


def thin_plate_dense(x1, y1, shape, step, lambd=.0, unroll_step_size=2**12):
    """thin_plate_dense of task1:242-262: fits the spline through y1 (1, n, f_dim) at x1 (1, n, 3), evaluates it on the align_corners=True
    lattice of shape // step and up-samples that trilinearly (align_corners=True) to `shape`.  Returns (1, D, H, W, f_dim) (a permuted
    view, as the reference's).  `unroll_step_size` is accepted for the reference's signature and has no effect: the lattice is never
    materialised."""
    del unroll_step_size
    D, H, W = [int(s) for s in shape]
    D1, H1, W1 = D // step, H // step, W // step
    theta = TPS.fit(x1[0], y1[0], lambd)
    y2 = tps_dense(x1[0], theta, (D1, H1, W1)).unsqueeze(0)
    return resize_trilinear_ac(y2, (D, H, W)).permute(0, 2, 3, 4, 1)


def tps_densify(disp_hr, fixed_mask, n_points=4096, step=4, lambd=0., generator=None):
    """The TPS step of task1:365-387 on a registered field.

    disp_hr    (1, 3, H, W, D) or (3, H, W, D) device tensor, displacement in voxels (channel a along array axis a), as the
               reference's `disp_hr`
    fixed_mask (H, W, D) tensor (any device), > 0 inside
    Returns the densified, smoothed field (1, 3, H, W, D) float32 in voxels (the reference's `disp_smooth`).

    1. the stride-3 lattice F.affine_grid(eye, (1,1,H//3,W//3,D//3), align_corners=True) restricted to fixed_mask[1::3,1::3,1::3];
    2. n_points of its in-mask points picked by torch.randperm(count, generator=generator) (host side: a seeded CPU generator makes the
       choice deterministic);
    3. the field, normalised and flipped to (x, y, z) order, sampled there by grid_sample with align_corners=False -- the reference's
       mix as written: an align_corners=True lattice sampled with the default False (task1:377);
    4. thin_plate_dense(points, samples, (H, W, D), step, lambd);
    5. back to voxels and three box_smooth(., 3) passes (task1:383,387).
    """
    from .convex_adam_utils import box_smooth, grid_sample
    disp_hr = require_device_tensor(disp_hr, "disp_hr")
    if disp_hr.dim() == 4:
        disp_hr = disp_hr.unsqueeze(0)
    dev = disp_hr.device
    H, W, D = [int(s) for s in disp_hr.shape[2:]]
    scale = torch.tensor([H - 1, W - 1, D - 1], dtype=torch.float32, device=dev)
    ident = torch.nn.functional.affine_grid(torch.eye(3, 4, device=dev).unsqueeze(0), (1, 1, H // 3, W // 3, D // 3), align_corners=True)
    disp = (f32c(disp_hr).permute(0, 2, 3, 4, 1) / scale.view(1, 1, 1, 1, 3) * 2).flip(4)
    mask3 = torch.as_tensor(fixed_mask)[1::3, 1::3, 1::3][:ident.shape[1], :ident.shape[2], :ident.shape[3]]
    inside = mask3.reshape(-1).to(dev) > 0
    ident1 = ident.view(-1, 3)[inside, :]
    pick = torch.randperm(int(ident1.shape[0]), generator=generator)[:int(n_points)].to(dev)
    ident_mask = ident1[pick]
    sampled = grid_sample(disp.permute(0, 4, 1, 2, 3).contiguous(), ident_mask.view(1, -1, 1, 1, 3))
    disp_sampled = sampled.view(1, 3, -1).permute(0, 2, 1)
    dense = thin_plate_dense(ident_mask.unsqueeze(0), disp_sampled, (H, W, D), step, lambd)
    dense_flow = dense.flip(4).permute(0, 4, 1, 2, 3) * scale.view(1, 3, 1, 1, 1) / 2
    return box_smooth(dense_flow.contiguous(), 3, passes=3)
