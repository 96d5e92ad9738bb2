"""The affine model around the convex stage (csrc/affine.hip): least_trimmed_squares of l2r_2020_convexAdam_CuRIOUS.py:272-278,
the affine twin of least_trimmed_rigid, with everything a user needs around it.

    find_affine_3d(x, y)                               the least-squares affine T (4, 4) with y_i^T ~ T x_i^T -- find_rigid_3d's orientation
    least_trimmed_affine(fixed_pts, moving_pts, iter)  `iter` least-squares fits, each later one on the half with the smallest residuals
    least_trimmed_squares(fixed_pts, moving_pts, iter) the reference's function: its name, its equation and its return orientation
    affine_from_field(disp_hr, mask_coarse, grid_sp)   rigid_from_field with the affine fit
    convex_adam_affine(img_fixed, imgs_moving, ...)    convex_adam_rigid with the affine fit, optionally in several rounds
    affine_to_field(T, shape, field=None)              the affine (after `field`) as ONE displacement field, analytic, float64
    register_with_affine(img_fixed, img_moving, ...)   affine pre-alignment + convex_adam_pt, returned as one pull-back field

Every fit -- all trimming iterations -- is one launch of k_affine_lts; a theta never leaves the device.  Device tensors are required where
rigid.py requires them; there is no CPU path.
"""
import torch

from ._lib import _shape, call, f32c, field_operand_from, ptr, require_device_tensor
from .rigid import _field_samples, _fit, _point_pair, _register, _trimmed_iters, _volume, affine_warp

MIN_CELLS = 8          # a trimmed affine fit works on n // 2 >= 4 points


def find_affine_3d(x, y):
    """(4, 4) float32 T = [A t; 0 0 0 1] with y[:, :3] ~ x[:, :3] A^T + t in the least-squares sense: the orientation find_rigid_3d returns,
    without its restriction to rotations.  x, y: (N, k >= 3) device tensors, N >= 4; columns beyond the third are ignored.  Raises
    CvxError on coplanar points (a singular system) or a non-finite coordinate."""
    _point_pair(x, y, ("x", "y"), 4)
    return _fit("cvx_affine_lts", x[:, :3], y[:, :3], False, 1, 0).t().contiguous()


def _trimmed(fixed_pts, moving_pts, iter, normal, return_inliers):
    n = _point_pair(fixed_pts, moving_pts, ("fixed_pts", "moving_pts"), 4, 4)
    if _trimmed_iters(iter) > 1 and n < MIN_CELLS:
        raise ValueError("a trimmed fit needs N >= %d points, got %d" % (MIN_CELLS, n))
    return _fit("cvx_affine_lts", fixed_pts, moving_pts, bool(return_inliers), int(iter), normal)


def least_trimmed_affine(fixed_pts, moving_pts, iter=5, return_inliers=False):
    """least_trimmed_rigid with an affine model: `iter` least-squares fits moving ~ fixed X, the first on all N points, each later one on
    the N // 2 points with the smallest residuals ||moving - fixed X|| under the previous fit (ties: lowest index first).  fixed_pts,
    moving_pts: (N, 4) device tensors (homogeneous points), N >= 8 (4 for iter = 1).  Returns T = X^T (4, 4) float32 -- moving_i^T ~ T
    fixed_i^T, last row exactly (0, 0, 0, 1) -- and with return_inliers=True also the (N,) bool mask of the points the returned fit used."""
    r = _trimmed(fixed_pts, moving_pts, iter, 0, return_inliers)
    return (r[0].t().contiguous(), r[1]) if return_inliers else r.t().contiguous()


def least_trimmed_squares(fixed_pts, moving_pts, iter=5):
    """least_trimmed_squares of l2r_2020_convexAdam_CuRIOUS.py:272-278 with its name, its equation and its return value: per fit
    x, _ = torch.solve(M^T M, M^T F), i.e. (M^T F) x = M^T M over the current rows F, M of fixed_pts, moving_pts -- an instrumental-variable
    form of moving ~ fixed x that equals the least-squares solution when the fit is exact -- then the N // 2 smallest residuals
    ||moving - fixed x||.  Returns x (4, 4) float32, NOT transposed: use least_trimmed_affine for the least-squares fit and a theta."""
    return _trimmed(fixed_pts, moving_pts, iter, 1, False)


def affine_from_field(disp_hr, mask_coarse, grid_sp, iter=15):
    """rigid_from_field with the affine fit: least_trimmed_affine(T1, T2, iter) with T1 the identity coordinates and T2 the displaced ones
    (normalised, x/y/z order) of the masked coarse cells.

    disp_hr     (1, 3, H, W, D) or (3, H, W, D) device tensor, displacement in voxels (channel a along array axis a)
    mask_coarse (H // grid_sp, W // grid_sp, D // grid_sp) tensor (any device, optionally with leading 1s), nonzero = use the cell
    Returns T (4, 4) float32: F.affine_grid(T[:3], ...) / affine_warp(vol, T) warp the moving image."""
    if int(iter) < 1:
        raise ValueError("iter must be >= 1, got %r" % (iter,))
    T1, T2 = _field_samples(disp_hr, mask_coarse, grid_sp)
    if int(T1.shape[0]) < MIN_CELLS:
        raise ValueError("mask_coarse selects %d cells; the affine fit needs at least %d" % (int(T1.shape[0]), MIN_CELLS))
    return least_trimmed_affine(T1, T2, int(iter))


class AffineRegistration:
    """Result of convex_adam_affine: T (4, 4) float32 on the device; mask_fix, mask_mov (h, w, d) bool and disp_hr (1, 3, H, W, D) voxels
    of the FIRST round (disp_hr with return_field=True or label volumes given, else None); tre_before, tre_deformable, tre_affine:
    per-label float64 CPU tensors of landmark_tre (label volumes given, else None)."""

    def __init__(self, T, mask_fix, mask_mov, disp_hr=None, tre_before=None, tre_deformable=None, tre_affine=None):
        self.T, self.mask_fix, self.mask_mov, self.disp_hr = T, mask_fix, mask_mov, disp_hr
        self.tre_before, self.tre_deformable, self.tre_affine = tre_before, tre_deformable, tre_affine


def convex_adam_affine(img_fixed, imgs_moving, mind_r=3, mind_d=3, grid_sp=6, disp_hw=6, mask_thresh=10., ic_iters=5, lts_iters=15,
                       seg_fixed=None, seg_moving=None, return_field=False, rounds=1):
    """convex_adam_rigid with an affine model: MIND-SSC features pooled to the coarse grid, the convex stage on cost volumes masked by
    coarse foreground masks, and a least-trimmed AFFINE fit (least_trimmed_affine) to the displaced coarse cells.  The arguments are those
    of convex_adam_rigid, plus

    rounds       > 1: the moving images are warped with the current T (affine_warp), stage and fit run again on the warped images, and
                 the 4 x 4 matrices are multiplied in float64 on the device (T <- T T_round).  This reaches motions beyond one search
                 range of grid_sp * disp_hw voxels and removes the whole-cell quantisation of the first fit.
    Returns an AffineRegistration.  T approximates the INVERSE of a matrix A that built the moving image as F.grid_sample(fixed,
    F.affine_grid(A)) (pull-back convention): affine_warp(moving, T) brings the moving image onto the fixed one.  A scale or shear
    difference between the scans, which a rigid fit cannot absorb, is part of T."""
    return _register(least_trimmed_affine, MIN_CELLS, "affine", AffineRegistration, "tre_affine", img_fixed, imgs_moving, mind_r, mind_d, grid_sp,
                     disp_hw, mask_thresh, ic_iters, lts_iters, seg_fixed, seg_moving, return_field, rounds)


def affine_to_field(T, shape, field=None):
    """The displacement field of an affine, in voxels: out(x) = A(x + field(x)) - x with A the map F.affine_grid(T[:3], align_corners=False)
    / affine_warp(.., T) describe, so that apply_convex(out, moving) is moving pulled through T (after `field`, if given: the single field
    equal to affine_warp(moving, T) followed by the warp with `field`).  Evaluated analytically in float64 -- no interpolation, no padding
    rule, which composing with a sampled affine field through compose_fields would bring in.

    T      (3, 4), (1, 3, 4) or (4, 4) device tensor (read on the device)
    shape  (H, W, D)
    field  None, or a displacement field on that grid: an (H, W, D, 3) array / host tensor (uploaded), or a device tensor (H, W, D, 3) or
           (3, H, W, D), float32 or float64, read in place
    Returns a float64 device tensor, (H, W, D, 3) -- or (3, H, W, D) where `field` is a device tensor of that layout."""
    ts = _shape(T, "T")
    if ts not in ((3, 4), (4, 4), (1, 3, 4)):
        raise ValueError("T must be (3, 4), (1, 3, 4) or (4, 4), got %s" % (ts,))
    try:
        H, W, D = [int(s) for s in shape]
    except (TypeError, ValueError):
        raise ValueError("shape must be three positive ints, got %r" % (shape,)) from None
    if min(H, W, D) < 1:
        raise ValueError("shape must be three positive ints, got %r" % (shape,))
    th = f32c(require_device_tensor(T, "T").reshape(-1, 4)[:3])
    dev = th.device
    if field is None:
        u, cs, vs, u64 = None, 0, 0, 0
        out = torch.empty((H, W, D, 3), dtype=torch.float64, device=dev)
        ocs, ovs = 1, 3
    else:
        u, ushape, cs, vs, u64, _ = field_operand_from(field, "field", dev)
        if ushape != (H, W, D) or u.device != dev:
            raise ValueError("affine_to_field: field is %s on %s, shape %s and T on %s" % (ushape, u.device, (H, W, D), dev))
        out = torch.empty(u.shape, dtype=torch.float64, device=dev)
        ocs, ovs = cs, vs
    call(dev, "cvx_affine_field_f64", ptr(th), H, W, D, ptr(u), u64, cs, vs, ptr(out), 1, ocs, ovs)
    return out


def register_with_affine(img_fixed, img_moving, affine_kwargs=None, **kw):
    """Affine pre-alignment followed by the deformable registration, returned as ONE field:

      1. res = convex_adam_affine(img_fixed, img_moving, **affine_kwargs)
      2. deformable = convex_adam_pt(img_fixed, affine_warp(img_moving, res.T), **kw)
      3. field = affine_to_field(res.T, shape, field=deformable)

    img_fixed, img_moving: (H, W, D) device tensors.  Returns (field, T): field (H, W, D, 3) float64 on the device, the pull-back field
    with fixed(x) ~ moving(x + field(x)) that apply_convex takes as it is; T (4, 4) float32 on the device."""
    from .convex_adam_MIND import convex_adam_pt
    shape = _volume(img_fixed, "img_fixed")
    if _volume(img_moving, "img_moving") != shape:
        raise ValueError("img_moving has extent %s, the fixed image %s" % (_volume(img_moving, "img_moving"), shape))
    fix = f32c(require_device_tensor(img_fixed, "img_fixed")).reshape(shape)
    mov = f32c(require_device_tensor(img_moving, "img_moving")).reshape(shape)
    res = convex_adam_affine(fix, mov, **(affine_kwargs or {}))
    warped = affine_warp(mov[None], res.T)[0]
    kw.setdefault("device", fix.device)
    deformable = convex_adam_pt(fix, warped, **kw)
    return affine_to_field(res.T, shape, field=deformable), res.T
