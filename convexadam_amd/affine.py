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

from . import _affine
from ._lib import check, f32c, ptr, require_device_tensor, stream_ptr, workspace
from .rigid import (_field_samples, _shape, _volume, affine_warp, convex_stage, landmark_tre, rigid_samples,
                    threshold_pool_mask)

MIN_CELLS = 8          # a trimmed affine fit works on n // 2 >= 4 points


def _points(t, name, exact_cols=None):
    s = _shape(t, name)
    if len(s) != 2 or s[0] < 4 or (s[1] != exact_cols if exact_cols else s[1] < 3):
        want = "(N, %d)" % exact_cols if exact_cols else "(N, k) with k >= 3"
        raise ValueError("%s must be %s and N >= 4, got %s" % (name, want, s))
    return s


def _fit(fixed, moving, iters, normal, want_inliers):
    f = f32c(require_device_tensor(fixed, "fixed"))
    m = f32c(require_device_tensor(moving, "moving"))
    if m.device != f.device:
        raise ValueError("both point sets must live on one device (%s, %s)" % (f.device, m.device))
    n = int(f.shape[0])
    X = torch.empty((4, 4), dtype=torch.float32, device=f.device)
    mask = torch.empty(n, dtype=torch.uint8, device=f.device) if want_inliers else None
    L = _affine.lib()
    with torch.cuda.device(f.device):
        nws = L.cvx_affine_lts_workspace_bytes(n)
        ws = workspace(nws, f.device)
        check(L.cvx_affine_lts_f32(ptr(f), int(f.shape[1]), ptr(m), int(m.shape[1]), n, int(iters), int(normal), ptr(X), ptr(mask), ptr(ws), nws,
                                   stream_ptr(f.device)))
    return (X, mask.bool()) if want_inliers else X


def find_affine_3d(x, y):
    """(4, 4) float32 T = [A t; 0 0 0 1] with y[:, :3] ~ x[:, :3] A^T + t in the least-squares sense: the orientation find_rigid_3d returns,
    without its restriction to rotations.  x, y: (N, k >= 3) device tensors, N >= 4; columns beyond the third are ignored.  Raises
    CvxError on coplanar points (a singular system) or a non-finite coordinate."""
    sx, sy = _points(x, "x"), _points(y, "y")
    if sx[0] != sy[0]:
        raise ValueError("x and y must have the same number of points, got %d and %d" % (sx[0], sy[0]))
    return _fit(x[:, :3], y[:, :3], 1, 0, False).t().contiguous()


def _trimmed(fixed_pts, moving_pts, iter, normal, return_inliers):
    sf, sm = _points(fixed_pts, "fixed_pts", 4), _points(moving_pts, "moving_pts", 4)
    if sf[0] != sm[0]:
        raise ValueError("fixed_pts and moving_pts must have the same number of points, got %d and %d" % (sf[0], sm[0]))
    if int(iter) < 1:
        raise ValueError("iter must be >= 1, got %r" % (iter,))
    if int(iter) > 1 and sf[0] < MIN_CELLS:
        raise ValueError("a trimmed fit needs N >= %d points, got %d" % (MIN_CELLS, sf[0]))
    return _fit(fixed_pts, moving_pts, int(iter), normal, bool(return_inliers))


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


def _round(fix, movs, mind_r, mind_d, g, hw, thr, it, lts, shape, want_field, mask_thresh):
    """one masked convex stage and one trimmed affine fit -> (T, mask_fix, mask_mov, disp_hr)"""
    from .convex_adam_utils import mind_pooled
    dev = fix.device
    ff = mind_pooled(fix[None, None], mind_r, mind_d, g, device=dev)
    feat_fix = torch.cat([ff] * len(movs), 1) if len(movs) > 1 else ff
    feat_mov = torch.cat([mind_pooled(mv[None, None], mind_r, mind_d, g, device=dev) for mv in movs], 1)
    mask_fix, mask_mov = threshold_pool_mask(fix, thr, g), threshold_pool_mask(movs[0], thr, g)
    kept = int(mask_fix.sum())
    if kept < MIN_CELLS:
        raise ValueError("mask_thresh = %r keeps %d coarse cells of the fixed image; the affine fit needs at least %d" % (mask_thresh, kept, MIN_CELLS))
    coarse, disp_hr = convex_stage(feat_fix, feat_mov, g, hw, shape, mask_fix, mask_mov, it, full_res=want_field)
    T1, T2 = rigid_samples(coarse if it > 0 else coarse * g, mask_fix, g, shape)
    return least_trimmed_affine(T1, T2, lts), mask_fix, mask_mov, disp_hr


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
    movs = list(imgs_moving) if isinstance(imgs_moving, (list, tuple)) else [imgs_moving]
    if not movs:
        raise ValueError("imgs_moving is empty")
    shape = _volume(img_fixed, "img_fixed")
    for i, mv in enumerate(movs):
        if _volume(mv, "imgs_moving[%d]" % i) != shape:
            raise ValueError("imgs_moving[%d] has extent %s, the fixed image %s" % (i, _volume(mv, "imgs_moving[%d]" % i), shape))
    try:
        g, hw, it, lts, nr = int(grid_sp), int(disp_hw), int(ic_iters), int(lts_iters), int(rounds)
        thr = float(mask_thresh)
    except (TypeError, ValueError):
        raise ValueError("grid_sp, disp_hw, ic_iters, lts_iters, rounds must be ints and mask_thresh a number") from None
    if not 1 <= g <= 64 or min(shape) < 2 * g or hw < 0 or it < 0 or lts < 1 or nr < 1:
        raise ValueError("need 1 <= grid_sp <= 64 with at least two cells per axis of %s, disp_hw >= 0, ic_iters >= 0, lts_iters >= 1, rounds >= 1; "
                         "got %r, %r, %r, %r, %r" % (shape, grid_sp, disp_hw, ic_iters, lts_iters, rounds))
    if (seg_fixed is None) != (seg_moving is None):
        raise ValueError("seg_fixed and seg_moving go together")
    if seg_fixed is not None and (_volume(seg_fixed, "seg_fixed") != shape or _volume(seg_moving, "seg_moving") != shape):
        raise ValueError("seg_fixed and seg_moving must have the images' extent %s" % (shape,))
    fix = f32c(require_device_tensor(img_fixed, "img_fixed")).reshape(shape)
    movs = [f32c(require_device_tensor(mv, "imgs_moving[%d]" % i)).reshape(shape) for i, mv in enumerate(movs)]
    want_field = bool(return_field) or seg_fixed is not None
    T, mask_fix, mask_mov, disp_hr = _round(fix, movs, mind_r, mind_d, g, hw, thr, it, lts, shape, want_field, mask_thresh)
    for _ in range(1, nr):
        warped = [affine_warp(mv[None], T)[0] for mv in movs]
        Tr = _round(fix, warped, mind_r, mind_d, g, hw, thr, it, lts, shape, False, mask_thresh)[0]
        T = (T.double() @ Tr.double()).float()
    res = AffineRegistration(T, mask_fix, mask_mov, disp_hr if want_field else None)
    if seg_fixed is not None:
        from .convexAdam_hyper_util import warp_labels_nearest
        sf = f32c(require_device_tensor(seg_fixed, "seg_fixed")).reshape(shape)
        sm = f32c(require_device_tensor(seg_moving, "seg_moving")).reshape(shape)
        ml = int(sm.max())
        if not 1 <= ml < 1024:
            raise ValueError("seg_moving must hold labels 1..1023, its maximum is %d" % ml)
        res.tre_before = landmark_tre(sf, sm, ml)
        res.tre_deformable = landmark_tre(sf, warp_labels_nearest(sm, disp_hr), ml)
        res.tre_affine = landmark_tre(sf, affine_warp(sm[None], T, mode="nearest")[0], ml)
    return res


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
    from . import convex_adam_utils  # noqa: F401  (first: fieldops imports it, and it imports fieldops)
    from .fieldops import _f64, _operand
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
        u, cs, vs = None, 0, 0
        out = torch.empty((H, W, D, 3), dtype=torch.float64, device=dev)
        ocs, ovs = 1, 3
    else:
        u, ushape, cs, vs, _ = _operand(field, "field", dev)
        if ushape != (H, W, D) or u.device != dev:
            raise ValueError("affine_to_field: field is %s on %s, shape %s and T on %s" % (ushape, u.device, (H, W, D), dev))
        out = torch.empty(u.shape, dtype=torch.float64, device=dev)
        ocs, ovs = cs, vs
    with torch.cuda.device(dev):
        check(_affine.lib().cvx_affine_field_f64(ptr(th), H, W, D, ptr(u), _f64(u) if u is not None else 0, cs, vs, ptr(out), 1, ocs, ovs,
                                                 stream_ptr(dev)))
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
