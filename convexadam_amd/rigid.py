"""Least-trimmed rigid fit and fused affine warp (convex_adam_utils.py:173-193; l2r_2020_convexAdam_CuRIOUS.py:349-390).

`find_rigid_3d` and `least_trimmed_rigid` keep the reference's names, positional signatures and (4, 4) float32 results; the whole fit --
every trimming iteration -- is one launch of csrc/rigid.hip.  `affine_warp` is F.grid_sample(vol, F.affine_grid(theta, ...)) with the
grid computed in the kernel.  `rigid_from_field` is the CuRIOUS script's rigid step after its convex stage.
"""
import ctypes as C

import torch

from ._lib import _shape, call, f32c, ptr, require_device_tensor, scratch

_MODES = {"bilinear": 0, "nearest": 1}


def _point_pair(a, b, names, min_n, exact_cols=None):
    """N of two point sets of one length, from the metadata only: (N, exact_cols), or (N, k >= 3), and N >= min_n"""
    want = "(N, %d)" % exact_cols if exact_cols else "(N, k) with k >= 3"
    n = []
    for t, name in zip((a, b), names):
        s = _shape(t, name)
        if len(s) != 2 or s[0] < min_n or (s[1] != exact_cols if exact_cols else s[1] < 3):
            raise ValueError("%s must be %s and N >= %d, got %s" % (name, want, min_n, s))
        n.append(s[0])
    if n[0] != n[1]:
        raise ValueError("%s and %s must have the same number of points, got %d and %d" % (names + tuple(n)))
    return n[0]


def _fit(entry, fixed, moving, want_inliers, *model_args):
    """One launch of <entry>_f32 (cvx_rigid_lts, cvx_affine_lts) -> X (4, 4) float32[, the (N,) bool inlier mask]; model_args:
    what the entry point takes between n and X (iters; the affine one also `normal`)"""
    f = f32c(require_device_tensor(fixed, "fixed"))
    m = f32c(require_device_tensor(moving, "moving"))
    if m.device != f.device:
        raise ValueError("both point sets must live on one device (%s, %s)" % (f.device, m.device))
    n = int(f.shape[0])
    X = torch.empty((4, 4), dtype=torch.float32, device=f.device)
    mask = torch.empty(n, dtype=torch.uint8, device=f.device) if want_inliers else None
    call(f.device, entry + "_f32", ptr(f), int(f.shape[1]), ptr(m), int(m.shape[1]), n, *model_args, ptr(X), ptr(mask),
         *scratch(f.device, entry + "_workspace_bytes", n))
    return (X, mask.bool()) if want_inliers else X


def _trimmed_iters(iter):
    if int(iter) < 1:
        raise ValueError("iter must be >= 1, got %r" % (iter,))
    return int(iter)


def find_rigid_3d(x, y):
    """(4, 4) T = [R t; 0 0 0 1] with y[:, :3] ~ x[:, :3] R^T + t, R the optimal proper rotation (convex_adam_utils.py:173-184).
    x, y: (N, k >= 3) device tensors, N >= 2.  Raises CvxError on a non-finite coordinate (the reference's torch.svd raises too)."""
    _point_pair(x, y, ("x", "y"), 2)
    return _fit("cvx_rigid_lts", x, y, False, 1)


def least_trimmed_rigid(fixed_pts, moving_pts, iter=5, return_inliers=False):
    """least_trimmed_rigid of convex_adam_utils.py:187-193: `iter` rigid fits, the first on all N points, each later one on the N // 2
    points with the smallest residuals ||moving - fixed T^T|| under the previous fit (ties: lowest index first).  fixed_pts, moving_pts:
    (N, 4) device tensors (homogeneous points).  Returns T (4, 4) float32, and with return_inliers=True also the (N,) bool mask of the
    points the returned fit used."""
    _point_pair(fixed_pts, moving_pts, ("fixed_pts", "moving_pts"), 2, 4)
    return _fit("cvx_rigid_lts", fixed_pts, moving_pts, bool(return_inliers), _trimmed_iters(iter))


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
    call(a.device, "cvx_affine_warp_f32", ptr(a), Cn, h, w, d, ptr(th), ho, wo, do_, _MODES[mode], ptr(out))
    return out.unsqueeze(0) if len(vs) == 5 else out


def _volume(t, name):
    """(H, W, D) of a volume given as (H, W, D) or with leading 1s, from the metadata only."""
    s = _shape(t, name)
    if len(s) < 3 or any(n != 1 for n in s[:-3]) or min(s[-3:]) < 1:
        raise ValueError("%s must be (H, W, D) (optionally with leading 1s), got %s" % (name, s))
    return s[-3:]


def threshold_pool_mask(img, thresh, grid_sp):
    """F.avg_pool3d((img > thresh).float(), grid_sp, stride=grid_sp) > .5 (CuRIOUS:328,330) in one kernel: img (H, W, D) (optionally with
    leading 1s) -> bool (H // grid_sp, W // grid_sp, D // grid_sp); remainder voxels are ignored, a NaN voxel counts as below."""
    H, W, D = _volume(img, "img")
    try:
        g = int(grid_sp)
        t = float(thresh)
    except (TypeError, ValueError):
        raise ValueError("thresh must be a number and grid_sp an int, got %r, %r" % (thresh, grid_sp)) from None
    if not 1 <= g <= 64 or min(H, W, D) < g:
        raise ValueError("grid_sp = %r must lie in 1..64 and fit the extent %s" % (grid_sp, (H, W, D)))
    a = f32c(require_device_tensor(img, "img"))
    out = torch.empty((H // g, W // g, D // g), dtype=torch.uint8, device=a.device)
    call(a.device, "cvx_threshold_pool_mask_u8", ptr(a), H, W, D, t, g, ptr(out))
    return out.view(torch.bool)


def _max_label(max_label):
    try:
        m = int(max_label)
    except (TypeError, ValueError):
        raise ValueError("max_label must be an int, got %r" % (max_label,)) from None
    if not 0 <= m < 1024:
        raise ValueError("max_label must lie in 0..1023, got %r" % (max_label,))
    return m


def label_centroids(seg, max_label, return_counts=False):
    """Centroid of every label 0..max_label of a label volume seg (H, W, D) (float- or integer-valued, optionally with leading 1s), in
    voxel indices along (H, W, D): `mesh[:, idx].mean(1)` of CuRIOUS:312-316 from exact integer sums (one kernel; the division runs on
    the host in float64).  Returns a (max_label + 1, 3) float64 CPU tensor; a label absent from the volume has a NaN centroid, like the
    script's empty mean.  return_counts=True: also the (max_label + 1,) int64 voxel counts."""
    H, W, D = _volume(seg, "seg")
    m = _max_label(max_label)
    a = f32c(require_device_tensor(seg, "seg"))
    acc = torch.empty((m + 1, 4), dtype=torch.int64, device=a.device)
    call(a.device, "cvx_label_centroids_i64", ptr(a), H, W, D, m, ptr(acc))
    acc = acc.cpu()
    counts = acc[:, 0]
    cent = acc[:, 1:].to(torch.float64) / counts.to(torch.float64).unsqueeze(1)        # 0 / 0 = NaN for an absent label
    return (cent, counts) if return_counts else cent


def landmark_tre(seg_a, seg_b, max_label=None):
    """The CuRIOUS script's target registration error (:312-319): per label 1..max_label the distance sqrt(sum((a - b)^2)) between the
    label's centroids in the two landmark volumes, in voxels, as a (max_label,) float64 CPU tensor (its mean is the script's score).
    max_label=None takes int(seg_b.max()), as the script takes its moving landmarks' maximum.  A label absent from either volume has a
    NaN entry."""
    sa, sb = _volume(seg_a, "seg_a"), _volume(seg_b, "seg_b")
    if sa != sb:
        raise ValueError("seg_a and seg_b must have the same extent, got %s and %s" % (sa, sb))
    if max_label is not None:
        m = _max_label(max_label)
    require_device_tensor(seg_a, "seg_a")
    require_device_tensor(seg_b, "seg_b")
    if max_label is None:
        m = _max_label(int(seg_b.max()))
    ca, cb = label_centroids(seg_a, m), label_centroids(seg_b, m)
    return (ca[1:] - cb[1:]).pow(2).sum(1).sqrt()


def _coarse_mask(mask, name, hwd):
    if mask is None:
        return None
    ms = _shape(mask, name)
    if len(ms) < 3 or ms[-3:] != hwd or any(s != 1 for s in ms[:-3]):
        raise ValueError("%s must be %s (optionally with leading 1s), got %s" % (name, hwd, ms))
    return mask


def convex_stage(feat_fix, feat_mov, grid_sp, disp_hw, shape, mask_fix=None, mask_mov=None, ic_iters=0, full_res=True):
    """The convex stage of CuRIOUS:335-357 in one library call: correlate -> coupled convex on the masked cost volume (forward volume
    masked by mask_fix; with ic_iters > 0 also the reverse one, masked by mask_mov, and that many inverse-consistency steps with the
    script's scale and flips) -> trilinear up-sampling to `shape`.  The cost volume is never multiplied by a mask and never copied.

    feat_fix, feat_mov  (1, C, h, w, d) or (C, h, w, d) coarse features, (h, w, d) = shape // grid_sp
    mask_fix, mask_mov  (h, w, d) (optionally with leading 1s), non-zero = keep the cell; None keeps every cell
    Returns (coarse_field, disp_hr): coarse_field (1, 3, h, w, d) = disp_soft (ic_iters 0, coarse voxels) or disp_ice.flip(1) * scale *
    grid_sp (voxels); disp_hr (1, 3, H, W, D) in voxels, or None with full_res=False.  float32 in the reference's evaluation order."""
    from ._lib import StageParams
    try:
        H, W, D = [int(s) for s in shape]
        g, hw, it = int(grid_sp), int(disp_hw), int(ic_iters)
    except (TypeError, ValueError):
        raise ValueError("shape must be three ints and grid_sp, disp_hw, ic_iters ints, got %r, %r, %r, %r" % (shape, grid_sp, disp_hw, ic_iters)) from None
    if g < 1 or hw < 0 or it < 0 or min(H, W, D) < g:
        raise ValueError("grid_sp >= 1, disp_hw >= 0, ic_iters >= 0 and shape >= grid_sp expected, got %r, %r, %r, %r" % (grid_sp, disp_hw, ic_iters, shape))
    hwd = (H // g, W // g, D // g)
    sf, sm = _shape(feat_fix, "feat_fix"), _shape(feat_mov, "feat_mov")
    if len(sf) == 5 and sf[0] == 1:
        sf = sf[1:]
    if len(sm) == 5 and sm[0] == 1:
        sm = sm[1:]
    if len(sf) != 4 or sf[0] < 1 or sf[1:] != hwd or sm != sf:
        raise ValueError("feat_fix and feat_mov must both be (1, C, %d, %d, %d), got %s and %s" % (hwd + (_shape(feat_fix, "feat_fix"), _shape(feat_mov, "feat_mov"))))
    if (2 * hw + 1) ** 3 * hwd[0] * hwd[1] * hwd[2] >= 2e9:
        raise ValueError("cost volume of (2 * %d + 1)^3 x %s entries is too large" % (hw, hwd))
    _coarse_mask(mask_fix, "mask_fix", hwd)
    _coarse_mask(mask_mov, "mask_mov", hwd)
    f = f32c(require_device_tensor(feat_fix, "feat_fix"))
    m = f32c(require_device_tensor(feat_mov, "feat_mov"))
    if m.device != f.device:
        raise ValueError("feat_fix and feat_mov must live on one device (%s, %s)" % (f.device, m.device))
    dev = f.device
    mf = None if mask_fix is None else (mask_fix.to(dev) != 0).to(torch.uint8).contiguous()
    mm = None if mask_mov is None else (mask_mov.to(dev) != 0).to(torch.uint8).contiguous()
    p = StageParams(sf[0], hwd[0], hwd[1], hwd[2], hw, g, it, H, W, D)
    coarse = torch.empty((1, 3) + hwd, dtype=torch.float32, device=dev)
    hr = torch.empty((1, 3, H, W, D), dtype=torch.float32, device=dev) if full_res else None
    call(dev, "cvx_convex_stage_f32", ptr(f), ptr(m), ptr(mf), ptr(mm), C.byref(p), ptr(coarse), ptr(hr),
         *scratch(dev, "cvx_convex_stage_workspace_bytes", C.byref(p), required=True))
    return coarse, hr


def rigid_samples(coarse_field, mask_coarse, grid_sp, shape):
    """T1, T2 of CuRIOUS:359-365 as (M, 4) float32 -- the rows _field_samples takes from a full-resolution field -- computed straight
    from the COARSE field of the convex stage: bit-identical to _field_samples(resize_trilinear(coarse_field, shape), mask_coarse,
    grid_sp) without forming that field or the coordinate volumes (one kernel; the number of kept cells reaches the host once).

    coarse_field (1, 3, h, w, d) or (3, h, w, d) device tensor in voxels, (h, w, d) = shape // grid_sp (convex_stage with ic_iters > 0;
                 with ic_iters = 0 its disp_soft times grid_sp)
    mask_coarse  (h, w, d) tensor (optionally with leading 1s), non-zero = use the cell"""
    try:
        H, W, D = [int(s) for s in shape]
        g = int(grid_sp)
    except (TypeError, ValueError):
        raise ValueError("shape must be three ints and grid_sp an int, got %r, %r" % (shape, grid_sp)) from None
    if g < 1 or min(H // g, W // g, D // g) < 1 or min(H, W, D) < 2:
        raise ValueError("grid_sp = %r does not fit the field extent %s" % (grid_sp, (H, W, D)))
    hwd = (H // g, W // g, D // g)
    cs = _shape(coarse_field, "coarse_field")
    if len(cs) == 5 and cs[0] == 1:
        cs = cs[1:]
    if cs != (3,) + hwd:
        raise ValueError("coarse_field must be (1, 3, %d, %d, %d), got %s" % (hwd + (_shape(coarse_field, "coarse_field"),)))
    _coarse_mask(mask_coarse, "mask_coarse", hwd)
    c = f32c(require_device_tensor(coarse_field, "coarse_field"))
    dev = c.device
    m = (mask_coarse.to(dev) != 0).to(torch.uint8).contiguous()
    v = hwd[0] * hwd[1] * hwd[2]
    T1 = torch.empty((v, 4), dtype=torch.float32, device=dev)
    T2 = torch.empty((v, 4), dtype=torch.float32, device=dev)
    count = C.c_int64(0)
    call(dev, "cvx_rigid_samples_f32", ptr(c), ptr(m), hwd[0], hwd[1], hwd[2], H, W, D, ptr(T1), ptr(T2), C.byref(count),
         *scratch(dev, "cvx_rigid_samples_workspace_bytes", hwd[0], hwd[1], hwd[2], H, W, D))
    M = int(count.value)
    if M < 2:
        raise ValueError("mask_coarse selects %d cells; the fit needs at least 2" % M)
    return T1[:M], T2[:M]


# convex_adam_rigid and convex_adam_affine take the rows of their fit from the coarse field (rigid_samples); False = from the up-sampled field (_field_samples),
# the same bits -- kept as a switch so that tools/time_rigidreg.py can time both in one process
SAMPLE_FROM_COARSE = True


class RigidRegistration:
    """Result of convex_adam_rigid: T (4, 4) float32 on the device; mask_fix, mask_mov (h, w, d) bool; disp_hr (1, 3, H, W, D) voxels
    (return_field=True or label volumes given, else None); tre_before, tre_deformable, tre_rigid: per-label float64 CPU tensors of
    landmark_tre (label volumes given, else None) -- their means are the three figures the script prints."""

    def __init__(self, T, mask_fix, mask_mov, disp_hr=None, tre_before=None, tre_deformable=None, tre_rigid=None):
        self.T, self.mask_fix, self.mask_mov, self.disp_hr = T, mask_fix, mask_mov, disp_hr
        self.tre_before, self.tre_deformable, self.tre_rigid = tre_before, tre_deformable, tre_rigid


def convex_adam_rigid(img_fixed, imgs_moving, mind_r=3, mind_d=3, grid_sp=6, disp_hw=6, mask_thresh=10., ic_iters=5, lts_iters=15,
                      seg_fixed=None, seg_moving=None, return_field=False):
    """Rigid registration of the CuRIOUS script (l2r_2020_convexAdam_CuRIOUS.py:321-391): MIND-SSC features pooled to the coarse grid,
    the convex stage on cost volumes masked by coarse foreground masks, and a least-trimmed rigid fit to the displaced coarse cells.

    img_fixed    (H, W, D) device tensor (optionally with leading 1s)
    imgs_moving  one such volume or a list of them -- several modalities of the moving subject on one grid (the script: T1, FLAIR);
                 their descriptors are concatenated and the fixed descriptor is repeated once per moving image (:326-327)
    mask_thresh  foreground = voxels above it; cells more than half foreground are kept (threshold_pool_mask) -- the fixed image's
                 cells mask the forward cost volume and select the points of the fit, the FIRST moving image's the reverse volume
    seg_fixed, seg_moving  landmark label volumes: the script's target registration error before, after the deformable field and
                 after the rigid transform (landmark_tre; labels 1..int(seg_moving.max()))
    Returns a RigidRegistration.  T approximates the INVERSE of a matrix A that built the moving image as F.grid_sample(fixed,
    F.affine_grid(A)) (pull-back convention): F.affine_grid(T[:3]) / affine_warp(moving, T) bring the moving image onto the fixed one.
    The search works on whole coarse cells: a motion below about half a cell (2-3 voxels at grid_sp 6) returns an all-zero coarse
    field and the identity; motions beyond grid_sp * disp_hw voxels are out of reach."""
    return _register(least_trimmed_rigid, 2, "rigid", RigidRegistration, "tre_rigid", img_fixed, imgs_moving, mind_r, mind_d, grid_sp, disp_hw,
                     mask_thresh, ic_iters, lts_iters, seg_fixed, seg_moving, return_field)


_NO_ROUNDS = object()


def _register(fit, min_cells, model, result, tre_name, img_fixed, imgs_moving, mind_r, mind_d, grid_sp, disp_hw, mask_thresh, ic_iters,
              lts_iters, seg_fixed, seg_moving, return_field, rounds=_NO_ROUNDS):
    """convex_adam_rigid and convex_adam_affine: features, masks, the convex stage, the rows of the fit, `fit(T1, T2, lts_iters)` on at
    least `min_cells` coarse cells, and the three landmark errors, the third as `result.<tre_name>`.  `model` is the fit's word in the
    messages.  rounds: _NO_ROUNDS for a model without that argument (one round, and no message names it); else the stage and the fit run
    again on the moving images warped with the current T, and the matrices are multiplied in float64 on the device (T <- T T_round)."""
    from .convex_adam_utils import mind_pooled
    movs = list(imgs_moving) if isinstance(imgs_moving, (list, tuple)) else [imgs_moving]
    if not movs:
        raise ValueError("imgs_moving is empty")
    shape = _volume(img_fixed, "img_fixed")
    for i, mv in enumerate(movs):
        if _volume(mv, "imgs_moving[%d]" % i) != shape:
            raise ValueError("imgs_moving[%d] has extent %s, the fixed image %s" % (i, _volume(mv, "imgs_moving[%d]" % i), shape))
    given = (grid_sp, disp_hw, ic_iters, lts_iters) + (() if rounds is _NO_ROUNDS else (rounds,))
    try:
        g, hw, it, lts = int(grid_sp), int(disp_hw), int(ic_iters), int(lts_iters)
        nr = 1 if rounds is _NO_ROUNDS else int(rounds)
        thr = float(mask_thresh)
    except (TypeError, ValueError):
        raise ValueError("grid_sp, disp_hw, ic_iters, lts_iters%s must be ints and mask_thresh a number"
                         % ("" if rounds is _NO_ROUNDS else ", rounds")) from None
    if not 1 <= g <= 64 or min(shape) < 2 * g or hw < 0 or it < 0 or lts < 1 or nr < 1:
        raise ValueError("need 1 <= grid_sp <= 64 with at least two cells per axis of %s, disp_hw >= 0, ic_iters >= 0, lts_iters >= 1%s; got %s"
                         % (shape, "" if rounds is _NO_ROUNDS else ", rounds >= 1", ", ".join(repr(v) for v in given)))
    if (seg_fixed is None) != (seg_moving is None):
        raise ValueError("seg_fixed and seg_moving go together")
    if seg_fixed is not None and (_volume(seg_fixed, "seg_fixed") != shape or _volume(seg_moving, "seg_moving") != shape):
        raise ValueError("seg_fixed and seg_moving must have the images' extent %s" % (shape,))
    fix = f32c(require_device_tensor(img_fixed, "img_fixed")).reshape(shape)
    movs = [f32c(require_device_tensor(mv, "imgs_moving[%d]" % i)).reshape(shape) for i, mv in enumerate(movs)]
    dev = fix.device

    def one_round(movs, want_field):
        """one masked convex stage and one trimmed fit -> (T, mask_fix, mask_mov, disp_hr)"""
        ff = mind_pooled(fix[None, None], mind_r, mind_d, g, device=dev)
        feat_fix = torch.cat([ff] * len(movs), 1) if len(movs) > 1 else ff
        feat_mov = torch.cat([mind_pooled(mv[None, None], mind_r, mind_d, g, device=dev) for mv in movs], 1)
        mask_fix, mask_mov = threshold_pool_mask(fix, thr, g), threshold_pool_mask(movs[0], thr, g)
        kept = int(mask_fix.sum())
        if kept < min_cells:
            raise ValueError("mask_thresh = %r keeps %d coarse cells of the fixed image; the %s fit needs at least %d"
                             % (mask_thresh, kept, model, min_cells))
        coarse, disp_hr = convex_stage(feat_fix, feat_mov, g, hw, shape, mask_fix, mask_mov, it, full_res=want_field or not SAMPLE_FROM_COARSE)
        if SAMPLE_FROM_COARSE:                  # same rows, bit for bit; a call without the field never forms it at full resolution
            T1, T2 = rigid_samples(coarse if it > 0 else coarse * g, mask_fix, g, shape)
        else:
            T1, T2 = _field_samples(disp_hr, mask_fix, g)
        return fit(T1, T2, lts), mask_fix, mask_mov, disp_hr

    want_field = bool(return_field) or seg_fixed is not None
    T, mask_fix, mask_mov, disp_hr = one_round(movs, want_field)
    for _ in range(1, nr):
        Tr = one_round([affine_warp(mv[None], T)[0] for mv in movs], False)[0]
        T = (T.double() @ Tr.double()).float()
    res = result(T, mask_fix, mask_mov, disp_hr if want_field else None)
    if seg_fixed is not None:
        from .convexAdam_hyper_util import warp_labels_nearest
        sf = f32c(require_device_tensor(seg_fixed, "seg_fixed")).reshape(shape)
        sm = f32c(require_device_tensor(seg_moving, "seg_moving")).reshape(shape)
        ml = int(sm.max())
        if not 1 <= ml < 1024:
            raise ValueError("seg_moving must hold labels 1..1023, its maximum is %d" % ml)
        res.tre_before = landmark_tre(sf, sm, ml)                                                          # (:312-319)
        res.tre_deformable = landmark_tre(sf, warp_labels_nearest(sm, disp_hr), ml)                       # (:376-382)
        setattr(res, tre_name, landmark_tre(sf, affine_warp(sm[None], T, mode="nearest")[0], ml))         # (:385-391)
    return res


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
        call(dev, "cvx_grid_sample_f32", ptr(v), 3, H, W, D, ptr(pts), M, 1, 1, ptr(s))
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
