"""Operator-level mirror of the reference's `convexAdam.convex_adam_utils` (src/convexAdam/
convex_adam_utils.py) on top of libconvexadam_hip.so.

Same names, argument meaning and return formats as the reference:
    MINDSSC             convex_adam_utils.py:24-68
    correlate           convex_adam_utils.py:72-89
    coupled_convex      convex_adam_utils.py:93-109
    inverse_consistency convex_adam_utils.py:114-129
    combineDeformation3d convex_adam_utils.py:133-135
    validate_image      convex_adam_utils.py:268-279
    pdist_squared, nnUNetNorm, nnUNetNormProps, nnUNetCTnorm, compute_steps_for_sliding_window, get_gaussian,
    create_nonzero_mask, get_bbox_from_mask, crop_to_bbox        convex_adam_utils.py:15-21, 142-170, 196-265   (prep.py)
Tensors must live on the HIP device (torch device type 'cuda'); the kernels compute in float32 and
results are cast back to the dtype the reference would return.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import CorrOpts, call, check, f32c, lib, ptr, require_device_tensor, scratch


# ---- table helpers (host, exact restatements of torch.linspace / affine_grid) ----------------------
def affine_base(S: int) -> np.ndarray:
    """Identity coordinate of F.affine_grid(eye, ..., align_corners=False) along an axis of size S."""
    out = np.empty(int(S), np.float32)
    lib().cvx_affine_base_host(int(S), out.ctypes.data_as(C.c_void_p))
    return out


def disp_mesh(disp_hw: int) -> np.ndarray:
    """(3, n^3) search mesh: what convex_adam_MIND.py:127 builds with affine_grid(align_corners=True)."""
    n = 2 * int(disp_hw) + 1
    out = np.empty((3, n ** 3), np.float32)
    lib().cvx_disp_mesh_host(int(disp_hw), out.ctypes.data_as(C.c_void_p))
    return out


def disp_mesh_t(disp_hw: int, device, dtype=torch.float32) -> torch.Tensor:
    """(3, n^3, 1) tensor, the `disp_mesh_t` argument of coupled_convex()."""
    return torch.from_numpy(disp_mesh(disp_hw)).to(device=device, dtype=dtype).unsqueeze(-1)


def _base_tables(h, w, d, device):
    return [torch.from_numpy(affine_base(s)).to(device) for s in (h, w, d)]


# ---- reference operators ---------------------------------------------------------------------------
def MINDSSC(img, radius=2, dilation=2, device='cuda'):
    """MIND-SSC descriptor: img (1,1,H,W,D) -> (1,12,H,W,D) in img's dtype.  (convex_adam_utils.py:24-68)"""
    img = require_device_tensor(img.to(device), "img")
    if img.dim() != 5 or img.shape[0] != 1 or img.shape[1] != 1:
        raise ValueError("MINDSSC expects a (1,1,H,W,D) tensor, got %s" % (tuple(img.shape),))
    H, W, D = [int(s) for s in img.shape[2:]]
    x = f32c(img)
    out = torch.empty((1, 12, H, W, D), dtype=torch.float32, device=x.device)
    call(x.device, "cvx_mindssc_f32", ptr(x), H, W, D, int(radius), int(dilation), ptr(out),
         *scratch(x.device, "cvx_mindssc_workspace_bytes", H, W, D, int(radius), int(dilation)))
    return out if img.dtype == torch.float32 else out.to(img.dtype)


def mind_pooled(img, radius, dilation, g1, g2=0, device='cuda', return_repairs=False):
    """F.avg_pool3d(MINDSSC(img, radius, dilation), g, stride=g) for g = g1 (and g2 > 0) without the full-resolution descriptor: what
    convex_adam_pt consumes (convex_adam_MIND.py:118-119, 149-150).  img (1,1,H,W,D) -> (1,12,H/g1,W/g1,D/g1) [, (1,12,H/g2,W/g2,D/g2)].
    return_repairs: also the number of blocks whose pooled cells were recomputed with the clamped variance (single-pass path)."""
    img = require_device_tensor(img.to(device), "img")
    if img.dim() != 5 or img.shape[0] != 1 or img.shape[1] != 1:
        raise ValueError("mind_pooled expects a (1,1,H,W,D) tensor, got %s" % (tuple(img.shape),))
    H, W, D = [int(s) for s in img.shape[2:]]
    x = f32c(img)
    g1, g2 = int(g1), int(g2)
    o1 = torch.empty((1, 12, H // g1, W // g1, D // g1), dtype=torch.float32, device=x.device)
    o2 = torch.empty((1, 12, H // g2, W // g2, D // g2), dtype=torch.float32, device=x.device) if g2 > 0 else None
    nsc = lib().cvx_mindssc_pooled_scratch_bytes(H, W, D, int(radius), int(dilation), g1, g2)     # a second buffer beside the workspace: the call's own
    if x.data_ptr() % 16:                      # (torch allocations are 256-byte aligned; a view may not be)
        x = x.clone()
    sc = torch.empty(max(nsc, 16), dtype=torch.uint8, device=x.device)
    rep = C.c_int(0)
    call(x.device, "cvx_mindssc_pooled_f32", ptr(x), H, W, D, int(radius), int(dilation), g1, ptr(o1), g2, ptr(o2) if o2 is not None else None,
         ptr(sc) if nsc else None, nsc, *scratch(x.device, "cvx_mindssc_workspace_bytes", H, W, D, int(radius), int(dilation)),
         C.byref(rep) if return_repairs else None)
    outs = (o1,) if o2 is None else (o1, o2)
    outs = tuple(o if img.dtype == torch.float32 else o.to(img.dtype) for o in outs)
    if return_repairs:
        return outs + (int(rep.value),)
    return outs if o2 is not None else outs[0]


def avg_pool(features, g):
    """F.avg_pool3d(features, g, stride=g) for a (1,C,H,W,D) device tensor.  (convex_adam_MIND.py:118-119)"""
    features = require_device_tensor(features, "features")
    _, Cn, H, W, D = [int(s) for s in features.shape]
    x = f32c(features)
    out = torch.empty((1, Cn, H // g, W // g, D // g), dtype=torch.float32, device=x.device)
    call(x.device, "cvx_avgpool_f32", ptr(x), Cn, H, W, D, int(g), ptr(out))
    return out if features.dtype == torch.float32 else out.to(features.dtype)


def correlate(mind_fix, mind_mov, disp_hw, grid_sp, shape, ch=12, cost="ssd", n_box=2, mode="exact", storage="fp32"):
    """SSD cost volume + argmin.  (convex_adam_utils.py:72-89)
    mind_fix/mind_mov (1,C,H',W',D') -> ssd (n^3,H',W',D') in the feature dtype, argmin (H',W',D') int64.
    Beyond the packaged operator: cost="sad" and n_box=1 are the variants of the challenge scripts
    (l2r_2021_convexAdam_task3_docker.py:54,56; task2:60); mode="fast" evaluates the same sums with fused multiply-adds and
    separable box filters (last-bit differences, not bit-compatible with the reference; SSD with two boxes only);
    storage="fp16" returns the cost volume as a torch.float16 tensor written by the kernel itself (float32 accumulation, one rounding
    on the way out: the reference's GPU default dtype, convex_adam_MIND.py:79,89-91) and the argmin of the stored values."""
    mind_fix = require_device_tensor(mind_fix, "mind_fix")
    mind_mov = require_device_tensor(mind_mov, "mind_mov")
    H, W, D = int(shape[0]), int(shape[1]), int(shape[2])
    h, w, d = H // grid_sp, W // grid_sp, D // grid_sp
    if tuple(mind_fix.shape) != (1, ch, h, w, d) or tuple(mind_mov.shape) != (1, ch, h, w, d):
        raise ValueError("correlate: features %s / %s do not match (1,%d,%d,%d,%d)" %
                         (tuple(mind_fix.shape), tuple(mind_mov.shape), ch, h, w, d))
    n = 2 * int(disp_hw) + 1
    f, m = f32c(mind_fix), f32c(mind_mov)
    if storage not in ("fp32", "fp16"):
        raise ValueError("correlate: storage must be 'fp32' or 'fp16'")
    half = storage == "fp16"
    ssd = torch.empty((n ** 3, h, w, d), dtype=torch.float16 if half else torch.float32, device=f.device)
    am = torch.empty((h, w, d), dtype=torch.int64, device=f.device)
    ws = scratch(f.device, "cvx_correlate_workspace_bytes", ch, h, w, d, int(disp_hw))
    if cost not in ("ssd", "sad") or n_box not in (1, 2) or mode not in ("exact", "fast", "certified"):
        raise ValueError("correlate: cost must be 'ssd' or 'sad', n_box 1 or 2, mode 'exact', 'fast' or 'certified'")
    # mode="certified": the pipeline's internal arithmetic (cvx_corr_opts.fast = 2) -- `ssd` holds the UNSCALED sums (729 x the mean to
    # within 2^-16 relative) and `argmin` is nevertheless the reference's argmin of the EXACT volume (certified, resolved exactly where needed)
    opts = CorrOpts(1 if cost == "sad" else 0, int(n_box), {"exact": 0, "fast": 1, "certified": 2}[mode], 2 if half else 0)
    call(f.device, "cvx_correlate_ex_f32", ptr(f), ptr(m), ch, h, w, d, int(disp_hw), C.byref(opts), ptr(ssd), ptr(am), *ws)
    if mind_fix.dtype != torch.float32 and not half:
        ssd = ssd.to(mind_fix.dtype)
    return ssd, am


def coupled_convex(ssd, ssd_argmin, disp_mesh_t, grid_sp, shape, cell_mask=None):
    """Coupled convex regularisation -> (1,3,H',W',D') in coarse-voxel units.  (convex_adam_utils.py:93-109)
    cell_mask (H',W',D') (optionally with leading 1s; non-zero = keep): the result on ssd * cell_mask, the cost-volume masking of
    l2r_2020_convexAdam_CuRIOUS.py:336-338, without writing `ssd` (float32 volumes only).  `ssd_argmin` stays the argmin of the unmasked
    volume, as in the script.  Columns of masked-out cells are not read: a NaN there does not reach the result."""
    H, W, D = int(shape[0]), int(shape[1]), int(shape[2])
    h, w, d = H // grid_sp, W // grid_sp, D // grid_sp
    if cell_mask is not None:                               # metadata only: a bad mask is a ValueError for CPU tensors too
        if not isinstance(cell_mask, torch.Tensor):
            raise TypeError("cell_mask must be a torch.Tensor")
        ms = tuple(int(s) for s in cell_mask.shape)
        if len(ms) < 3 or ms[-3:] != (h, w, d) or any(s != 1 for s in ms[:-3]):
            raise ValueError("coupled_convex: cell_mask must be (%d, %d, %d) (optionally with leading 1s), got %s" % (h, w, d, ms))
        if isinstance(ssd, torch.Tensor) and ssd.dtype == torch.float16:
            raise ValueError("coupled_convex: cell_mask needs a float32 cost volume (fp16 storage of the masked path is not built)")
    ssd = require_device_tensor(ssd, "ssd")
    K = int(ssd.shape[0])
    n = int(round(K ** (1.0 / 3.0)))
    if n ** 3 != K or tuple(ssd.shape[1:]) != (h, w, d):
        raise ValueError("coupled_convex: ssd shape %s does not match (n^3,%d,%d,%d)" % (tuple(ssd.shape), h, w, d))
    half = ssd.dtype == torch.float16                       # fp16 storage: the passes read the half-precision volume as it is
    s = ssd.detach().contiguous() if half else f32c(ssd)
    am = ssd_argmin.to(device=s.device, dtype=torch.int64).contiguous()
    mesh = f32c(disp_mesh_t.to(s.device)).reshape(3, K)
    out = torch.empty((1, 3, h, w, d), dtype=torch.float32, device=s.device)
    ws = scratch(s.device, "cvx_coupled_convex_workspace_bytes", h, w, d, (n - 1) // 2)
    if cell_mask is not None:
        cm = (cell_mask.to(s.device) != 0).to(torch.uint8).reshape(h, w, d).contiguous()
        call(s.device, "cvx_coupled_convex_masked_f32", ptr(s), ptr(am), ptr(mesh), ptr(cm), h, w, d, (n - 1) // 2, ptr(out), *ws)
    else:
        call(s.device, "cvx_coupled_convex_f16" if half else "cvx_coupled_convex_f32", ptr(s), ptr(am), ptr(mesh), h, w, d, (n - 1) // 2, ptr(out), *ws)
    return out if disp_mesh_t.dtype == torch.float32 else out.to(disp_mesh_t.dtype)


def inverse_consistency(disp_field1s, disp_field2s, iter=20):
    """Symmetric inverse-consistency fixed point on two normalised fields (1,3,h,w,d).  (convex_adam_utils.py:114-129)"""
    d1 = require_device_tensor(disp_field1s, "disp_field1s")
    d2 = require_device_tensor(disp_field2s, "disp_field2s")
    B, Cn, h, w, d = [int(s) for s in d1.shape]
    if B != 1 or Cn != 3 or d2.shape != d1.shape:
        raise ValueError("inverse_consistency expects two (1,3,h,w,d) fields")
    a, b = f32c(d1), f32c(d2)
    o1, o2 = torch.empty_like(a), torch.empty_like(b)
    bh, bw, bd = _base_tables(h, w, d, a.device)
    call(a.device, "cvx_inverse_consistency_f32", ptr(a), ptr(b), h, w, d, int(iter), ptr(bh), ptr(bw), ptr(bd), ptr(o1), ptr(o2),
         *scratch(a.device, "cvx_inverse_consistency_workspace_bytes", h, w, d))
    if d1.dtype != torch.float32:
        o1, o2 = o1.to(d1.dtype), o2.to(d1.dtype)
    return o1, o2


def resize_trilinear(x, size):
    """F.interpolate(x, size=size, mode='trilinear', align_corners=False) for (1,C,h,w,d).  (convex_adam_MIND.py:141,153,182)"""
    x = require_device_tensor(x, "x")
    _, Cn, h, w, d = [int(s) for s in x.shape]
    H, W, D = [int(s) for s in size]
    a = f32c(x)
    out = torch.empty((1, Cn, H, W, D), dtype=torch.float32, device=a.device)
    call(a.device, "cvx_resize_trilinear_f32", ptr(a), Cn, h, w, d, ptr(out), H, W, D)
    return out if x.dtype == torch.float32 else out.to(x.dtype)


def grid_sample(vol, grid):
    """F.grid_sample(vol, grid) (bilinear, zeros, align_corners=False): vol (1,C,h,w,d), grid (1,ho,wo,do,3)."""
    vol = require_device_tensor(vol, "vol")
    _, Cn, h, w, d = [int(s) for s in vol.shape]
    _, ho, wo, do_, three = [int(s) for s in grid.shape]
    if three != 3:
        raise ValueError("grid_sample: grid must be (1,ho,wo,do,3)")
    a, g = f32c(vol), f32c(grid.to(vol.device))
    out = torch.empty((1, Cn, ho, wo, do_), dtype=torch.float32, device=a.device)
    call(a.device, "cvx_grid_sample_f32", ptr(a), Cn, h, w, d, ptr(g), ho, wo, do_, ptr(out))
    return out if vol.dtype == torch.float32 else out.to(vol.dtype)


def box_smooth(x, k, passes=1):
    """`passes` x F.avg_pool3d(x, k, stride=1, padding=k//2) for (1,C,H,W,D).  (convex_adam_MIND.py:166,191)
    Odd k keeps the extent; an even k returns (1,C,H+passes,W+passes,D+passes) like torch."""
    x = require_device_tensor(x, "x")
    _, Cn, H, W, D = [int(s) for s in x.shape]
    a = f32c(x)
    if int(k) > 0 and int(k) % 2 == 0:
        # an even kernel makes every axis one voxel longer per pool (padding k//2 on both sides of k taps): what the reference's even
        # `selected_smooth` does (convex_adam_MIND.py:184-191)
        for _ in range(int(passes)):
            out = torch.empty((1, Cn, H + 1, W + 1, D + 1), dtype=torch.float32, device=a.device)
            call(a.device, "cvx_box_grow_f32", ptr(a), Cn, H, W, D, int(k), ptr(out))
            a, H, W, D = out, H + 1, W + 1, D + 1
        return a if x.dtype == torch.float32 else a.to(x.dtype)
    out = torch.empty_like(a)
    call(a.device, "cvx_box_smooth_f32", ptr(a), Cn, H, W, D, int(k), int(passes), ptr(out),
         *scratch(a.device, "cvx_box_smooth_workspace_bytes", Cn, H, W, D, int(passes)))
    return out if x.dtype == torch.float32 else out.to(x.dtype)


def smooth_fast(x, smoother, backward=False):
    """The separable restatement of a box-chain smoother (convexAdam_hyper_util.kovesi_spline) on a (1,3,h,w,d) / (3,h,w,d) device
    tensor (cvx_smooth_fast_f32); backward = the adjoint."""
    t = f32c(require_device_tensor(x, "x"))
    h, w, d = [int(s) for s in t.shape[-3:]]
    if t.numel() != 3 * h * w * d:
        raise ValueError("smooth_fast expects three channels")
    out = torch.empty_like(t)
    call(t.device, "cvx_smooth_fast_f32", ptr(t), h, w, d, C.byref(smoother.spec), 1 if backward else 0, ptr(out))
    return out


def box3_fast(x):
    """The separable restatement of box3(box3(box3(x))) (zero padding per stage) that adam_mode "fast" uses for the adjoint:
    x (1,3,h,w,d) or (3,h,w,d) device tensor -> same shape (cvx_box3_fast_f32)."""
    t = f32c(require_device_tensor(x, "x"))
    h, w, d = [int(s) for s in t.shape[-3:]]
    if t.numel() != 3 * h * w * d:
        raise ValueError("box3_fast expects three channels")
    out = torch.empty_like(t)
    call(t.device, "cvx_box3_fast_f32", ptr(t), h, w, d, ptr(out))
    return out


def combineDeformation3d(disp_1st, disp_2nd, identity):
    """disp_2nd + grid_sample(disp_1st, disp_2nd.permute(0,2,3,4,1) + identity).  (convex_adam_utils.py:133-135)"""
    return disp_2nd + grid_sample(disp_1st, disp_2nd.permute(0, 2, 3, 4, 1) + identity)


def adam_run(feat_fix, feat_mov, P0, lambda_weight, niter, cost_scale=12.0, snapshot_iters=(), return_state=False,
             state=None, smoother=None, storage="fp32", mode="exact"):
    """Adam instance optimisation of convex_adam_MIND.py:155-182 on pooled features (1,C,h,w,d) and an
    initial control grid P0 (1,3,h,w,d) in grid units.  Returns disp_sample of the last forward pass
    (1,3,h,w,d) [and optionally snapshots / optimiser state].  `smoother` = a GaussianSmoothing / kovesi_spline object of
    convexadam_amd.convexAdam_hyper_util replaces the three 3^3 boxes (adam_run_withconfig_shiftSpline.py:217).
    storage="fp16": the loop keeps its copies of the features in half precision (rounded once; float32 arithmetic; every mode).
    mode="fast": throughput arithmetic (cvx_adam_run_fast_f32: FMA / factored warp gradient, separable adjoint boxes, one division in
    the update; forward boxes in ATen's order) -- same mathematics, graded by end-point error; packaged smoother, float32 only;
    mode="fast_all": the forward boxes separable too (cvx_adam_run_fast_all_f32; faster, outside the fast mode's acceptance criteria)."""
    if storage not in ("fp32", "fp16"):
        raise ValueError("storage must be 'fp32' or 'fp16', got %r" % (storage,))
    if mode not in ("exact", "fast", "fast_all"):
        raise ValueError("mode must be 'exact', 'fast' or 'fast_all', got %r" % (mode,))
    F2 = f32c(require_device_tensor(feat_fix, "feat_fix"))
    M2 = f32c(require_device_tensor(feat_mov, "feat_mov"))
    _, Cn, h, w, d = [int(s) for s in F2.shape]
    dev = F2.device
    if state is None:
        P = f32c(P0.to(dev)).clone()
        m = torch.zeros_like(P)
        v = torch.zeros_like(P)
        step0 = 0
    else:
        P, m, v, step0 = state["P"], state["m"], state["v"], state["step"]
    U = torch.zeros_like(P)
    G = torch.zeros_like(P)
    bh, bw, bd = _base_tables(h, w, d, dev)
    snaps = sorted(int(i) for i in snapshot_iters)
    snap_arr = (C.c_int * max(len(snaps), 1))(*snaps) if snaps else None
    snap_buf = torch.empty((len(snaps), 3, h, w, d), dtype=torch.float32, device=dev) if snaps else None
    # the two entries differ in their name and in what their mode word means
    if mode in ("fast", "fast_all"):
        entry, word = "cvx_adam_run_mode_f32", (1 if mode == "fast" else 2) + (16 if storage == "fp16" else 0)
    else:
        entry, word = "cvx_adam_run_ex_f32", 1 if storage == "fp16" else 0
    call(dev, entry, ptr(F2), ptr(M2), Cn, h, w, d, ptr(P), ptr(m), ptr(v), float(lambda_weight), int(niter), int(step0), float(cost_scale),
         ptr(bh), ptr(bw), ptr(bd), ptr(U), ptr(G), C.cast(snap_arr, C.c_void_p) if snaps else None, len(snaps), ptr(snap_buf),
         C.byref(smoother.spec) if smoother is not None else None, word, *scratch(dev, "cvx_adam_workspace_bytes", Cn, h, w, d))
    if return_state:
        return U, dict(P=P, m=m, v=v, step=step0 + int(niter), G=G, snapshots=snap_buf)
    return U


_adam_sqrt_table = None


def sqrt_codes_from_low_bitmaps(normal, denormal):
    """Packed bit maps of the classes whose root is one ulp LOW (the layout of tests/golden/mkl_vssqrt_low.npz) -> 2-bit code table."""
    low = np.concatenate([np.unpackbits(np.ascontiguousarray(normal, np.uint8), bitorder="little"),
                          np.unpackbits(np.ascontiguousarray(denormal, np.uint8), bitorder="little")]).astype(np.uint8) * 2
    c = low.reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8)


def set_adam_sqrt_table(codes=None, denormal=None, device="cuda"):
    """Adam update with the reference build's square root (torch CPU -> MKL vsSqrt: the IEEE root or a neighbour, a function of exponent
    parity and mantissa) instead of the IEEE one.  `codes`: the 6 MiB 2-bit table of cvx_set_adam_sqrt_table (reference_bits.
    build_sqrt_table), or -- with `denormal` -- the two packed bit maps of tests/golden/mkl_vssqrt_low.npz; None restores the default.
    With the table `adam_run` is bit-identical to the reference's loop for given features."""
    global _adam_sqrt_table
    if codes is None:
        check(lib().cvx_set_adam_sqrt_table(None))
        _adam_sqrt_table = None
        return
    if denormal is not None:
        codes = sqrt_codes_from_low_bitmaps(codes, denormal)
    tbl = codes if isinstance(codes, torch.Tensor) else torch.from_numpy(np.array(codes, dtype=np.uint8, order="C"))
    assert tbl.dtype == torch.uint8 and tbl.numel() == 3 << 21, "2-bit codes of 2^24 + 2^23 classes expected"
    _adam_sqrt_table = tbl.to(device).contiguous()                          # (the library keeps its own copy)
    call(_adam_sqrt_table.device, "cvx_context_set_adam_sqrt_table", None, ptr(_adam_sqrt_table))
    _adam_sqrt_table = None


def validate_image(img, dtype=float):
    """np.ndarray / torch.Tensor (and SimpleITK / nibabel images when those packages are installed) -> torch.Tensor.
    Like the reference (convex_adam_utils.py:268-279) tensors pass through unchanged and everything else is converted with
    `astype(dtype)` -- float64 by default, so an int16 SimpleITK image is interpolated in floating point downstream;
    raises ValueError for unsupported types."""
    from .imageio import Image
    if isinstance(img, Image):
        img = img.array
    try:
        import SimpleITK as sitk  # noqa: N813
        if isinstance(img, sitk.Image):
            img = sitk.GetArrayFromImage(img)
    except ImportError:
        pass
    try:
        import nibabel as nib
        if isinstance(img, nib.Nifti1Image):
            img = img.get_fdata()
    except ImportError:
        pass
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img.astype(dtype)))
    if not isinstance(img, torch.Tensor):
        raise ValueError("Input image must be a SimpleITK image, a nibabel image, a numpy array or a torch tensor")
    return img


# ---- geometry helpers around the registration (convex_adam_utils.py:282-351) -----------------------------------------------------
# Kept importable under the reference's names (tests/test_convex_adam_mind_aniso.py:10-12, convex_adam_translation.py:9).  SimpleITK
# images go through SimpleITK's resampler exactly as in the reference; `imageio.Image` objects (the built-in image class, used when
# SimpleITK is not installed or simply not wanted) go through imageio.resample on the host, which follows ITK's index -> physical-point
# convention and linear interpolation -- or, with `device=` given, through the kernels of csrc/geometry.hip (geometry.py), which
# restate the same arithmetic in float64 and return the same types.
def _sitk():
    try:
        import SimpleITK as sitk  # noqa: N813
    except ImportError as e:
        raise ImportError("this call received an object that is not a convexadam_amd.imageio.Image and needs SimpleITK's resampler "
                          "(as in the reference, convex_adam_utils.py:282-351); SimpleITK is not installed") from e
    return sitk


def _is_builtin(img):
    from .imageio import Image
    return isinstance(img, Image)


def _linear_resampler(sitk, spacing, size, direction, origin):
    r = sitk.ResampleImageFilter()
    r.SetInterpolator(sitk.sitkLinear)
    r.SetTransform(sitk.Transform())          # identity
    r.SetDefaultPixelValue(0)                 # outside the source: zero
    r.SetOutputSpacing(spacing)
    r.SetSize(size)
    r.SetOutputDirection(direction)
    r.SetOutputOrigin(origin)
    return r


def _resample(img, spacing, size, direction, origin, device=None):
    if _is_builtin(img):
        if device is not None:
            from . import geometry
            from .imageio import Image
            out_grid = geometry.Grid(tuple(int(v) for v in size), tuple(spacing), tuple(origin), tuple(direction))
            out = geometry.resample_device(geometry.upload(img, device), geometry.grid_of(img), out_grid)
            return Image(out.cpu().numpy().astype(img.array.dtype, copy=False), spacing, origin, direction)
        from .imageio import resample
        return resample(img, spacing, size, direction, origin)
    return _linear_resampler(_sitk(), spacing, size, direction, origin).Execute(img)


def resample_img(img, spacing, device=None):
    """Linear resampling of an image to `spacing` on its own origin / orientation; size = floor(n * old / new + 0.5).
    device: None = on the host; a HIP device = built-in images through the resampling kernel (same type and geometry out)."""
    size = [int(n * old / new + 0.5) for n, old, new in zip(img.GetSize(), img.GetSpacing(), spacing)]
    return _resample(img, spacing, size, img.GetDirection(), img.GetOrigin(), device)


def resample_moving_to_fixed(fixed, moving, device=None):
    """Linear resampling of `moving` onto the voxel grid of `fixed` (zero outside); device as for resample_img."""
    return _resample(moving, fixed.GetSpacing(), fixed.GetSize(), fixed.GetDirection(), fixed.GetOrigin(), device)


def rescale_displacement_field(displacement_field, moving_image, fixed_image, fixed_image_resampled, device=None):
    """Displacement field (H,W,D,3; components z,y,x in voxels of `fixed_image_resampled`) -> the grid, axes and voxel size of the
    original `moving_image`: every component is resampled onto the moving grid, the vectors are rotated by the rotation between
    the two direction-cosine frames and scaled by the spacing ratio.
    device: None = on the host; a HIP device = built-in images through one launch of the carry-over kernel (float64 array out)."""
    if device is not None and _is_builtin(moving_image):
        from . import geometry
        field = displacement_field if isinstance(displacement_field, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(displacement_field))
        return geometry.rescale_displacement_field_device(field.to(device), moving_image, fixed_image, fixed_image_resampled).cpu().numpy()
    field = np.asarray(displacement_field)
    comps = []
    if _is_builtin(moving_image):
        from .imageio import Image, resample
        for axis in range(3):
            comp = Image(np.ascontiguousarray(field[..., axis]))
            comp.CopyInformation(fixed_image_resampled)
            comps.append(resample(comp, moving_image.GetSpacing(), moving_image.GetSize(), moving_image.GetDirection(),
                                  moving_image.GetOrigin()).array)
    else:
        sitk = _sitk()
        onto_moving = sitk.ResampleImageFilter()
        onto_moving.SetReferenceImage(moving_image)
        onto_moving.SetInterpolator(sitk.sitkLinear)
        for axis in range(3):
            comp = sitk.GetImageFromArray(field[..., axis])
            comp.CopyInformation(fixed_image_resampled)
            comps.append(sitk.GetArrayFromImage(onto_moving.Execute(comp)))
    moved = np.stack(comps, axis=-1)                                   # (..., 3) in z, y, x order
    frame_fixed = np.array(fixed_image.GetDirection()).reshape(3, 3)
    frame_moving = np.array(moving_image.GetDirection()).reshape(3, 3)
    rot = np.linalg.inv(frame_fixed) @ frame_moving
    rotated = (moved[..., ::-1] @ rot)[..., ::-1]                      # rotate in x, y, z order, back to z, y, x
    ratio = np.array(fixed_image_resampled.GetSpacing()) / np.array(moving_image.GetSpacing())     # x, y, z
    return rotated * ratio[::-1]


def gpu_usage():
    print('gpu usage (current/max): {:.2f} / {:.2f} GB'.format(torch.cuda.memory_allocated() * 1e-9,
                                                                 torch.cuda.max_memory_allocated() * 1e-9))


# thin-plate-spline densification (l2r_2021_convexAdam_task1_docker.py:198-262,365-387): csrc/tps.hip
from .tps import TPS, thin_plate_dense, tps_densify  # noqa: E402,F401
# least-trimmed rigid fit and fused affine warp (convex_adam_utils.py:173-193, l2r_2020_convexAdam_CuRIOUS.py:349-390): csrc/rigid.hip
from .rigid import affine_warp, find_rigid_3d, least_trimmed_rigid, rigid_from_field  # noqa: E402,F401
# the script's coarse foreground mask and landmark score (l2r_2020_convexAdam_CuRIOUS.py:312-319,328-330): csrc/rigidreg.hip
from .rigid import convex_adam_rigid, convex_stage, label_centroids, landmark_tre, rigid_samples, threshold_pool_mask  # noqa: E402,F401
# physical-space resampling and field carry-over on the device (convex_adam_utils.py:282-351, apply_convex.py:27-78): csrc/geometry.hip
from .geometry import (Grid, field_mean_device, grid_of, index_map, register_images, resample_device,  # noqa: E402,F401
                       rescale_displacement_field_device)
# a cropped-grid field carried to the original fixed grid at half resolution (l2r_2021_convexAdam_task1_docker.py:38-105,390-400): csrc/cropfield.hip
from .cropfield import (CropCase, convert_crop_field, half_resolution_field, physical_displacement, read_cases,  # noqa: E402,F401
                        submission_field)
# the nnU-Net preprocessing helpers (convex_adam_utils.py:15-21,142-170,196-265): csrc/prep.hip
from .prep import (compute_steps_for_sliding_window, create_nonzero_mask, crop_to_bbox, get_bbox_from_mask, get_gaussian,  # noqa: E402,F401
                   nnUNetCTnorm, nnUNetNorm, nnUNetNormProps, normalise_and_crop, pdist_squared)
# the opposite direction of a result -- inverse and composition of displacement fields (no counterpart in the reference): csrc/fieldops.hip
from .fieldops import apply_convex_inverse, compose_fields, invert_field  # noqa: E402,F401
# the affine model: least-trimmed affine fit, the affine as a field, affine pre-alignment (l2r_2020_convexAdam_CuRIOUS.py:272-278): csrc/affine.hip
from .affine import (affine_from_field, affine_to_field, convex_adam_affine, find_affine_3d, least_trimmed_affine,  # noqa: E402,F401
                     least_trimmed_squares, register_with_affine)
# the soft reading of the cost volume -- mean, covariance, entropy per coarse cell (no counterpart in the reference): csrc/softstats.hip
from .confidence import (Confidence, convex_confidence, soft_covariance, soft_displacement, soft_entropy, soft_sigma,  # noqa: E402,F401
                         soft_stats)
# mutual information of a pair -- fused warp + joint histogram, entropies, MI and NMI (no counterpart in the reference): csrc/simhist.hip
from .similarity import (RegistrationMI, entropies, joint_histogram, mutual_information,  # noqa: E402,F401
                         normalized_mutual_information, registration_mi, value_range)
# cubic B-spline interpolation -- prefilter, warp and resampling at scipy's order=3 (apply_convex(order=3), resample_device(order=3)): csrc/spline.hip
from .spline import spline_coefficients, warp_cubic  # noqa: E402,F401
