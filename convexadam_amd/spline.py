"""Cubic B-spline interpolation on the device: `order=3` of scipy.ndimage with the defaults apply_convex uses
(mode='constant', cval=0, prefilter=True), in float64 -- for the step a user looks at, the final warp of the moving INTENSITY image and
the resampling of an image to the registration grid and back, where the linear gather blurs by an amount that depends on the sub-voxel
phase of the field.

    spline_coefficients(volume)                    the recursive prefilter along all three axes -> float64 coefficients
    warp_cubic(moving, disp, prefiltered=False)    the volume sampled at identity + disp, 0 outside
    apply_convex(disp, moving, order=3)            convexadam_amd.apply_convex, the reference's function with scipy's keyword
    resample_device(src, ..., order=3)             convexadam_amd.geometry, the ITK-convention resampling with the same keyword

The entry points are those of include/convexadam_spline.h (cvx_spline_prefilter_f64, cvx_map_coordinates_cubic_f64,
cvx_resample_cubic_f64); the arithmetic is stated in csrc/spline_core.h and restated in tests/spline_restatement.py.  Tensors must live
on the HIP device; there is no CPU path.

Not built: orders 2, 4 and 5; boundary modes other than 'constant' with cval = 0 (and ITK's buffer rule in resample_device); a cubic
variant of the warped output of cvx_field_to_grid_f64 (rescale_displacement_field_device) and of the joint histogram's fused warp; anything
inside the registration itself, which stays trilinear; gradients."""
import torch

from . import _lib
from ._lib import call, field_operand, ptr, require_device_tensor


def _samples(volume, name):
    """(z, y, x) device tensor -> (float32 / float64 contiguous tensor, is_f64, shape); every other dtype is read as float64"""
    volume = require_device_tensor(volume, name)
    if volume.dim() != 3:
        raise ValueError("%s must be an (H, W, D) volume, got %s" % (name, tuple(volume.shape)))
    t = volume.detach()
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t.contiguous(), int(t.dtype == torch.float64), tuple(int(s) for s in t.shape)


def spline_coefficients(volume):
    """The cubic B-spline coefficients of an (H, W, D) device volume -> float64 device tensor of the same shape: what
    scipy.ndimage.spline_filter(volume, order=3, mode='constant') returns.  float32 and float64 samples are read as they are."""
    s, s64, shape = _samples(volume, "volume")
    _lib.spline_lib()
    coef = torch.empty(shape, dtype=torch.float64, device=s.device)
    call(s.device, "cvx_spline_prefilter_f64", ptr(s), s64, *shape, ptr(coef))
    return coef


def warp_cubic(moving, disp, prefiltered=False):
    """moving sampled at identity + disp with cubic B-splines -> (H, W, D) float64 device tensor, 0.0 where the sampling point lies outside
    the volume or is not finite: scipy.ndimage.map_coordinates(moving, identity + disp, order=3).

    moving       (H, W, D) device tensor; with prefiltered=True the float64 coefficients spline_coefficients returned (one prefilter
                 for many warps)
    disp         (H, W, D, 3) or (3, H, W, D) device tensor in voxels, float32 or float64, read where it lies"""
    moving = require_device_tensor(moving, "moving")
    disp = require_device_tensor(disp, "disp")
    if prefiltered:
        if moving.dim() != 3 or moving.dtype != torch.float64:
            raise ValueError("prefiltered=True expects the (H, W, D) float64 tensor of spline_coefficients")
        coef = moving.detach().contiguous()
    else:
        coef = spline_coefficients(moving)
    shape = tuple(int(s) for s in coef.shape)
    u, _, cs, vs, f64 = field_operand(disp.to(coef.device), grid=shape, name="disp")
    _lib.spline_lib()
    out = torch.empty(shape, dtype=torch.float64, device=coef.device)
    call(coef.device, "cvx_map_coordinates_cubic_f64", ptr(coef), ptr(u), f64, cs, vs, *shape, ptr(out))
    return out


def resample_cubic(src, out_shape, map12, default=0.0, out_f64=True):
    """The cubic twin of the launch inside geometry.resample_device: src (z, y, x) device samples, map12 the ctypes array of the index map."""
    coef = spline_coefficients(src)
    out = torch.empty(tuple(out_shape), dtype=torch.float64 if out_f64 else torch.float32, device=coef.device)
    sz, sy, sx = coef.shape
    oz, oy, ox = out.shape
    call(coef.device, "cvx_resample_cubic_f64", ptr(coef), sz, sy, sx, ptr(out), int(out_f64), oz, oy, ox, map12, float(default))
    return out
