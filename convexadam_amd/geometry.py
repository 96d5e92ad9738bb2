"""Physical-space resampling and field carry-over on the HIP device (csrc/geometry.hip): the steps the reference does
with SimpleITK's resampler before and after a registration (convex_adam_utils.py:282-351, apply_convex.py:27-78).

    grid_of(img)                                   Grid(size, spacing, origin, direction) of anything with SimpleITK's accessors
    index_map(src_grid, out_grid)                  M (3, 3), t (3,): source index (x, y, z) = M @ output index + t
    resample_device(src, src_grid, out_grid)       ITK-convention linear (order=3: cubic B-spline) resampling of a (z, y, x) device tensor
                                                   onto another grid
    rescale_displacement_field_device(...)         a field on the resampled fixed grid -> the original moving image's grid, axes and voxel
                                                   size and, in the same launch, that image warped by it
    field_mean_device(field, ...)                  sums and count of a field over all voxels, a mask, or a segmentation on its own grid
                                                   (csrc/fieldmean.hip): convex_adam_translation's reduction
    register_images(fixed_image, moving_image)     the reference tests' whole flow, one upload per image

Geometry travels as `Grid` tuples (x, y, z order like SimpleITK), voxels as device tensors in (z, y, x) order like sitk.GetArrayFromImage.
The twelve numbers of an index map are computed on the host exactly as imageio.resample computes them; everything per voxel runs in the
kernels, in float64.  Nothing here synchronises with the host except register_images, which returns an image and two numbers.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from ._lib import call, field_operand, ptr, require_device_tensor, scratch

Grid = namedtuple("Grid", "size spacing origin direction")          # x, y, z; direction: 9 values, row-major
Registration = namedtuple("Registration", "field carried_field warped ssim_before ssim_after")


def grid_of(img):
    """Size, spacing, origin and direction of an image (GetSize / GetSpacing / GetOrigin / GetDirection: imageio.Image, SimpleITK)."""
    if isinstance(img, Grid):
        return img
    return Grid(tuple(int(v) for v in img.GetSize()), tuple(float(v) for v in img.GetSpacing()), tuple(float(v) for v in img.GetOrigin()),
                tuple(float(v) for v in img.GetDirection()))


def _index_to_physical(grid):
    """(A, o) with p = A @ index_xyz + o (imageio.Image.index_to_physical_matrix)."""
    D = np.array(grid.direction, dtype=np.float64).reshape(3, 3)
    return D * np.array(grid.spacing, dtype=np.float64)[None, :], np.array(grid.origin, dtype=np.float64)


def index_map(src_grid, out_grid):
    """M, t with source index (x, y, z) = M @ output index (x, y, z) + t: the two solves of imageio.resample, so that the host path and
    the kernels start from the same twelve numbers."""
    Ao, oo = _index_to_physical(grid_of(out_grid))
    As, os_ = _index_to_physical(grid_of(src_grid))
    return np.linalg.solve(As, Ao), np.linalg.solve(As, oo - os_)


def _doubles(*arrays):
    flat = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in arrays])
    return (C.c_double * flat.size)(*flat.tolist())


def _volume(t, grid, name):
    """float32 / float64 contiguous (z, y, x) device tensor matching `grid` -> (tensor, is_f64)"""
    if tuple(t.shape) != tuple(grid.size)[::-1]:
        raise ValueError("%s has shape %s, its grid says (z, y, x) = %s" % (name, tuple(t.shape), tuple(grid.size)[::-1]))
    t = t.detach()
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)                                  # integers (and half floats) are interpolated in float64
    return t.contiguous(), int(t.dtype == torch.float64)


def resample_device(src, src_grid, out_grid, default=0.0, order=1):
    """Linear resampling of the (z, y, x) device tensor `src` living on `src_grid` onto `out_grid`, identity transform, `default`
    outside (imageio.resample on the device).  float32 and float64 keep their dtype; integer sources are interpolated in float64 and
    cast back with round-half-even, like np.rint there.  order=3: cubic B-splines instead (convexadam_amd.spline: the prefilter, then the
    gather under the same inside rule); every other order raises ValueError."""
    if order not in (1, 3):
        raise ValueError("resample_device: order must be 1 (linear) or 3 (cubic B-spline), got %r" % (order,))
    require_device_tensor(src, "src")
    src_grid, out_grid = grid_of(src_grid), grid_of(out_grid)
    s, s64 = _volume(src, src_grid, "src")
    M, t = index_map(src_grid, out_grid)
    sx, sy, sz = src_grid.size
    ox, oy, oz = out_grid.size
    if order == 3:
        from .spline import resample_cubic
        out = resample_cubic(s, (oz, oy, ox), _doubles(M, t), default, out_f64=bool(s64))
    else:
        out = torch.empty((oz, oy, ox), dtype=s.dtype, device=s.device)
        call(s.device, "cvx_resample_linear_f64", ptr(s), s64, sz, sy, sx, ptr(out), s64, oz, oy, ox, _doubles(M, t), float(default))
    if src.dtype in (torch.float32, torch.float64):
        return out
    if src.dtype.is_floating_point:
        return out.to(src.dtype)
    return torch.round(out).to(src.dtype)                       # torch.round: half to even


def field_frame(moving_grid, fixed_grid, fixed_resampled_grid):
    """R = inv(D_fixed) @ D_moving and ratio = spacing(resampled fixed) / spacing(moving), x, y, z order (convex_adam_utils.py:340-351)."""
    frame_fixed = np.array(grid_of(fixed_grid).direction).reshape(3, 3)
    frame_moving = np.array(grid_of(moving_grid).direction).reshape(3, 3)
    rot = np.linalg.inv(frame_fixed) @ frame_moving
    ratio = np.array(grid_of(fixed_resampled_grid).spacing) / np.array(grid_of(moving_grid).spacing)
    return rot, ratio


def rescale_displacement_field_device(field, moving_grid, fixed_grid, fixed_resampled_grid, moving=None, want_field=True,
                                      warped_dtype=torch.float32):
    """rescale_displacement_field, and apply_convex of the original moving image, in one launch.

    field: device tensor on the resampled fixed grid, (H, W, D, 3) as convex_adam_pt returns it or (3, H, W, D) as register_pair_device
    does, float32 or float64, read in place (no copy, no transposition); components z, y, x in voxels.  Returns the carried field,
    (mz, my, mx, 3) float64 on the moving grid; with `moving` (the original moving image's voxels, (mz, my, mx) device tensor) also the
    warped volume in `warped_dtype` (float32 like the reference's .astype(np.float32), or float64).  want_field=False skips the field
    and returns the warped volume alone."""
    require_device_tensor(field, "field")
    mg, fg, rg = grid_of(moving_grid), grid_of(fixed_grid), grid_of(fixed_resampled_grid)
    f, shape, cs, vs, f64 = field_operand(field, tuple(rg.size)[::-1])
    dev = f.device
    mx, my, mz = mg.size
    m, m64 = (None, 0)
    if moving is not None:
        require_device_tensor(moving, "moving")
        if moving.device != dev:
            raise ValueError("field on %s, moving on %s" % (dev, moving.device))
        m, m64 = _volume(moving, mg, "moving")
    elif not want_field:
        raise ValueError("nothing to compute: want_field=False and no moving volume")
    if warped_dtype not in (torch.float32, torch.float64):
        raise ValueError("warped_dtype must be torch.float32 or torch.float64")
    carried = torch.empty((mz, my, mx, 3), dtype=torch.float64, device=dev) if want_field else None
    warped = torch.empty((mz, my, mx), dtype=warped_dtype, device=dev) if m is not None else None
    M, t = index_map(rg, mg)
    rot, ratio = field_frame(mg, fg, rg)
    call(dev, "cvx_field_to_grid_f64", ptr(f), f64, cs, vs, shape[0], shape[1], shape[2], _doubles(M, t), _doubles(rot), _doubles(ratio),
         ptr(m), m64, mz, my, mx, ptr(carried), ptr(warped), int(warped_dtype == torch.float64))
    if moving is None:
        return carried
    return (carried, warped) if want_field else warped


_QUANTIZE = {None: 0, 0: 0, 1: 1, torch.float32: 0, torch.float16: 1}          # the `quantize` of cvx_pack_field_f64
SEG_KIND_F64, SEG_KIND_F32, SEG_KIND_INT = 0, 1, 2


def field_mean_device(field, field_grid=None, mask=None, seg=None, seg_grid=None, quantize=None):
    """Sums and count of a displacement field over the voxels that count (cvx_field_mean_f64): the reduction of convex_adam_translation
    (convex_adam_translation.py:88-103) without the field leaving the device.

    field: (H, W, D, 3) or (3, H, W, D) device tensor, float32 or float64, read in place; components z, y, x.
    quantize: None / torch.float32 / 0 = the values as they are; torch.float16 / 1 = each value through convex_adam_pt's default `dtype` round trip
    first (float32 fields only).
    Which voxels count: all of them; or those where `mask` ((H, W, D) device tensor) is nonzero; or those where `seg`, a (z, y, x) device
    tensor on `seg_grid`, resampled onto `field_grid` is > 0 -- bit for bit the mask `resample_device(seg, seg_grid, field_grid) > 0`, decided
    per voxel inside the kernel; the resampled volume is never written.  `mask` and `seg` exclude each other.
    Returns (sums float64[3], count int64 scalar), two views of one 32-byte device buffer; nothing here waits for the device.  The mean
    is sums / count; the order of the additions is fixed, so two calls give the same bits."""
    out = field_mean_buffer(field, field_grid, mask, seg, seg_grid, quantize)
    return out[:3], out[3:].view(torch.int64)[0]


def field_mean_buffer(field, field_grid=None, mask=None, seg=None, seg_grid=None, quantize=None):
    """field_mean_device's result as the one device buffer the kernel wrote: float64[4], the three sums and the bits of the int64 count
    (for a caller that downloads all 32 bytes at once)."""
    require_device_tensor(field, "field")
    if quantize not in _QUANTIZE:
        raise ValueError("quantize must be None / torch.float32 / 0, or torch.float16 / 1")
    grid = tuple(grid_of(field_grid).size)[::-1] if field_grid is not None else tuple(mask.shape) if mask is not None else None
    f, shape, cs, vs, f64 = field_operand(field, grid, strict=True)         # no grid, no mask: the shape itself has to say the layout
    dev = f.device
    if mask is not None and seg is not None:
        raise ValueError("mask and seg exclude each other")
    m = s = None
    kind, sext, m12 = 0, (0, 0, 0), None
    if mask is not None:
        require_device_tensor(mask, "mask")
        if mask.device != dev or tuple(mask.shape) != shape:
            raise ValueError("mask %s on %s does not match the field's grid %s on %s" % (tuple(mask.shape), mask.device, shape, dev))
        m = (mask.detach() != 0).to(torch.uint8).contiguous()
    if seg is not None:
        require_device_tensor(seg, "seg")
        if seg_grid is None or field_grid is None:
            raise ValueError("seg needs seg_grid and field_grid")
        if seg.device != dev:
            raise ValueError("field on %s, seg on %s" % (dev, seg.device))
        sg = grid_of(seg_grid)
        kind = SEG_KIND_F64 if seg.dtype == torch.float64 else SEG_KIND_F32 if seg.dtype == torch.float32 else SEG_KIND_INT
        if seg.dtype.is_floating_point and kind == SEG_KIND_INT:
            raise ValueError("seg must be float32, float64 or an integer type, got %s" % seg.dtype)
        s, _ = _volume(seg, sg, "seg")
        sext = tuple(sg.size)[::-1]
        m12 = _doubles(*index_map(sg, grid_of(field_grid)))
    out = torch.empty(4, dtype=torch.float64, device=dev)
    call(dev, "cvx_field_mean_f64", ptr(f), f64, cs, vs, shape[0], shape[1], shape[2], _QUANTIZE[quantize], ptr(m), ptr(s), kind,
         sext[0], sext[1], sext[2], m12, C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 24),
         *scratch(dev, "cvx_field_mean_workspace_bytes", *shape, required=True))
    return out


def resampled_grid(grid, spacing):
    """The grid resample_img puts an image on: same origin and direction, `spacing`, size int(n * old / new + 0.5)."""
    grid = grid_of(grid)
    size = tuple(int(n * old / new + 0.5) for n, old, new in zip(grid.size, grid.spacing, spacing))
    return Grid(size, tuple(float(v) for v in spacing), grid.origin, grid.direction)


def upload(img, device):
    """The voxels of an imageio.Image (or a (z, y, x) array) as a device tensor in their own dtype (unsigned 16/32/64-bit: as int64)."""
    arr = np.ascontiguousarray(getattr(img, "array", img))
    if arr.dtype in (np.dtype(np.uint16), np.dtype(np.uint32), np.dtype(np.uint64)):
        arr = arr.astype(np.int64)
    if not arr.flags.writeable:
        arr = arr.copy()                                         # (torch.from_numpy warns about read-only arrays)
    return torch.from_numpy(arr).to(device)


def register_images(fixed_image, moving_image, spacing=(1.0, 1.0, 1.0), window_size=11, **registration_keywords):
    """The reference tests' flow (tests/test_convex_adam_mind_aniso.py) for two imageio.Image objects with their own spacing, origin and
    direction, on the device with one upload per image:

        fixed resampled to `spacing` (size int(n * old / new + 0.5)), moving resampled onto that grid, register_pair_device,
        one launch that carries the field to the original moving grid and warps the original moving image, SSIM before / after

    Returns Registration(field, carried_field, warped, ssim_before, ssim_after): the (3, H, W, D) float32 field on the resampled grid and
    the (mz, my, mx, 3) float64 carried field, both on the device; the warped original moving image as a float32 Image with the moving
    image's geometry; ssim3D(fixed, moving) and ssim3D(fixed, moving warped) on the resampled grid as floats.
    The field is register_pair_device's float32 field as it is: it does NOT pass through convex_adam_pt's packing (fp16 rounding on the
    device, float64 on the host), so it differs from convex_adam_pt's return value by that rounding.
    Keywords: `device` (default: the current HIP device); everything else goes to register_pair_device."""
    from .convex_adam_MIND import register_pair_device
    from .imageio import Image
    from .ssim import registration_ssim, ssim3D
    dev = torch.device(registration_keywords.pop("device", None) or ("cuda:%d" % torch.cuda.current_device()))
    gf, gm = grid_of(fixed_image), grid_of(moving_image)
    gr = resampled_grid(gf, spacing)
    fix, mov = upload(fixed_image, dev), upload(moving_image, dev)
    fix_r = resample_device(fix, gf, gr).to(torch.float32)
    mov_r = resample_device(mov, gm, gr).to(torch.float32)
    field = register_pair_device(fix_r, mov_r, **registration_keywords)
    if tuple(field.shape) != (3,) + tuple(fix_r.shape):
        raise ValueError("register_images needs the full-resolution field, got %s for images of %s" % (tuple(field.shape), tuple(fix_r.shape)))
    carried, warped = rescale_displacement_field_device(field, gm, gf, gr, moving=mov)
    before = ssim3D(fix_r[None, None], mov_r[None, None], window_size=window_size)
    after = registration_ssim(fix_r, mov_r, field, window_size=window_size)
    out = Image(warped.cpu().numpy(), gm.spacing, gm.origin, gm.direction)
    return Registration(field, carried, out, float(before), float(after))
