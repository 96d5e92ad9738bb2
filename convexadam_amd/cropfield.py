"""A field on the crop + resize grid carried to the original fixed image at half resolution (csrc/cropfield.hip): what
l2r_2021_convexAdam_task1_docker.py does between its thin-plate spline and the file it submits (:38-105, :390-400), in one launch.

    CropCase(...)                                        one row of the reference's cases.csv: shapes, spacings and crops of a pair
    read_cases(path)                                     {Id: CropCase} of such a file
    physical_displacement(disp, fix_sp, mov_sp)          voxel field -> displacement in millimetres (task1:390-397), for callers who want it
    convert_crop_field(case, fix_affine_disp_p)          the reference's function: (1, H, W, D, 3) physical field -> (3, S0//2, S1//2, S2//2)
    submission_field(disp_voxels, fix_sp, mov_sp, case)  the same from the (1, 3, H, W, D) voxel field of tps_densify, still one launch
    half_resolution_field(disp)                          F.interpolate(disp, scale_factor=0.5, mode='trilinear') alone (task2:308, task3:214)

The per-case constants are computed on the host in float32 exactly as the reference computes them (:53-58) and handed to the kernel as
doubles; everything per voxel runs in the kernel.  Device tensors only; nothing here synchronises with the host.
"""
import csv
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from ._lib import _shape, call, f32c, field_operand, ptr, require_device_tensor

CROP_FIELD_VOXELS, CROP_OUT_F32, CROP_IDENTITY = 1, 2, 4          # the flags of cvx_crop_field_half_f32
_FLIP_BITS = {"x": 1, "y": 2, "z": 4}                              # the reference's letters: 'x' = array axis 0, 'y' = 1, 'z' = 2
_OUT = {torch.float16: 0, torch.float32: CROP_OUT_F32}

_CropCase = namedtuple("CropCase", "fix_shape fix_spacing fix_crop mov_shape mov_spacing mov_crop ref_spacing flip")


class CropCase(_CropCase):
    """Shapes (voxels), spacings (mm) and crops of a fixed / moving pair.  A crop is six numbers (lo0, hi0, lo1, hi1, lo2, hi2), the
    reference's `view(3, 2)`; ref_spacing is the isotropic spacing the crops were resized towards; flip names the axes that the
    submission format turns ('x', 'y', 'z' = array axis 0, 1, 2)."""
    __slots__ = ()

    def __new__(cls, fix_shape, fix_spacing, fix_crop, mov_shape, mov_spacing, mov_crop, ref_spacing=2.0, flip="xy"):
        def numbers(v, n, name):
            try:
                t = tuple(float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1))
            except (TypeError, ValueError):
                raise ValueError("%s must be %d numbers, got %r" % (name, n, v)) from None
            if len(t) != n or not all(np.isfinite(t)):
                raise ValueError("%s must be %d finite numbers, got %r" % (name, n, v))
            return t
        fs, ms = numbers(fix_shape, 3, "fix_shape"), numbers(mov_shape, 3, "mov_shape")
        if any(s < 1 or s != int(s) for s in fs + ms):
            raise ValueError("shapes must be positive integers, got %r and %r" % (fix_shape, mov_shape))
        fsp, msp = numbers(fix_spacing, 3, "fix_spacing"), numbers(mov_spacing, 3, "mov_spacing")
        if any(s <= 0 for s in fsp + msp) or not (np.isfinite(float(ref_spacing)) and float(ref_spacing) > 0):
            raise ValueError("spacings must be positive")
        fc, mc = numbers(fix_crop, 6, "fix_crop"), numbers(mov_crop, 6, "mov_crop")
        if any(c[2 * a + 1] <= c[2 * a] for c in (fc, mc) for a in range(3)):
            raise ValueError("a crop must have hi > lo on every axis, got %r and %r" % (fix_crop, mov_crop))
        if not isinstance(flip, str) or any(ch not in _FLIP_BITS for ch in flip):
            raise ValueError("flip must name axes out of 'x', 'y', 'z', got %r" % (flip,))
        return super().__new__(cls, tuple(int(s) for s in fs), fsp, fc, tuple(int(s) for s in ms), msp, mc, float(ref_spacing), flip)

    @property
    def flip_mask(self):
        return sum(bit for ch, bit in _FLIP_BITS.items() if ch in self.flip)

    def constants(self):
        """The per-axis numbers of convert_crop_field in the reference's own float32 arithmetic (task1:53-58), as float32 arrays:
        new_shape, fix_scale (new_fix_scale_factor), new_fix_spacing, mov_scale (new_mov_scale_factor), new_mov_spacing, and the crops'
        lower and upper corners."""
        f32 = np.float32
        fix_crop, mov_crop = np.array(self.fix_crop, f32).reshape(3, 2), np.array(self.mov_crop, f32).reshape(3, 2)
        fix_sp, mov_sp = np.array(self.fix_spacing, f32), np.array(self.mov_spacing, f32)
        fix_ext, mov_ext = fix_crop[:, 1] - fix_crop[:, 0], mov_crop[:, 1] - mov_crop[:, 0]
        new_shape = np.round(fix_ext * (fix_sp / np.full(3, self.ref_spacing, f32)))          # half to even, like torch.round
        fix_scale, mov_scale = new_shape / fix_ext, new_shape / mov_ext
        return dict(new_shape=new_shape, fix_scale=fix_scale, new_fix_spacing=fix_sp / fix_scale, mov_scale=mov_scale,
                    new_mov_spacing=mov_sp / mov_scale, fix_crop_lo=fix_crop[:, 0], fix_crop_hi=fix_crop[:, 1], mov_crop_lo=mov_crop[:, 0])

    def geometry(self, pre_fix_spacing=(1.0, 1.0, 1.0), pre_mov_spacing=(1.0, 1.0, 1.0)):
        """geom27_host of cvx_crop_field_half_f32: nine triples of float64."""
        k = self.constants()
        pre = [np.array(tuple(float(v) for v in s), np.float32) for s in (pre_fix_spacing, pre_mov_spacing)]
        if any(p.shape != (3,) or not np.all(np.isfinite(p)) or np.any(p <= 0) for p in pre):
            raise ValueError("the preprocessed spacings must be three positive numbers each")
        return np.concatenate([k["fix_scale"], k["fix_crop_lo"], k["new_fix_spacing"], k["new_mov_spacing"], k["mov_scale"], k["mov_crop_lo"],
                               pre[0], pre[1], k["fix_crop_hi"]]).astype(np.float64)

    def check_field_shape(self, shape):
        """ValueError unless `shape` (H, W, D) is the grid this case's fixed crop resizes to."""
        want = tuple(int(v) for v in self.constants()["new_shape"])
        if tuple(shape) != want:
            raise ValueError("the field lives on %s, the case's fixed crop resizes to %s" % (tuple(shape), want))


def _bracketed(text, n, name):
    t = text.strip()
    if not (t.startswith("[") and t.endswith("]")):
        raise ValueError("%s must be a bracketed list, got %r" % (name, text))
    v = [float(j) for j in t[1:-1].split()]
    if len(v) != n:
        raise ValueError("%s must hold %d numbers, got %r" % (name, n, text))
    return v


def read_cases(path, ref_spacing=2.0, flip="xy"):
    """{Id: CropCase} of the reference's cases.csv (task1:39-49): columns Id, FixShape, FixSpacing, FixCrop, MovShape, MovSpacing,
    MovCrop, values bracketed and space-separated, six numbers per crop."""
    cases = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            try:
                cases[row["Id"]] = CropCase(_bracketed(row["FixShape"], 3, "FixShape"), _bracketed(row["FixSpacing"], 3, "FixSpacing"),
                                            _bracketed(row["FixCrop"], 6, "FixCrop"), _bracketed(row["MovShape"], 3, "MovShape"),
                                            _bracketed(row["MovSpacing"], 3, "MovSpacing"), _bracketed(row["MovCrop"], 6, "MovCrop"),
                                            ref_spacing, flip)
            except (KeyError, TypeError, AttributeError):
                raise ValueError("%s: a row lacks one of the columns Id, FixShape, FixSpacing, FixCrop, MovShape, MovSpacing, MovCrop"
                                 % path) from None
    return cases


def _spacing(v, name):
    try:
        s = tuple(float(x) for x in (v.tolist() if isinstance(v, torch.Tensor) else v))
    except (TypeError, ValueError):
        raise ValueError("%s must be three positive numbers, got %r" % (name, v)) from None
    if len(s) != 3 or not all(np.isfinite(s)) or any(x <= 0 for x in s):
        raise ValueError("%s must be three positive numbers, got %r" % (name, v))
    return s


def _out_flag(out_dtype):
    if out_dtype not in _OUT:
        raise ValueError("out_dtype must be torch.float16 or torch.float32, got %r" % (out_dtype,))
    return _OUT[out_dtype]


def _check_full(full):
    if min(full) < 2:
        raise ValueError("an original grid of %s has no half-resolution output" % (tuple(full),))


def _launch(t, name, planar, grid, geom, full, flip_mask, flags, out_dtype):
    """t: the field with its leading 1 (if any), float32 to the kernel whatever its dtype; planar: (3, H, W, D), else (H, W, D, 3)"""
    t = require_device_tensor(t, name)
    f, grid, cs, vs, _ = field_operand(t.reshape(t.shape[-4:]), grid, planar=planar, f32=True)
    out = torch.empty((3,) + tuple(s // 2 for s in full), dtype=out_dtype, device=f.device)
    g = (C.c_double * 27)(*geom.tolist()) if geom is not None else None
    call(f.device, "cvx_crop_field_half_f32", ptr(f), cs, vs, grid[0], grid[1], grid[2], g, full[0], full[1], full[2], flip_mask, flags, ptr(out))
    return out


def physical_displacement(disp, fix_spacing, mov_spacing):
    """disp_p of task1:390-397: (y + u(y)) * mov_spacing - y * fix_spacing for the (1, 3, H, W, D) voxel field u on its own grid, as
    (1, H, W, D, 3) float32 in millimetres.  A few element-wise device operations for callers who want the field itself; the path to
    the submission (submission_field) never forms it."""
    s = _shape(disp, "disp")
    if len(s) != 5 or s[0] != 1 or s[1] != 3:
        raise ValueError("disp must be (1, 3, H, W, D), got %s" % (s,))
    fix_spacing, mov_spacing = _spacing(fix_spacing, "fix_spacing"), _spacing(mov_spacing, "mov_spacing")
    d = f32c(require_device_tensor(disp, "disp"))
    dev = d.device
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, device=dev) for n in s[2:]], indexing="ij"), dim=3).unsqueeze(0)
    fs, ms = torch.tensor(fix_spacing, device=dev), torch.tensor(mov_spacing, device=dev)
    return (grid + d.permute(0, 2, 3, 4, 1)) * ms - grid * fs


def convert_crop_field(case, fix_affine_disp_p, out_dtype=torch.float16):
    """convert_crop_field of task1:38-105.  case: a CropCase; fix_affine_disp_p: (1, H, W, D, 3) device tensor, the displacement in
    millimetres on the crop + resize grid.  Returns the displacement on the original fixed grid, axes flipped as the case says, at half
    resolution: (3, S0//2, S1//2, S2//2) in `out_dtype` (float16 like the reference's file, or float32)."""
    if not isinstance(case, CropCase):
        raise TypeError("case must be a CropCase (read_cases gives them by Id)")
    s = _shape(fix_affine_disp_p, "fix_affine_disp_p")
    if len(s) != 5 or s[0] != 1 or s[4] != 3:
        raise ValueError("fix_affine_disp_p must be (1, H, W, D, 3), got %s" % (s,))
    case.check_field_shape(s[1:4])
    _check_full(case.fix_shape)
    flags = _out_flag(out_dtype)
    return _launch(fix_affine_disp_p, "fix_affine_disp_p", False, s[1:4], case.geometry(), case.fix_shape, case.flip_mask, flags, out_dtype)


def submission_field(disp_voxels, pre_fix_spacing, pre_mov_spacing, case, out_dtype=torch.float16):
    """task1:390-400 in one launch: the (1, 3, H, W, D) (or (3, H, W, D)) voxel field that tps_densify returns, the spacings of the two
    preprocessed images it was registered on, and the case -> what convert_crop_field(case, physical_displacement(...)) returns, without
    the millimetre field in between (the kernel converts each tap as it reads it)."""
    if not isinstance(case, CropCase):
        raise TypeError("case must be a CropCase (read_cases gives them by Id)")
    s = _shape(disp_voxels, "disp_voxels")
    if len(s) == 4:
        s = (1,) + s
    if len(s) != 5 or s[0] != 1 or s[1] != 3:
        raise ValueError("disp_voxels must be (1, 3, H, W, D) or (3, H, W, D), got %s" % (tuple(disp_voxels.shape),))
    case.check_field_shape(s[2:])
    _check_full(case.fix_shape)
    geom = case.geometry(_spacing(pre_fix_spacing, "pre_fix_spacing"), _spacing(pre_mov_spacing, "pre_mov_spacing"))
    flags = _out_flag(out_dtype) | CROP_FIELD_VOXELS
    return _launch(disp_voxels, "disp_voxels", True, s[2:], geom, case.fix_shape, case.flip_mask, flags, out_dtype)


def half_resolution_field(disp, out_dtype=torch.float32):
    """F.interpolate(disp, scale_factor=0.5, mode='trilinear', align_corners=False) of a (1, 3, H, W, D) or (3, H, W, D) field, bit for
    bit in float32 (task2:308, task3:214); torch.float16 gives its round-to-nearest-even cast.  Not resize_trilinear to size = shape // 2:
    the two differ on odd extents, where ATen's scale is exactly 2 under scale_factor and in / out under size."""
    s = _shape(disp, "disp")
    lead = s[:-4]
    if len(s) not in (4, 5) or s[-4] != 3 or lead not in ((), (1,)):
        raise ValueError("disp must be (1, 3, H, W, D) or (3, H, W, D), got %s" % (s,))
    _check_full(s[-3:])
    flags = _out_flag(out_dtype) | CROP_IDENTITY
    out = _launch(disp, "disp", True, s[-3:], None, s[-3:], 0, flags, out_dtype)
    return out.unsqueeze(0) if lead else out
