"""The opposite direction of a registration result, on the HIP device (csrc/fieldops.hip).

convex_adam_pt returns the forward field u on the fixed grid: apply_convex(u, moving)(x) = moving(x + u(x)).  The reference has nothing that
turns it round; a user needs that to bring the fixed image (or a segmentation drawn on it) into the moving frame, to carry moving-space
landmarks to the fixed image, and to see how far from invertible a result is.

    invert_field(disp, max_iters=50, tol=1e-4)     v with v(y) = -u(y + v(y)): the fixed-point iteration v <- -u(y + v), all iterations of a
                                                   voxel in registers inside ONE launch
    compose_fields(first, second)                  the single field equal to warping with `first`, then with `second`:
                                                   out(x) = second(x) + first(x + second(x))
    apply_convex_inverse(disp, fixed)              apply_convex(invert_field(disp), fixed): the fixed image in the moving frame

Fields are in voxels, component a along array axis a.  (H, W, D, 3) numpy arrays, images and host tensors go up, are computed in float64
and come back as float64 numpy arrays, as apply_convex treats its inputs.  A device tensor -- (H, W, D, 3) as convex_adam_pt returns it or
(3, H, W, D) as register_pair_device does, float32 or float64, read in place -- gives a device tensor of the same layout and dtype;
nothing is downloaded.  Coordinates are clamped to the grid (border padding); the arithmetic is float64 in a fixed order, so two calls give
the same bits.  There is no CPU path.
"""
import numpy as np
import torch

from ._lib import call, field_operand_from, ptr


def invert_field(disp, max_iters=50, tol=1e-4, return_info=False, device=None):
    """The inverse v of the displacement field `disp`: v(y) = -disp(y + v(y)), so that apply_convex(v, fixed) is the fixed image in the
    moving frame and compose_fields(disp, v) is (nearly) zero.

    Fixed-point iteration v <- -disp(y + v) from v = -disp, at most `max_iters` (1 .. 1000) times per voxel; a voxel stops as soon as a
    step moves it by at most `tol` voxels (max-norm; the default is a tenth of the 1e-3 voxel the package accepts between arithmetic
    variants), tol = 0 runs all iterations everywhere.  It converges where `disp` changes by less than one voxel per voxel (no folding).
    return_info=True also returns dict(residual, iters, not_converged, non_finite, max_residual): per voxel the max-norm of
    compose_fields(disp, v) and the iterations it ran (arrays like the result: numpy or device tensors), the number of voxels that never
    met `tol`, the number whose coordinates were not finite (they hold NaN), and the largest finite residual."""
    u, shape, cs, vs, f64, host = field_operand_from(disp, "disp", device)
    dev = u.device
    out_dtype = disp.dtype if not host else torch.float64
    v = torch.empty_like(u)
    residual = torch.empty(shape, dtype=torch.float64, device=dev) if return_info else None
    iters = torch.empty(shape, dtype=torch.uint8, device=dev) if return_info else None
    stats = torch.empty(3, dtype=torch.int64, device=dev) if return_info else None
    call(dev, "cvx_field_invert_f64", ptr(u), f64, cs, vs, shape[0], shape[1], shape[2], int(max_iters), float(tol), ptr(v), f64, cs, vs,
         ptr(residual), ptr(iters), ptr(stats))
    v = v.cpu().numpy() if host else v.to(out_dtype)
    if not return_info:
        return v
    s = stats.cpu()
    info = dict(residual=residual.cpu().numpy() if host else residual, iters=iters.cpu().numpy() if host else iters,
                not_converged=int(s[0]), non_finite=int(s[1]), max_residual=float(s[2:].view(torch.float64)[0]))
    return v, info


def compose_fields(first, second, device=None):
    """The single field equal to warping with `first` and then with `second` in apply_convex's convention:
    out(x) = second(x) + first(x + second(x)), so that apply_convex(second, apply_convex(first, img)) ~ apply_convex(out, img).
    Both fields live on the same grid.  Host inputs give a float64 numpy array; if `first` is a device tensor the result is a device
    tensor of its layout and dtype (`second` may use the other layout or element type)."""
    a, shape, acs, avs, a64, host = field_operand_from(first, "first", device)
    b, bshape, bcs, bvs, b64, _ = field_operand_from(second, "second", a.device)
    if bshape != shape or b.device != a.device:
        raise ValueError("compose_fields: first is %s on %s, second %s on %s" % (shape, a.device, bshape, b.device))
    out = torch.empty_like(a)
    call(a.device, "cvx_field_compose_f64", ptr(a), a64, acs, avs, ptr(b), b64, bcs, bvs, shape[0], shape[1], shape[2], ptr(out), a64, acs, avs)
    return out.cpu().numpy() if host else out.to(first.dtype)


def apply_convex_inverse(disp, fixed, **kw):
    """apply_convex(invert_field(disp, **kw), fixed): the fixed image (or a map drawn on it) sampled in the moving frame, linear
    interpolation in float64 like apply_convex.  Keywords: max_iters, tol, device."""
    from .apply_convex import apply_convex
    inv = invert_field(disp, **kw)
    if isinstance(inv, torch.Tensor) and inv.shape[-1] != 3:
        inv = inv.permute(1, 2, 3, 0)
    return apply_convex(inv, fixed, device=kw.get("device"))


def main(argv=None):
    """python -m convexadam_amd.fieldops --input_field disp.nii.gz --output_inverse inv.nii.gz [--max_iters 50] [--tol 1e-4]
    NIfTI through nifti_io, as apply_convex.main reads its field; prints the not-converged count and the largest residual."""
    import argparse
    from . import nifti_io
    ap = argparse.ArgumentParser()
    ap.add_argument("--input_field", required=True, help="input convex displacement field (.nii.gz) full resolution")
    ap.add_argument("--output_inverse", required=True, help="output inverse displacement field (.nii.gz)")
    ap.add_argument("--max_iters", type=int, default=50)
    ap.add_argument("--tol", type=float, default=1e-4)
    a = ap.parse_args(argv)
    disp = nifti_io.load_fdata(a.input_field).astype("float32")
    inv, info = invert_field(disp, max_iters=a.max_iters, tol=a.tol, return_info=True)
    nifti_io.save_image(inv.astype(np.float32), nifti_io.load_affine(a.input_field), a.output_inverse)
    print("inverse of %s: %d of %d voxels not converged to %g within %d iterations, %d non-finite, max residual %.6g voxel"
          % (a.input_field, info["not_converged"], int(np.prod(disp.shape[:3])), a.tol, a.max_iters, info["non_finite"], info["max_residual"]))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
