"""Translation-only registration wrapper around convex_adam_pt (reference: src/convexAdam/convex_adam_translation.py:12-131).

Host-side geometry on SimpleITK images; the registration itself runs through convexadam_amd.convex_adam_MIND.convex_adam_pt
(HIP).  SimpleITK is imported when a function that needs it is called, so the module also imports on hosts without it.
With device= (a HIP device) the resamplings, the registration and the masked mean of the field all run on the device and 32 bytes come
back (csrc/geometry.hip, csrc/fieldmean.hip); device=None is the host path as it always was.

    index_translation_to_world_translation(index_translation, direction)        :12-29
    apply_translation(moving_image, translation_ijk)                            :32-54
    convex_adam_translation(fixed_image, moving_image, segmentation=None, co_moving_images=None, device=None)    :57-114
    convex_adam_translation_from_file(...)                                      :117-146
"""
import numpy as np

from .convex_adam_MIND import convex_adam_pt
from .convex_adam_utils import _is_builtin, _sitk, resample_img, resample_moving_to_fixed


def index_translation_to_world_translation(index_translation, direction):
    """Translation along the image axes (i, j, k; mm) -> world axes (x, y, z; mm): direction-cosine matrix times the vector."""
    n = int(np.sqrt(len(direction)))
    return np.array(direction).reshape((n, n)) @ np.array(index_translation)


def apply_translation(moving_image, translation_ijk=(0, 0, 0)):
    """Copy of `moving_image` whose origin is shifted by the world-space equivalent of `translation_ijk` (mm along the image axes)."""
    moved = moving_image.copy() if _is_builtin(moving_image) else _sitk().Image(moving_image)
    shift = index_translation_to_world_translation(translation_ijk, moved.GetDirection()[0:9])
    origin = np.array(moved.GetOrigin(), dtype=float)
    origin[0:3] -= shift
    moved.SetOrigin(tuple(origin))
    return moved


def mean_to_translation(mean_zyx, spacing_xyz):
    """Mean displacement (z, y, x; voxels of a 1 mm grid) -> whole-voxel translation of an image with spacing `spacing_xyz`, in mm as
    (x, y, z)   (:100-103)."""
    spacing_zyx = np.array(list(spacing_xyz)[::-1])
    voxels = np.round(mean_zyx / spacing_zyx, decimals=0)
    return tuple(list((voxels * spacing_zyx)[::-1]))


def field_to_translation(displacement_field, spacing_xyz, mask=None):
    """Mean displacement (over `mask` if given) of a (H,W,D,3) field in voxels of a 1 mm grid -> whole-voxel translation of an image
    with spacing `spacing_xyz`, returned in mm as (x, y, z)   (:88-103)."""
    field = np.asarray(displacement_field)
    mean_zyx = np.mean(field[mask], axis=0) if mask is not None else np.mean(field, axis=(0, 1, 2))
    return mean_to_translation(mean_zyx, spacing_xyz)


def register_on_1mm_device(fixed_image, moving_image, device="cuda"):
    """One upload per image, the fixed image resampled to 1 mm and the moving image onto that grid (resample_device), register_pair_device
    with convex_adam_pt's defaults.  Returns (field (3, H, W, D) float32 on the device, the 1 mm grid)."""
    import torch
    from . import geometry
    from .convex_adam_MIND import register_pair_device
    from .imageio import get_array
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("device=%s: the device path runs only on a HIP (ROCm 'cuda') device; device=None is the host path" % (device,))
    gf, gm = geometry.grid_of(fixed_image), geometry.grid_of(moving_image)
    gr = geometry.resampled_grid(gf, (1.0, 1.0, 1.0))
    fix_r = geometry.resample_device(geometry.upload(get_array(fixed_image), dev), gf, gr).to(torch.float32)
    mov_r = geometry.resample_device(geometry.upload(get_array(moving_image), dev), gm, gr).to(torch.float32)
    field = register_pair_device(fix_r, mov_r)
    if tuple(field.shape) != (3,) + tuple(fix_r.shape):
        raise ValueError("convex_adam_translation needs the full-resolution field, got %s for images of %s" % (tuple(field.shape), tuple(fix_r.shape)))
    return field, gr


def translation_mean_device(fixed_image, moving_image, segmentation=None, device="cuda"):
    """The device path up to the mean: register_on_1mm_device, one field_mean_device with the float16 round trip of convex_adam_pt's
    default dtype and the segmentation on its own grid, one 32-byte download.  Returns (mean_zyx float64[3], count).  Anything with
    SimpleITK's accessors goes this way.  An empty mask or a non-finite mean raises ValueError."""
    import torch
    from . import geometry
    from .imageio import get_array
    field, gr = register_on_1mm_device(fixed_image, moving_image, device)
    seg = geometry.upload(get_array(segmentation), field.device) if segmentation is not None else None
    seg_grid = geometry.grid_of(segmentation) if segmentation is not None else None
    both = geometry.field_mean_buffer(field, gr, seg=seg, seg_grid=seg_grid, quantize=torch.float16).cpu()     # three sums and the count
    n = int(both[3:].view(torch.int64)[0])
    if n == 0:
        raise ValueError("convex_adam_translation: the segmentation is empty on the fixed image's 1 mm grid (no voxel above zero)")
    mean_zyx = both[:3].numpy() / np.float64(n)
    if not np.all(np.isfinite(mean_zyx)):
        raise ValueError("convex_adam_translation: the mean displacement is not finite (%s)" % (mean_zyx,))
    return mean_zyx, n


def convex_adam_translation(fixed_image, moving_image, segmentation=None, co_moving_images=None, device=None):
    """Register `moving_image` to `fixed_image` with convex_adam_pt on a 1 mm grid, reduce the field to one whole-voxel translation
    (mean over the segmentation if given) and apply it to the moving image and to the co-moving images.
    Returns (translation_xyz in mm, moved image, moved co-moving images).
    device: None = resampling, thresholding and the mean on the host, as in the reference; a HIP device = all of it on the device
    (translation_mean_device); an empty segmentation or a non-finite mean then raises ValueError."""
    if device is not None:
        mean_zyx, _ = translation_mean_device(fixed_image, moving_image, segmentation, device)
        translation_xyz = mean_to_translation(mean_zyx, moving_image.GetSpacing())
    else:
        fixed_1mm = resample_img(fixed_image, spacing=(1.0, 1.0, 1.0))
        moving_1mm = resample_moving_to_fixed(fixed_1mm, moving_image)
        field = convex_adam_pt(img_fixed=fixed_1mm, img_moving=moving_1mm)
        mask = None
        if segmentation is not None:
            # linear resampling blurs the labels: everything above zero counts
            from .imageio import get_array
            mask = get_array(resample_moving_to_fixed(moving=segmentation, fixed=fixed_1mm)) > 0
        translation_xyz = field_to_translation(field, moving_image.GetSpacing(), mask)
    moved = apply_translation(moving_image=moving_image, translation_ijk=translation_xyz)
    if co_moving_images is not None:
        for i, image in enumerate(co_moving_images):
            co_moving_images[i] = apply_translation(moving_image=image, translation_ijk=translation_xyz)
    return translation_xyz, moved, co_moving_images


def convex_adam_translation_from_file(fixed_path="/input/fixed.mha", moving_path="/input/moving.mha",
                                      segmentation_path="/input/segmentation.nii.gz", moving_output_path="/output/moving_warped.mha",
                                      co_moving_paths=None, co_moving_output_paths=None, device=None):
    """File front end (:117-146).  SimpleITK reads and writes when it is installed; otherwise the built-in MetaImage / NIfTI readers
    and the MetaImage writer of convexadam_amd.imageio do.  device: as for convex_adam_translation."""
    try:
        import SimpleITK as sitk  # noqa: N813
        read, write = (lambda p: sitk.ReadImage(str(p))), (lambda img, p: sitk.WriteImage(img, str(p)))
    except ImportError:
        from .imageio import read_image, write_mha
        read, write = (lambda p: read_image(str(p))), (lambda img, p: write_mha(img, str(p)))
    co = [read(p) for p in co_moving_paths] if co_moving_paths is not None else None
    translation_xyz, moved, co = convex_adam_translation(
        fixed_image=read(fixed_path), moving_image=read(moving_path),
        segmentation=read(segmentation_path) if segmentation_path is not None else None, co_moving_images=co, device=device)
    write(moved, moving_output_path)
    if co is not None:
        for image, path in zip(co, co_moving_output_paths):
            write(image, path)
    return translation_xyz


def main(argv=None):
    """python -m convexAdam.convex_adam_translation (convex_adam_translation.py:149-166)."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixed_path", default="/input/fixed.mha")
    ap.add_argument("--moving_path", default="/input/moving.mha")
    ap.add_argument("--segmentation_path", default=None)
    ap.add_argument("--moving_output_path", default="/output/moving_warped.mha")
    ap.add_argument("--co_moving_paths", nargs="+", default=None)
    ap.add_argument("--co_moving_output_paths", nargs="+", default=None)
    ap.add_argument("--device", default=None, help="a HIP device (e.g. cuda): resampling, registration and the masked mean on the device; default: the host path")
    a = ap.parse_args(argv)
    print(convex_adam_translation_from_file(a.fixed_path, a.moving_path, a.segmentation_path, a.moving_output_path, a.co_moving_paths,
                                            a.co_moving_output_paths, device=a.device))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
