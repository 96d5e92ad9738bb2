"""The end-to-end inputs of the translation tests (tests/test_gpu_translation.py), in one place so that the CPU oracle can be run on the
very same images.  Test infrastructure only: the product never imports it.

All of them: phantom (48, 40, 44) at 1 mm as the fixed image, the moving image that volume rolled by whole voxels.

    known_shift    the inputs of test_translation_wrapper_and_original_moving_warp_on_metaimage_files: rolled by (3, 0, -2) (z, y, x);
                   the host path gives (-2, 0, 3) mm (x, y, z)
    segmentation   ... with a uint8 ellipsoid (labels 1 and 2) given on a 2 mm grid of its own
    shift_2_1_-1   rolled by (2, 1, -1), no segmentation
    moving_1x1x2   the moving image at spacing (1, 1, 2): every second slice of the volume rolled by (2, 1, -1)

TIE_FREE names the cases whose host-path value before rounding (mean displacement / spacing, per axis) lies at least 0.25 from a
half-integer; the CPU oracle pipeline (oracle.convex_adam_pipeline, bit-identical to the device's exact mode) gives, z, y, x:

    known_shift    2.616 -0.001 -1.752   0.116 from 2.5: NOT tie-free.  The mean over the whole volume of a roll by 3 is about 0.87 x 3
                   (the field fades towards the faces the roll wraps around), whatever the seeds: 24 structure seeds and 16 noise seeds
                   of the phantom gave 2.57 .. 2.62.  The case is kept for its known answer and the reference test's own criterion.
    segmentation   2.882 -0.003 -1.905   0.38
    shift_2_1_-1   1.759  0.911 -0.923   0.26
    moving_1x1x2   0.896  0.919 -0.916   0.40   (rolled by 3 or 4 along z the value is 1.3 or 1.7 voxels of 2 mm: not tie-free either)
"""
import numpy as np

from convexadam_amd.imageio import Image
from convexadam_amd.phantom import phantom

NAMES = ("known_shift", "segmentation", "shift_2_1_-1", "moving_1x1x2")
TIE_FREE = ("segmentation", "shift_2_1_-1", "moving_1x1x2")
SHAPE = (48, 40, 44)


def ellipsoid_2mm():
    """uint8 labels on a 2 mm grid whose origin lies half a millimetre off the fixed image's: 2 inside the inner ellipsoid, 1 in the shell"""
    nz, ny, nx = 23, 19, 21
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    r2 = ((z - 11.0) / 8.0) ** 2 + ((y - 9.0) / 6.5) ** 2 + ((x - 10.0) / 7.0) ** 2
    lab = np.where(r2 <= 0.45, 2, np.where(r2 <= 1.0, 1, 0)).astype(np.uint8)
    return Image(lab, (2.0, 2.0, 2.0), (0.5, 0.5, 0.5))


def make(name):
    """-> (fixed, moving, segmentation or None, applied roll (z, y, x) in voxels of the 1 mm volume)"""
    vol = phantom(SHAPE, 5, 50).numpy()
    fixed = Image(vol, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    shift = (3, 0, -2) if name in ("known_shift", "segmentation") else (2, 1, -1)
    rolled = np.roll(vol, shift, (0, 1, 2))
    if name == "moving_1x1x2":
        return fixed, Image(rolled[::2].copy(), (1.0, 1.0, 2.0), (0.0, 0.0, 0.0)), None, shift
    return fixed, Image(rolled, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), (ellipsoid_2mm() if name == "segmentation" else None), shift
