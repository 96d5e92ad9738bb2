"""Times convex_adam_translation on the host path (as the parent commit has it: device=None) and on the device path (device=...), on the
geometry of tools/time_geometry.py: a fixed image of 320 x 320 x 24 voxels at (0.5, 0.5, 3.6) mm, a moving image of 256 x 256 x 20 at
(0.6, 0.6, 4.0) mm whose axes are turned by 10 degrees about z, and a uint8 segmentation on the moving image's grid.

    python tools/time_translation.py [--reps 10] [--host-reps 2]

Prints, in ms: the two paths end to end (wall clock, with the uploads and downloads they include; best of --host-reps / of --reps) and the
translations they return; then cvx_field_mean_f64 alone on resident tensors, bracketed by device events (the host's part of a call -- a
3 x 3 solve, the ctypes call -- is inside the figure), median of --reps after two warm-up calls: on the registration's field (all voxels;
a byte mask; the segmentation in its own grid) and on a float32 planar field of the benchmark's size, 160 x 192 x 224, with the bytes it
reads and the rate that makes, for one call and for 50 calls in a row between one pair of events."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_geometry import timed, wall  # noqa: E402

from convexadam_amd import geometry  # noqa: E402
from convexadam_amd.convex_adam_translation import convex_adam_translation, register_on_1mm_device  # noqa: E402
from convexadam_amd.imageio import Image  # noqa: E402
from convexadam_amd.phantom import phantom  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    c, s = np.cos(np.deg2rad(10.0)), np.sin(np.deg2rad(10.0))
    fixed = Image(phantom((24, 320, 320), 1, 10).numpy(), (0.5, 0.5, 3.6))
    direction = (c, -s, 0, s, c, 0, 0, 0, 1)
    moving = Image(phantom((20, 256, 256), 1, 11).numpy(), (0.6, 0.6, 4.0), (4.0, -9.0, 2.0), direction)
    z, y, x = np.meshgrid(np.arange(20), np.arange(256), np.arange(256), indexing="ij")
    seg = Image((((z - 10) / 8.0) ** 2 + ((y - 128) / 90.0) ** 2 + ((x - 128) / 100.0) ** 2 <= 1.0).astype(np.uint8), moving.GetSpacing(),
                moving.GetOrigin(), direction)
    gr = geometry.resampled_grid(geometry.grid_of(fixed), (1.0, 1.0, 1.0))
    print("fixed %s @ %s -> %s @ 1 mm; moving and segmentation %s @ %s, 10 degrees about z" % (
        fixed.GetSize(), fixed.GetSpacing(), gr.size, moving.GetSize(), moving.GetSpacing()), flush=True)

    for name, sg in (("no segmentation", None), ("segmentation", seg)):
        t_host, r_host = wall(lambda: convex_adam_translation(fixed, moving, segmentation=sg), args.host_reps)
        t_dev, r_dev = wall(lambda: convex_adam_translation(fixed, moving, segmentation=sg, device=dev), args.reps)
        print("%s: host path (device=None) %.1f ms -> %s; device path %.2f ms -> %s" % (name, t_host, r_host[0], t_dev, r_dev[0]), flush=True)

    # the reduction alone, on resident tensors
    field, _ = register_on_1mm_device(fixed, moving, dev)
    seg_d, sgrid = geometry.upload(seg, dev), geometry.grid_of(seg)
    mask = geometry.resample_device(seg_d, sgrid, gr) > 0
    half = torch.float16
    k_all = timed(lambda: geometry.field_mean_device(field, gr, quantize=half), args.reps)
    k_mask = timed(lambda: geometry.field_mean_device(field, gr, mask=mask, quantize=half), args.reps)
    k_seg = timed(lambda: geometry.field_mean_device(field, gr, seg=seg_d, seg_grid=sgrid, quantize=half), args.reps)
    k_two = timed(lambda: geometry.field_mean_device(field, gr, mask=geometry.resample_device(seg_d, sgrid, gr) > 0, quantize=half), args.reps)
    print("field mean on the %s field (device events): all voxels %.4f ms, byte mask %.4f ms, segmentation in its own grid %.4f ms "
          "(resample_device, > 0, byte mask: %.4f ms)" % (tuple(field.shape), k_all, k_mask, k_seg, k_two), flush=True)
    big = torch.randn(3, 160, 192, 224, device=dev)
    gb = geometry.Grid((224, 192, 160), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 0, 0, 0, 1, 0, 0, 0, 1))
    k_big = timed(lambda: geometry.field_mean_device(big, gb, quantize=half), max(args.reps, 20))
    k_row = timed(lambda: [geometry.field_mean_device(big, gb, quantize=half) for _ in range(50)], args.reps) / 50
    nbytes = big.numel() * 4
    print("field mean on a float32 (3, 160, 192, 224) field, %.1f MB read once: one call %.4f ms = %.2f TB/s; 50 calls in a row %.4f ms each = "
          "%.2f TB/s (both launches and the host's part of a call included)" % (nbytes / 1e6, k_big, nbytes / (k_big * 1e-3) / 1e12, k_row,
                                                                                 nbytes / (k_row * 1e-3) / 1e12), flush=True)


if __name__ == "__main__":
    main()
