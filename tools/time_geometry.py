"""Times the physical-space steps around a registration on the host (as the parent commit has them: device=None) and on the device
(csrc/geometry.hip), for a fixed image of 320 x 320 x 24 voxels at (0.5, 0.5, 3.6) mm and a moving image of 256 x 256 x 20 at
(0.6, 0.6, 4.0) mm whose axes are turned by 10 degrees about z.

    python tools/time_geometry.py [--reps 10] [--host-reps 2]

Prints, in ms: the host path's two resamplings (resample_img to 1 mm, resample_moving_to_fixed) and its carry + warp
(apply_convex_original_moving: three host resamplings, the rotation, an upload and the warp kernel), wall clock, best of --host-reps;
the device calls for the same steps on resident tensors, each bracketed by device events (so the host's part of a call -- two 3 x 3
solves, the ctypes call -- is inside the figure), median of --reps after two warm-up calls; and the device= keyword
of the public functions, wall clock with the uploads and downloads they include.  Then the largest differences between the two paths."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd import geometry  # noqa: E402
from convexadam_amd.apply_convex import apply_convex_original_moving  # noqa: E402
from convexadam_amd.convex_adam_utils import resample_img, resample_moving_to_fixed  # noqa: E402
from convexadam_amd.imageio import Image  # noqa: E402
from convexadam_amd.phantom import phantom  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def wall(fn, reps):
    best, out = float("inf"), None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    c, s = np.cos(np.deg2rad(10.0)), np.sin(np.deg2rad(10.0))
    fixed = Image(phantom((24, 320, 320), 1, 10).numpy(), (0.5, 0.5, 3.6))
    moving = Image(phantom((20, 256, 256), 1, 11).numpy(), (0.6, 0.6, 4.0), (4.0, -9.0, 2.0), (c, -s, 0, s, c, 0, 0, 0, 1))
    gf, gm = geometry.grid_of(fixed), geometry.grid_of(moving)
    gr = geometry.resampled_grid(gf, (1.0, 1.0, 1.0))
    shape = gr.size[::-1]
    g = torch.Generator().manual_seed(0)
    field32 = 2.0 * torch.nn.functional.interpolate(torch.randn(1, 3, 3, 3, 3, generator=g), size=shape, mode="trilinear", align_corners=True)[0]
    field_host = field32.permute(1, 2, 3, 0).double().contiguous().numpy()            # (H, W, D, 3) float64, as convex_adam_pt returns it
    print("fixed %s @ %s -> %s @ 1 mm; moving %s @ %s, 10 degrees about z" % (gf.size, gf.spacing, gr.size, gm.size, gm.spacing), flush=True)

    # host path, as the parent commit has it
    t_fix, fixed_r = wall(lambda: resample_img(fixed, (1.0, 1.0, 1.0)), args.host_reps)
    t_mov, moving_r = wall(lambda: resample_moving_to_fixed(fixed_r, moving), args.host_reps)
    t_carry, warped_host = wall(lambda: apply_convex_original_moving(field_host, moving, fixed, fixed_r), args.host_reps)
    print("host   (device=None, wall clock): resample fixed %.1f ms, moving onto fixed %.1f ms, carry + warp %.1f ms" % (t_fix, t_mov, t_carry), flush=True)

    # device calls on resident tensors
    fx, mv = geometry.upload(fixed, dev), geometry.upload(moving, dev)
    f32, f64 = field32.to(dev).contiguous(), torch.from_numpy(field_host).to(dev)
    k_fix = timed(lambda: geometry.resample_device(fx, gf, gr), args.reps)
    k_mov = timed(lambda: geometry.resample_device(mv, gm, gr), args.reps)
    k_both32 = timed(lambda: geometry.rescale_displacement_field_device(f32, gm, gf, gr, moving=mv), args.reps)
    k_both64 = timed(lambda: geometry.rescale_displacement_field_device(f64, gm, gf, gr, moving=mv), args.reps)
    k_carry = timed(lambda: geometry.rescale_displacement_field_device(f64, gm, gf, gr), args.reps)
    k_warp = timed(lambda: geometry.rescale_displacement_field_device(f64, gm, gf, gr, moving=mv, want_field=False), args.reps)
    print("device (calls on resident tensors, device events): resample fixed %.4f ms, moving onto fixed %.4f ms, carry + warp %.4f ms (float32 planar field) "
          "%.4f ms (float64 interleaved field); carry alone %.4f ms, warp alone %.4f ms" % (k_fix, k_mov, k_both32, k_both64, k_carry, k_warp), flush=True)

    # the device= keyword: the same public functions, uploads and downloads included
    w_fix, fixed_d = wall(lambda: resample_img(fixed, (1.0, 1.0, 1.0), device=dev), args.reps)
    w_mov, moving_d = wall(lambda: resample_moving_to_fixed(fixed_d, moving, device=dev), args.reps)
    w_carry, warped_dev = wall(lambda: apply_convex_original_moving(field_host, moving, fixed, fixed_d, device=dev), args.reps)
    print("device (device= keyword, wall clock with transfers): resample fixed %.2f ms, moving onto fixed %.2f ms, carry + warp %.2f ms" % (w_fix, w_mov, w_carry), flush=True)
    print("largest differences host - device: fixed %.3g, moving %.3g, warped %.3g" % (
        float(np.abs(fixed_r.array.astype(np.float64) - fixed_d.array).max()), float(np.abs(moving_r.array.astype(np.float64) - moving_d.array).max()),
        float(np.abs(warped_host.array.astype(np.float64) - warped_dev.array).max())), flush=True)


if __name__ == "__main__":
    main()
