"""Times the fused warp + joint histogram (csrc/simhist.hip, cvx_joint_hist_f32) against what a user can write without it: warp_device,
the same float32 bin arithmetic in torch, then torch.bincount.

    python tools/time_simhist.py [--reps 9] [--inner 5] [--small]

Two pairs at 160 x 192 x 224 (convexadam_amd/phantom.py; --small: 48^3, for a quick check): the textured deformed_pair and the
zero_background_pair, where one cell holds two thirds of the voxels; the moving image passes through the non-monotone remap
exp(-1.3 x) + 0.1 x^2.  Bins 32 x 32 (four LDS copies per workgroup) and 128 x 128 (one copy, exactly the LDS limit), without a field and
with a smooth float32 field of about 4 voxels in the (3, H, W, D) layout.  Both forms get the range as a device tensor; the range pass is
timed beside them.  The forms alternate in ONE process on resident tensors; a stamp brackets --inner calls with device events behind a
device synchronisation, --reps rounds after two warm-up rounds; medians and the spread (min .. max) per call are printed, their ratio, and
the bytes the fused form must move -- both images, the field, the histogram -- over its time against the 8 TB/s HBM peak.  The histograms of
the two forms are compared.  A run without a HIP device fails."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd.phantom import deformed_pair, zero_background_pair  # noqa: E402
from convexadam_amd.similarity import joint_histogram, value_range  # noqa: E402
from convexadam_amd.ssim import warp_device  # noqa: E402

HBM_PEAK = 8.0e12


def eager_bins(x, lo, hi, nb):
    scale = torch.where(hi > lo, nb / (hi - lo), torch.zeros_like(lo))
    scale = torch.where(torch.isfinite(scale), scale, torch.zeros_like(scale))
    return ((x - lo) * scale).clamp_(0, nb - 1).long()


def eager_hist(fixed, moving, bins, rng, disp=None):
    """the parent commit's operators: the warped volume, the bins of both images, bincount"""
    b = warp_device(moving, disp) if disp is not None else moving
    cell = eager_bins(fixed.reshape(-1), rng[0], rng[1], bins) * bins + eager_bins(b.reshape(-1), rng[2], rng[3], bins)
    return torch.bincount(cell, minlength=bins * bins).reshape(bins, bins)


def stamp(fn, inner):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_simhist.py measures on a HIP device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    shape = (48, 48, 48) if args.small else (160, 192, 224)
    V = shape[0] * shape[1] * shape[2]
    g = torch.Generator().manual_seed(3)
    field = (4.0 * F.interpolate(torch.randn(1, 3, 3, 3, 4, generator=g), size=shape, mode="trilinear", align_corners=False))[0].contiguous().to(dev)
    print("pairs at %s: %.1f MB per image, the field %.1f MB" % (shape, 4e-6 * V, 12e-6 * V), flush=True)
    for name, make in (("textured", deformed_pair), ("zero background", zero_background_pair)):
        fix, mov = make(shape)
        fix = fix.to(dev).contiguous()
        mov = (torch.exp(-1.3 * mov.double()) + 0.1 * mov.double() ** 2).float().to(dev).contiguous()
        for with_field in (False, True):
            disp = field if with_field else None
            rng = value_range(fix, mov, disp=disp)
            for bins in (32, 128):
                forms = {"fused": lambda: joint_histogram(fix, mov, bins, disp=disp, value_range=rng),
                         "eager": lambda: eager_hist(fix, mov, bins, rng, disp),
                         "range": lambda: value_range(fix, mov, disp=disp)}
                times = {k: [] for k in forms}
                for r in range(args.reps + 2):
                    for k, fn in forms.items():
                        t = stamp(fn, args.inner)
                        if r >= 2:
                            times[k].append(t)
                fused, eager, rpass = spread(times["fused"]), spread(times["eager"]), spread(times["range"])
                h, info = joint_histogram(fix, mov, bins, disp=disp, value_range=rng, return_info=True)
                same = bool(torch.equal(h, eager_hist(fix, mov, bins, rng, disp)))
                nbytes = 8 * V + (12 * V if with_field else 0) + 8 * bins * bins
                print("%s pair, %s, %d x %d bins, %d rounds of %d calls after 2 warm-up rounds (largest cell %.1f %% of the voxels; stats %s):"
                      % (name, "field" if with_field else "no field", bins, bins, args.reps, args.inner, 100.0 * float(h.max()) / V, info["stats"].tolist()))
                print("  fused call (cvx_joint_hist_f32)    median %8.3f ms  (min %.3f, max %.3f)   %.1f MB: %.2f TB/s = %.1f %% of the 8.0 TB/s HBM peak"
                      % (fused + (1e-6 * nbytes, 1e-12 * nbytes / (fused[0] * 1e-3), 100.0 * nbytes / (fused[0] * 1e-3) / HBM_PEAK)))
                print("  eager: warp_device, bins, bincount median %8.3f ms  (min %.3f, max %.3f)   ratio eager / fused %.2f;  histograms equal: %s"
                      % (eager + (eager[0] / fused[0], same)))
                print("  range pass (cvx_sim_range_f32)     median %8.3f ms  (min %.3f, max %.3f)" % rpass, flush=True)


if __name__ == "__main__":
    main()
