"""Times the preprocessing operators (convexadam_amd/prep.py, csrc/prep.hip) on the device at 160 x 192 x 224 and 512 x 512 x 300, on
random data and on a CT-like volume whose background is ONE value (the case the histogram kernels must not serialise on).

    python tools/time_prep.py [--reps 20] [--shapes 160x192x224,512x512x300]

Each call runs on resident float32 tensors and is bracketed by device events (the host's part of a call -- the ctypes calls, the
output allocation, and for the mask the one flag read per round -- is inside the figure); median of --reps after three warm-up calls.
For nnUNetCTnorm the line also gives the bytes the algorithm needs -- four reads and one write of the volume -- over the time, and that
rate's share of the 8.0 TB/s HBM peak.  The hole filling prints its round count.  A run without a HIP device fails."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd import prep  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def volumes(shape, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = torch.randn(shape, generator=g, device=dev) * 600.0 + 40.0
    # a body (an ellipsoid of soft tissue with a little bone) in air of one value
    ax = [torch.linspace(-1, 1, s, device=dev) for s in shape]
    r2 = (ax[0][:, None, None] / 0.8) ** 2 + (ax[1][None, :, None] / 0.7) ** 2 + (ax[2][None, None, :] / 0.9) ** 2
    body = r2 < 1.0
    ct = torch.where(body, torch.randn(shape, generator=g, device=dev) * 180.0 + 40.0, torch.full((), -1024.0, device=dev))
    ct = torch.where(body & (torch.rand(shape, generator=g, device=dev) < 0.01), torch.full((), 1800.0, device=dev), ct)
    return {"random": rnd.contiguous(), "ct-like": ct.contiguous()}, body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="160x192x224,512x512x300")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_prep.py measures on a HIP device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    props = {'mean': 93.25, 'sd': 217.625, 'percentile_00_5': -958.0, 'percentile_99_5': 1203.5}
    for spec in args.shapes.split(","):
        shape = tuple(int(v) for v in spec.split("x"))
        n = int(np.prod(shape))
        vols, body = volumes(shape, dev)
        print("== %s (%d voxels, %.1f MB as float32)" % (spec, n, 4e-6 * n), flush=True)
        for name, x in vols.items():
            def line(what, t, nbytes=None):
                extra = ""
                if nbytes:
                    rate = nbytes / (t[0] * 1e-3)
                    extra = "   %.2f TB/s of needed bytes = %.1f %% of the 8.0 TB/s HBM peak" % (rate * 1e-12, 100.0 * rate / HBM_PEAK)
                print("  %-8s %-34s median %8.3f ms  (min %.3f, max %.3f)%s" % (name, what, t[0], t[1], t[2], extra), flush=True)

            line("statistics of nnUNetCTnorm (3 reads)", timed(lambda: prep._stats(x, 1, (-1000.0, 1500.0), (0.005, 0.995)), args.reps), 3 * 4 * n)
            line("nnUNetCTnorm (4 reads + 1 write)", timed(lambda: prep.nnUNetCTnorm(x), args.reps), 5 * 4 * n)
            line("nnUNetNorm (3 reads + 1 write)", timed(lambda: prep.nnUNetNorm(x), args.reps), 4 * 4 * n)
            line("nnUNetNormProps (1 read + 1 write)", timed(lambda: prep.nnUNetNormProps(x, props), args.reps), 2 * 4 * n)
        # the mask of the body: air is zero, the body is not; a cavity inside is filled
        data = (vols["ct-like"] + 1024.0)[None].contiguous()
        lo = [s // 2 - s // 16 for s in shape]
        data[0, lo[0]:lo[0] + shape[0] // 8, lo[1]:lo[1] + shape[1] // 8, lo[2]:lo[2] + shape[2] // 8] = 0
        mask, _, rounds = prep._nonzero_mask(data)
        t = timed(lambda: prep.create_nonzero_mask(data), args.reps)
        print("  %-8s %-34s median %8.3f ms  (min %.3f, max %.3f)   %d rounds of sweeps, %d of %d voxels set" %
              ("body", "create_nonzero_mask", t[0], t[1], t[2], rounds, int(mask.sum()), n), flush=True)
        t = timed(lambda: prep.get_bbox_from_mask(mask), args.reps)
        print("  %-8s %-34s median %8.3f ms  (min %.3f, max %.3f)   box %s" % ("body", "get_bbox_from_mask (24 bytes down)", t[0], t[1], t[2],
                                                                            prep.get_bbox_from_mask(mask)), flush=True)
        for kind in ("ct", "nonzero"):
            t = timed(lambda: prep.normalise_and_crop(data[0], kind), args.reps)
            print("  %-8s %-34s median %8.3f ms  (min %.3f, max %.3f)" % ("body", "normalise_and_crop(kind=%r)" % kind, t[0], t[1], t[2]), flush=True)
        # a mask that needs many rounds: noise at density 0.6 (the complement is a maze)
        noise = (torch.rand((1,) + shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) < 0.6).float()
        rounds = prep._nonzero_mask(noise)[2]
        t = timed(lambda: prep.create_nonzero_mask(noise), max(3, args.reps // 4))
        print("  %-8s %-34s median %8.3f ms  (min %.3f, max %.3f)   %d rounds of sweeps" % ("noise", "create_nonzero_mask", t[0], t[1], t[2], rounds), flush=True)
        del vols, data, noise, mask, body
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
