"""Times the cubic B-spline operators (csrc/spline.hip) at 160 x 192 x 224 (--small: 48^3, for a quick check).

    python tools/time_spline.py [--reps 9] [--inner 5] [--small] [--no-scipy] [--passes DIR]

In ONE process, on resident tensors, alternating: the whole prefilter (cvx_spline_prefilter_f64: float32 samples, float64 samples, in
place), the warp (cvx_map_coordinates_cubic_f64, a smooth float32 field of about 4 voxels in the (3, H, W, D) layout), the resampling
(cvx_resample_cubic_f64, a grid shifted by a fraction of a voxel), their linear counterparts (warp_device's float64 twin and
cvx_resample_linear_f64), and a device-to-device copy of the same float64 volume -- the yardstick: every pass must at least read and write
the volume once.  A stamp brackets --inner calls with device events behind a device synchronisation, --reps rounds after two warm-up
rounds; medians and the spread (min .. max) per call are printed, and each as a multiple of the copy.  scipy.ndimage.map_coordinates
(order=3) warps the same volume with the same field once on the host, and the two results are compared.

--passes DIR: the three axis passes separately.  They are three kernels of one call (k_spline_strided<float> = axis 0 for float32 samples,
k_spline_strided<double> = axis 1, k_spline_contig = axis 2), so their times come from `rocprofv3 --kernel-trace --stats --output-format csv` around a child
process of this script that only calls the prefilter (a run of its own, tracing slows the host), written under DIR; each pass is printed
as a multiple of the copy time the parent measured in the same call.  A run without a HIP device fails."""
import argparse
import csv
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd import geometry  # noqa: E402
from convexadam_amd._lib import call, lib, ptr, spline_lib  # noqa: E402
from convexadam_amd.spline import spline_coefficients, warp_cubic  # noqa: E402

PASSES = (("axis 0 (strided, float32 samples in)", "k_spline_strided<float>"), ("axis 1 (strided, in place)", "k_spline_strided<double>"),
          ("axis 2 (contiguous, staged through LDS)", "k_spline_contig"))


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


def volume(shape, dev):
    g = torch.Generator().manual_seed(11)
    return (300.0 * torch.rand(shape, generator=g, dtype=torch.float64)).to(dev)


def passes_child(shape, calls):
    dev = torch.device("cuda:0")
    src = volume(shape, dev).float()
    for _ in range(calls):
        spline_coefficients(src)
    torch.cuda.synchronize()


def kernel_stats(directory):
    """{kernel name: (calls, average ns)} from the *kernel_stats.csv rocprofv3 wrote under `directory`"""
    out = {}
    for root, _, files in os.walk(directory):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                for r in csv.DictReader(open(os.path.join(root, f))):
                    out[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--passes", metavar="DIR")
    ap.add_argument("--passes-child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_spline.py measures on a HIP device; there is nothing to time without one"
    shape = (48, 48, 48) if args.small else (160, 192, 224)
    if args.passes_child:
        return passes_child(shape, args.passes_child)
    dev = torch.device("cuda:0")
    V = shape[0] * shape[1] * shape[2]
    vol64 = volume(shape, dev)
    vol32 = vol64.float()
    g = torch.Generator().manual_seed(3)
    field = (4.0 * F.interpolate(torch.randn(1, 3, 3, 3, 4, generator=g), size=shape, mode="trilinear", align_corners=False))[0].contiguous().to(dev)
    coef = spline_coefficients(vol64)
    scratch, dst = vol64.clone(), torch.empty_like(vol64)
    grid = geometry.Grid(shape[::-1], (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).reshape(-1)))
    shifted = geometry.Grid(shape[::-1], (1.0, 1.0, 1.0), (0.3, -0.4, 0.2), tuple(np.eye(3).reshape(-1)))
    m12 = geometry._doubles(*geometry.index_map(grid, shifted))
    out64 = torch.empty_like(vol64)
    disp64 = field.permute(1, 2, 3, 0).contiguous().double()
    spline_lib()

    def in_place():
        scratch.copy_(vol64)
        call(dev, "cvx_spline_prefilter_f64", ptr(scratch), 1, *shape, ptr(scratch))

    forms = {
        "copy, device to device (float64 volume)": lambda: dst.copy_(vol64),
        "prefilter, float32 samples": lambda: spline_coefficients(vol32),
        "prefilter, float64 samples": lambda: spline_coefficients(vol64),
        "prefilter, in place (+ the copy that refills it)": in_place,
        "cubic warp (coefficients given)": lambda: warp_cubic(coef, field, prefiltered=True),
        "linear warp (cvx_map_coordinates_linear_f64)": lambda: call(dev, "cvx_map_coordinates_linear_f64", ptr(vol64), ptr(disp64), *shape, ptr(out64)),
        "cubic resampling (coefficients given)": lambda: call(dev, "cvx_resample_cubic_f64", ptr(coef), *shape, ptr(out64), 1, *shape, m12, 0.0),
        "linear resampling (cvx_resample_linear_f64)": lambda: call(dev, "cvx_resample_linear_f64", ptr(vol64), 1, *shape, ptr(out64), 1, *shape, m12, 0.0),
    }
    lib()
    times = {k: [] for k in forms}
    for r in range(args.reps + 2):
        for k, fn in forms.items():
            t = stamp(fn, args.inner)
            if r >= 2:
                times[k].append(t)
    copy = spread(times["copy, device to device (float64 volume)"])[0]
    print("volume %s: %.1f MB as float64, the field %.1f MB; %d rounds of %d calls after 2 warm-up rounds" % (shape, 8e-6 * V, 12e-6 * V, args.reps, args.inner))
    for k in forms:
        med, lo, hi = spread(times[k])
        print("  %-52s median %8.3f ms  (min %.3f, max %.3f)   %6.2f x the copy" % (k, med, lo, hi, med / copy), flush=True)
    print("  the copy moves 16 bytes per voxel: %.2f TB/s" % (16e-12 * V / (copy * 1e-3)))
    if not args.no_scipy:
        from scipy import ndimage
        got = warp_cubic(vol64, field).cpu().numpy()
        ident = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), 0)
        coords = field.cpu().numpy().astype(np.float64) + ident
        t0 = time.perf_counter()
        want = ndimage.map_coordinates(vol64.cpu().numpy(), coords, order=3, mode="constant", cval=0.0)
        host = time.perf_counter() - t0
        both = spread(times["prefilter, float64 samples"])[0] + spread(times["cubic warp (coefficients given)"])[0]
        print("  scipy.ndimage.map_coordinates(order=3) on the host: %.2f s; device prefilter + warp %.3f ms (%.0f x); largest difference %.3g of max|volume|"
              % (host, both, 1e3 * host / both, float(np.abs(got - want).max()) / float(vol64.abs().max())), flush=True)
    if args.passes:
        os.makedirs(args.passes, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.passes, "-o", "spline", "--", sys.executable, os.path.abspath(__file__),
               "--passes-child", "20"] + (["--small"] if args.small else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        stats = kernel_stats(args.passes)
        if r.returncode != 0 or not stats:
            print("  rocprofv3 run failed (exit %d):\n%s" % (r.returncode, r.stdout[-2000:]))
            return 1
        print("  the three passes of the prefilter (float32 samples), kernel times from rocprofv3 --kernel-trace --stats, 20 calls in a child process:")
        total = 0.0
        for label, name in PASSES:
            hit = [v for k, v in stats.items() if k.replace("cvx::", "").replace("void ", "").startswith(name)]
            if not hit:
                print("    %-44s not found among %s" % (label, sorted(stats)))
                continue
            calls, avg = hit[0]
            total += avg * 1e-6
            print("    %-44s %8.3f ms per launch (%d launches)   %6.2f x the copy" % (label, avg * 1e-6, calls, avg * 1e-6 / copy))
        print("    sum %.3f ms; the whole call by device events: %.3f ms" % (total, spread(times["prefilter, float32 samples"])[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
