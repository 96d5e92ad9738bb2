"""Times the fused field inversion (csrc/fieldops.hip, one launch) against what a user can write without it: the same fixed-point
iteration as an eager PyTorch loop of F.grid_sample calls (border padding, align_corners=True, float32), one launch chain per iteration.

    python tools/time_fieldops.py [--reps 9] [--iters 20] [--small]

The input is a field of the benchmark pair: deformed_pair at 160 x 192 x 224 (convexadam_amd/phantom.py) registered with the defaults of
convex_adam_pt, the (3, H, W, D) float32 device tensor register_pair_device returns (--small: 40 x 36 x 44, for a quick check).  Both
forms run --iters iterations at tol = 0 on resident tensors; the two alternate in ONE process, each call bracketed by device events behind
a device synchronisation, --reps rounds after two warm-up rounds; medians and the spread (min .. max) are printed, and the bytes the fused
form needs -- u read once, v written once -- over its time.  Then the field's own convergence at the defaults of invert_field (50
iterations, tol = 1e-4): iterations, not-converged fraction, largest residual; and the largest difference between the two forms' results.
A run without a HIP device fails."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd.convex_adam_MIND import register_pair_device  # noqa: E402
from convexadam_amd.fieldops import compose_fields, invert_field  # noqa: E402
from convexadam_amd.phantom import deformed_pair  # noqa: E402

HBM_PEAK = 8.0e12


def eager_invert(u, iters):
    """v <- -u(y + v), u (3, H, W, D) float32 in voxels: what a user writes today.  grid_sample wants (x, y, z) = (axis 2, 1, 0) in [-1, 1]."""
    _, H, W, D = u.shape
    dev = u.device
    ident = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device=dev) for n in (H, W, D)], indexing="ij"), 0)
    scale = torch.tensor([2.0 / max(n - 1, 1) for n in (H, W, D)], device=dev).view(3, 1, 1, 1)
    src = u[None]
    v = -u
    for _ in range(iters):
        g = ((ident + v) * scale - 1.0).flip(0).permute(1, 2, 3, 0)[None]
        v = -F.grid_sample(src, g, mode="bilinear", padding_mode="border", align_corners=True)[0]
    return v


def stamp(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_fieldops.py measures on a HIP device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    shape = (40, 36, 44) if args.small else (160, 192, 224)
    fix, mov = deformed_pair(shape, 0, 4.0)
    u = register_pair_device(fix.to(dev).contiguous(), mov.to(dev).contiguous()).contiguous()
    V = shape[0] * shape[1] * shape[2]
    print("field %s float32 of the benchmark pair at %s: %.1f MB, largest displacement %.2f voxels" % (tuple(u.shape), shape, 12e-6 * V, float(u.abs().max())),
          flush=True)

    forms = {"fused": lambda: invert_field(u, max_iters=args.iters, tol=0.0), "eager": lambda: eager_invert(u, args.iters)}
    times = {k: [] for k in forms}
    for r in range(args.reps + 2):
        for k, fn in forms.items():
            t = stamp(fn)
            if r >= 2:
                times[k].append(t)
    fused, eager = spread(times["fused"]), spread(times["eager"])
    nbytes = 2 * 12 * V
    print("%d iterations, tol = 0, %d alternating rounds after 2 warm-up rounds:" % (args.iters, args.reps))
    print("  fused launch (cvx_field_invert_f64)    median %8.3f ms  (min %.3f, max %.3f)   u read once + v written once = %.1f MB: %.2f TB/s = %.1f %% of the "
          "8.0 TB/s HBM peak" % (fused + (1e-6 * nbytes, 1e-12 * nbytes / (fused[0] * 1e-3), 100.0 * nbytes / (fused[0] * 1e-3) / HBM_PEAK)))
    print("  eager loop of F.grid_sample, float32   median %8.3f ms  (min %.3f, max %.3f)   ratio eager / fused %.2f" % (eager + (eager[0] / fused[0],)), flush=True)

    a, b = invert_field(u, max_iters=args.iters, tol=0.0), eager_invert(u, args.iters)
    print("largest difference between the two results: %.3g voxels (float64 taps rounded once against float32 taps in normalised coordinates)"
          % float((a - b).abs().max()))
    v, info = invert_field(u, return_info=True)
    it = info["iters"]
    print("at the defaults (50 iterations, tol 1e-4): not converged %d of %d voxels (%.4f %%), non-finite %d, largest residual %.4g voxels, iterations median %d, "
          "max %d" % (info["not_converged"], V, 100.0 * info["not_converged"] / V, info["non_finite"], info["max_residual"], int(it.flatten().float().median()),
                      int(it.max())))
    res = float(compose_fields(u, v).abs().max())
    print("max |compose_fields(u, v)| = %.4g voxels (float32 field in, float32 inverse out)" % res, flush=True)


if __name__ == "__main__":
    main()
