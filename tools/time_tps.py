"""Times the thin-plate-spline densification at the task1 setting: n centres (default 4096) on 160 x 192 x 224, step 4.

    python tools/time_tps.py [--n 4096] [--reps 10]

Prints the median over --reps (after two warm-up calls) of: TPS.fit, the dense lattice evaluation (40 x 48 x 56), the align_corners=True
up-sampling, thin_plate_dense, and tps_densify (sampling + thin_plate_dense + three 3^3 boxes), each bracketed by device events."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd.tps import TPS, resize_trilinear_ac, thin_plate_dense, tps_dense, tps_densify  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, D = 160, 192, 224
    g = torch.Generator().manual_seed(0)
    ident = torch.nn.functional.affine_grid(torch.eye(3, 4).unsqueeze(0), (1, 1, H // 3, W // 3, D // 3), align_corners=True).view(-1, 3)
    c = ident[torch.randperm(ident.shape[0], generator=g)[:args.n]].to(dev)
    f = (0.02 * torch.sin(3 * c) + 0.002 * torch.randn(args.n, 3, generator=g).to(dev)).contiguous()
    theta = TPS.fit(c, f)
    coarse = tps_dense(c, theta, (H // 4, W // 4, D // 4)).unsqueeze(0)
    disp = (torch.randn(1, 3, H // 8, W // 8, D // 8, generator=g) * 3).to(dev)
    disp_hr = torch.nn.functional.interpolate(disp, (H, W, D), mode="trilinear", align_corners=False).contiguous()
    mask = torch.ones(H, W, D)
    res = {
        "fit_ms": timed(lambda: TPS.fit(c, f), args.reps),
        "dense_eval_ms": timed(lambda: tps_dense(c, theta, (H // 4, W // 4, D // 4)), args.reps),
        "resize_ac_ms": timed(lambda: resize_trilinear_ac(coarse, (H, W, D)), args.reps),
        "thin_plate_dense_ms": timed(lambda: thin_plate_dense(c.unsqueeze(0), f.unsqueeze(0), (H, W, D), 4), args.reps),
        "tps_densify_ms": timed(lambda: tps_densify(disp_hr, mask, n_points=args.n, generator=torch.Generator().manual_seed(1)), args.reps),
    }
    print("n = %d, %d x %d x %d, step 4:" % (args.n, H, W, D), " ".join("%s %.3f" % kv for kv in res.items()))


if __name__ == "__main__":
    main()
