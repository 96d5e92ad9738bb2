"""Times the 3-D SSIM kernel against the torch-on-device composition of the reference's expression (five dense conv3d calls with the
11^3 window: what a user of the parent commit would write) at 160 x 192 x 224 and at 64 volumes of 40^3 in one call.

    python tools/time_ssim.py [--reps 10] [--window 11]

Prints the median over --reps (after two warm-up calls) of: the mean alone, the map alone, the map and the mean in two calls, and the
composition, each bracketed by device events; then the largest difference between the two maps and between the two means."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd.ssim import create_window_3D, ssim3D, ssim3D_map  # noqa: E402


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


def torch_composition(x, y, win, ws):
    """tests/helper_functions.py:114-135 of the reference on device tensors -> (map, mean)"""
    c, pad = x.shape[1], ws // 2
    mu1, mu2 = F.conv3d(x, win, padding=pad, groups=c), F.conv3d(y, win, padding=pad, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv3d(x * x, win, padding=pad, groups=c) - mu1_sq
    s2 = F.conv3d(y * y, win, padding=pad, groups=c) - mu2_sq
    s12 = F.conv3d(x * y, win, padding=pad, groups=c) - mu1_mu2
    m = ((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return m, m.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=11)
    ap.add_argument("--no-torch", action="store_true", help="skip the dense composition")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ws = args.window
    g = torch.Generator().manual_seed(0)
    for shape in ((1, 1, 160, 192, 224), (64, 1, 40, 40, 40)):
        x = torch.rand(*shape, generator=g).to(dev)
        y = (x + 0.1 * torch.randn(*shape, generator=g).to(dev)).clamp_(0, 1)
        res = {
            "mean_ms": timed(lambda: ssim3D(x, y, ws), args.reps),
            "map_ms": timed(lambda: ssim3D_map(x, y, ws), args.reps),
            "map_and_mean_ms": timed(lambda: (ssim3D_map(x, y, ws), ssim3D(x, y, ws)), args.reps),
        }
        line = "%s ws %d: " % ("x".join(str(v) for v in shape), ws) + " ".join("%s %.4f" % kv for kv in res.items())
        if not args.no_torch:
            win = create_window_3D(ws, shape[1]).to(dev)
            line += " torch_conv3d_ms %.4f" % timed(lambda: torch_composition(x, y, win, ws), args.reps)
            m, r = torch_composition(x, y, win, ws)
            line += " | max map diff %.3g mean diff %.3g" % (float((m - ssim3D_map(x, y, ws)).abs().max()), abs(float(r) - float(ssim3D(x, y, ws))))
        print(line, flush=True)


if __name__ == "__main__":
    main()
