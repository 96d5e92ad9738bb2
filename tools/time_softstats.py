"""Times the fused soft statistics of a cost volume (csrc/softstats.hip, cvx_soft_stats_f32) against what a user can write without it: the
eager PyTorch formula -- the minimum, exp(-beta (e - min)), its sum, and the weighted sums of displacement, displacement products and
excess energy (the nine moment sums as ONE matrix product, the kindest eager form) -- in float32.

    python tools/time_softstats.py [--reps 9] [--small]

The input is the cost volume of the benchmark pair: deformed_pair at 160 x 192 x 224 (convexadam_amd/phantom.py), MIND-SSC features pooled
by 6, correlate with disp_hw 6 -> (2197, 26, 32, 37), once as float32 and once with float16 storage, and coupled_convex's field on it
(--small: 48^3, grid 4, hw 2, for a quick check).  beta is 4 / (the median over cells of the cost's spread between its minimum and its
median entry).  Four cases: {float32, float16} x {data term, coupled energy around the field}.  The two forms alternate in ONE process on
resident tensors, each call bracketed by device events behind a device synchronisation, --reps rounds after two warm-up rounds; medians
and the spread (min .. max) are printed, their ratio, and the bytes the fused form needs -- the volume read once, the field, the twelve
output channels -- over its time against the 8 TB/s HBM peak (the kernels read the volume twice, the second time from the caches where
they hold it: the figure says how far the call is from the single-read bound).  A run without a HIP device fails."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd.confidence import soft_stats  # noqa: E402
from convexadam_amd.convex_adam_MIND import extract_features  # noqa: E402
from convexadam_amd.convex_adam_utils import avg_pool, correlate, coupled_convex, disp_mesh_t  # noqa: E402
from convexadam_amd.phantom import deformed_pair  # noqa: E402

HBM_PEAK = 8.0e12


def eager_stats(ssd, mesh, beta, field=None, coupling=0.0):
    """(12, h, w, d) float32 by the plain formula.  mesh: (K, 3) displacements in k order."""
    K = ssd.shape[0]
    grid = tuple(ssd.shape[1:])
    e = ssd.reshape(K, -1).float()
    if field is not None:
        u = field.reshape(3, -1)
        e = e + coupling * ((mesh[:, :, None] - u[None]) ** 2).sum(1)
    m = e.amin(0)
    r = e - m
    p = torch.exp(-beta * r)
    Z = p.sum(0)
    w = p / Z
    r = torch.where(torch.isfinite(r), r, torch.zeros_like(r))
    feats = torch.cat([mesh, mesh[:, [0, 0, 0, 1, 1, 2]] * mesh[:, [0, 1, 2, 1, 2, 2]]], 1)          # (K, 9)
    mom = feats.t() @ w                                                                             # (9, V)
    mean = mom[0:3]
    cov = mom[3:9] - mean[[0, 0, 0, 1, 1, 2]] * mean[[0, 1, 2, 1, 2, 2]]
    return torch.cat([mean, cov, Z[None], (w * r).sum(0)[None], m[None]], 0).reshape((12,) + grid)


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
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_softstats.py measures on a HIP device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    shape, grid_sp, hw = ((48, 48, 48), 4, 2) if args.small else ((160, 192, 224), 6, 6)
    fix, mov = deformed_pair(shape, 0, 4.0)
    ff, fm = extract_features(fix.to(dev).contiguous(), mov.to(dev).contiguous(), 1, 2, False, None, None, device=dev, dtype=torch.float32)
    ff, fm = avg_pool(ff, grid_sp), avg_pool(fm, grid_sp)
    mesh_t = disp_mesh_t(hw, dev)
    mesh = mesh_t[:, :, 0].t().contiguous()
    volumes = {}
    for storage in ("fp32", "fp16"):
        ssd, am = correlate(ff, fm, hw, grid_sp, shape, 12, storage=storage)
        volumes[storage] = (ssd, coupled_convex(ssd, am, mesh_t, grid_sp, shape)[0].contiguous())
    del ff, fm
    ssd32 = volumes["fp32"][0]
    K, V = int(ssd32.shape[0]), int(ssd32[0].numel())
    flat = ssd32.reshape(K, -1)
    beta = 4.0 / float((flat.median(0).values - flat.amin(0)).median())
    print("cost volume %s of the benchmark pair at %s: %.1f MB as float32; beta = %.4g" % (tuple(ssd32.shape), shape, 4e-6 * K * V, beta), flush=True)

    for storage in ("fp32", "fp16"):
        ssd, field = volumes[storage]
        for with_field in (False, True):
            u, c = (field, 1.0) if with_field else (None, 0.0)
            forms = {"fused": lambda: soft_stats(ssd, hw, beta, u, c), "eager": lambda: eager_stats(ssd, mesh, beta, u, c)}
            times = {k: [] for k in forms}
            for r in range(args.reps + 2):
                for k, fn in forms.items():
                    t = stamp(fn)
                    if r >= 2:
                        times[k].append(t)
            fused, eager = spread(times["fused"]), spread(times["eager"])
            nbytes = K * V * ssd.element_size() + (12 * V if with_field else 0) + 48 * V
            a, info = soft_stats(ssd, hw, beta, u, c, return_info=True)
            b = eager_stats(ssd, mesh, beta, u, c)
            print("%s volume, %s, %d alternating rounds after 2 warm-up rounds (non-finite cells: %d, median Z %.1f):"
                  % (storage, "coupled energy around the field" if with_field else "data term", args.reps, info["non_finite"], float(a[9].median())))
            print("  fused call (cvx_soft_stats_f32)   median %8.3f ms  (min %.3f, max %.3f)   volume once + outputs = %.1f MB: %.2f TB/s = %.1f %% of the "
                  "8.0 TB/s HBM peak" % (fused + (1e-6 * nbytes, 1e-12 * nbytes / (fused[0] * 1e-3), 100.0 * nbytes / (fused[0] * 1e-3) / HBM_PEAK)))
            print("  eager formula, float32            median %8.3f ms  (min %.3f, max %.3f)   ratio eager / fused %.2f;  largest difference: mean %.3g, cov %.3g, "
                  "Z %.3g relative" % (eager + (eager[0] / fused[0], float((a[0:3] - b[0:3]).abs().max()), float((a[3:9] - b[3:9]).abs().max()),
                                               float((a[9] / b[9] - 1).abs().max()))), flush=True)


if __name__ == "__main__":
    main()
