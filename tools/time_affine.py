"""Times the least-trimmed affine fit (n = 2 000 and 30 000 points, 15 fits, both equations) and the affine displacement field
(160 x 192 x 224), each beside the torch expression it replaces on the same GPU: torch.linalg.solve + torch.topk per iteration; the
float64 coordinates of F.affine_grid un-normalised minus the voxel index (with a field: the same map applied to x + u(x)).

    python tools/time_affine.py [--reps 20]

Prints the median over --reps (after two warm-up calls) of each call, bracketed by device events."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd.affine import affine_to_field, least_trimmed_affine, least_trimmed_squares  # noqa: E402


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


def torch_lts(f, m, iters, normal):
    idx = torch.arange(f.shape[0], device=f.device)
    for _ in range(iters):
        F_, M_ = f[idx], m[idx]
        x = torch.linalg.solve(M_.t() @ F_, M_.t() @ M_) if normal else torch.linalg.solve(F_.t() @ F_, F_.t() @ M_)
        r = ((m - f @ x) ** 2).sum(1).sqrt()
        idx = torch.topk(r, f.shape[0] // 2, largest=False).indices
    return x


def torch_field(T, shape, u=None):
    """float64 on the device: theta applied to the normalised coordinates of x (+ u), un-normalised, minus x; (H, W, D, 3)"""
    dev = T.device
    S = torch.tensor(shape, dtype=torch.float64, device=dev)
    x = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64, device=dev) for n in shape], indexing="ij"), -1)
    p = x if u is None else x + u.double()
    n = ((2 * p + 1) / S - 1).flip(-1)                                      # (x, y, z) order
    g = n @ T[:3, :3].double().t() + T[:3, 3].double()
    return ((g.flip(-1) + 1) * S - 1) / 2 - x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {}
    A = torch.tensor([[1.06, 0.03, -0.02], [-0.04, 0.95, 0.05], [0.02, -0.03, 1.0]])
    for n in (2000, 30000):
        x = torch.rand(n, 3, generator=g) * 2 - 1
        y = x @ A + torch.tensor([0.05, -0.08, 0.03]) + 0.01 * torch.randn(n, 3, generator=g)
        y[:n // 4] += torch.randn(n // 4, 3, generator=g)
        f = torch.cat([x, torch.ones(n, 1)], 1).to(dev)
        m = torch.cat([y, torch.ones(n, 1)], 1).to(dev)
        tag = "lts_%dk" % (n // 1000)
        res[tag + "_hip_ms"] = timed(lambda: least_trimmed_affine(f, m, 15), args.reps)
        res[tag + "_torch_ms"] = timed(lambda: torch_lts(f, m, 15, 0), args.reps)
        res[tag + "_ref_eq_hip_ms"] = timed(lambda: least_trimmed_squares(f, m, 15), args.reps)
        res[tag + "_ref_eq_torch_ms"] = timed(lambda: torch_lts(f, m, 15, 1), args.reps)
    shape = (160, 192, 224)
    T = least_trimmed_affine(f, m, 15)
    u = (3 * torch.randn(shape + (3,), generator=g)).to(dev)
    res["field_hip_ms"] = timed(lambda: affine_to_field(T, shape), args.reps)
    res["field_torch_ms"] = timed(lambda: torch_field(T, shape), args.reps)
    res["field_u_hip_ms"] = timed(lambda: affine_to_field(T, shape, field=u), args.reps)
    res["field_u_torch_ms"] = timed(lambda: torch_field(T, shape, u), args.reps)
    err = float((affine_to_field(T, shape, field=u) - torch_field(T, shape, u)).abs().max())
    print("15 fits; field %d x %d x %d float64:" % shape, " ".join("%s %.3f" % kv for kv in res.items()), "max|hip - torch| field %.3g voxel" % err)


if __name__ == "__main__":
    main()
