"""Times the least-trimmed rigid fit and the fused affine warp at the CuRIOUS setting (256 x 256 x 288, grid_sp 4), each beside the
same computation in eager torch on the GPU (torch.linalg.svd + torch.topk per iteration; F.affine_grid + F.grid_sample).

    python tools/time_rigid.py [--reps 20]

Prints the median over --reps (after two warm-up calls) of each call, bracketed by device events."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd.rigid import _field_samples, affine_warp, least_trimmed_rigid, rigid_from_field  # noqa: E402


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


def torch_kabsch(x, y):
    xm, ym = x[:, :3].mean(0), y[:, :3].mean(0)
    U, _, Vh = torch.linalg.svd((x[:, :3] - xm).t() @ (y[:, :3] - ym))
    V = Vh.t()
    m = torch.eye(3, device=x.device)
    m[2, 2] = torch.det(V @ U.t())
    R = V @ m @ U.t()
    T = torch.eye(4, device=x.device)
    T[:3, :3], T[:3, 3] = R, ym - R @ xm
    return T


def torch_lts(f, m, iters):
    idx = torch.arange(f.shape[0], device=f.device)
    for _ in range(iters):
        T = torch_kabsch(f[idx], m[idx])
        r = ((m - f @ T.t()) ** 2).sum(1).sqrt()
        idx = torch.topk(r, f.shape[0] // 2, largest=False).indices
    return T


def torch_warp(vol, R, mode):
    grid = F.affine_grid(R[:3].unsqueeze(0), (1,) + tuple(vol.shape), align_corners=False)
    return F.grid_sample(vol.unsqueeze(0), grid, mode=mode, align_corners=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {}
    for n in (40000, 85000):
        x = torch.randn(n, 3, generator=g) * torch.tensor([0.6, 0.4, 0.3])
        c, s = torch.cos(torch.tensor(0.1)), torch.sin(torch.tensor(0.1))
        R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        y = x @ R.t() + 0.01 * torch.randn(n, 3, generator=g)
        y[:n // 4] += torch.randn(n // 4, 3, generator=g)
        f = torch.cat([x, torch.ones(n, 1)], 1).to(dev)
        m = torch.cat([y, torch.ones(n, 1)], 1).to(dev)
        res["lts_%dk_hip_ms" % (n // 1000)] = timed(lambda: least_trimmed_rigid(f, m, 15), args.reps)
        res["lts_%dk_torch_ms" % (n // 1000)] = timed(lambda: torch_lts(f, m, 15), args.reps)
    H, W, D, sp = 256, 256, 288, 4
    vol = torch.randint(0, 10, (1, H, W, D), generator=g).float().to(dev)
    T = least_trimmed_rigid(f, m, 15)
    for mode in ("nearest", "bilinear"):
        res["warp_%s_hip_ms" % mode] = timed(lambda: affine_warp(vol, T, mode=mode), args.reps)
        res["warp_%s_torch_ms" % mode] = timed(lambda: torch_warp(vol, T, mode), args.reps)
    disp_hr = F.interpolate(torch.randn(1, 3, H // 16, W // 16, D // 16, generator=g) * 4, (H, W, D), mode="trilinear",
                            align_corners=False).to(dev)
    mask = (F.avg_pool3d(torch.rand(1, 1, H, W, D, generator=g), sp, stride=sp) > 0.5).to(dev)[0, 0]
    mask[: H // sp // 4] = False
    res["cells"] = int(mask.sum())

    def torch_from_field():
        affine = F.affine_grid(torch.eye(3, 4, device=dev).unsqueeze(0), (1, 1, H, W, D), align_corners=False)
        disp0 = (disp_hr.permute(0, 2, 3, 4, 1) / torch.tensor([H - 1, W - 1, D - 1], device=dev).view(1, 1, 1, 1, 3) * 2).flip(4)
        pts = F.affine_grid(torch.eye(3, 4, device=dev).unsqueeze(0), (1, 1, H // sp, W // sp, D // sp), align_corners=False)
        pts = pts.reshape(-1, 3)[torch.nonzero(mask.reshape(-1)).squeeze(1)]
        T1 = F.grid_sample(affine.permute(0, 4, 1, 2, 3), pts.view(1, -1, 1, 1, 3), align_corners=False)[0, :, :, 0, 0].t()
        T2 = F.grid_sample((affine + disp0).permute(0, 4, 1, 2, 3), pts.view(1, -1, 1, 1, 3), align_corners=False)[0, :, :, 0, 0].t()
        ones = torch.ones(pts.shape[0], 1, device=dev)
        return torch_lts(torch.cat([T1, ones], 1), torch.cat([T2, ones], 1), 15)

    res["field_samples_hip_ms"] = timed(lambda: _field_samples(disp_hr, mask, sp), args.reps)
    res["rigid_from_field_hip_ms"] = timed(lambda: rigid_from_field(disp_hr, mask, sp, 15), args.reps)
    res["rigid_from_field_torch_ms"] = timed(torch_from_field, args.reps)
    print("%d x %d x %d, grid_sp %d, iter 15:" % (H, W, D, sp), " ".join("%s %s" % (k, ("%.3f" % v) if isinstance(v, float) else v)
                                                                          for k, v in res.items()))


if __name__ == "__main__":
    main()
