"""Times the crop-field conversion of the abdomen MR-CT script (l2r_2021_convexAdam_task1_docker.py:38-105,390-400) as one fused launch
(csrc/cropfield.hip) against the same chain written in torch device operations, which materialise the full-resolution field the way the
reference does (a float32 coordinate list, its homogeneous copy, the matmul results, the sampled field, the flips, F.interpolate, .half()).

    python tools/time_cropfield.py [--reps 10] [--small]

The case: an original fixed CT of 512 x 512 x 150 voxels at (0.78, 0.78, 2.5) mm whose crop [10, 502] x [50, 460] x [-2, 152] resizes to the
registration grid 192 x 160 x 192 at 2 mm (--small: 64 x 64 x 30 and 24 x 20 x 24, for a quick check).  Prints, in ms, medians of --reps
after two warm-up calls, each call bracketed by device events on resident tensors: convert_crop_field (physical field, float16 and float32
out), submission_field (voxel field), the torch chain, half_resolution_field of a full-resolution field against F.interpolate on the device;
then the largest differences between the fused results and the torch chain's."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd.cropfield import (CropCase, convert_crop_field, half_resolution_field, physical_displacement,  # noqa: E402
                                      submission_field)


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


def torch_chain(case, disp_p, full_only=False):
    """convert_crop_field in torch device operations, float32, in the reference's order; the constants as CropCase computes them"""
    dev = disp_p.device
    k = {n: torch.from_numpy(v).to(dev) for n, v in case.constants().items()}
    S = case.fix_shape
    eye = torch.eye(4, device=dev)
    fix_affine, mov_affine = eye.clone(), eye.clone()
    for a in range(3):
        fix_affine[a, a], fix_affine[a, 3] = 1 / k["fix_scale"][a], k["fix_crop_lo"][a]
        mov_affine[a, a], mov_affine[a, 3] = 1 / k["mov_scale"][a], k["mov_crop_lo"][a]
    grid = torch.stack(torch.meshgrid(*[torch.arange(float(n), device=dev) for n in S], indexing="ij"), dim=3).view(1, -1, 3)
    ones = torch.ones(grid.shape[1], 1, device=dev)
    g = torch.matmul(fix_affine.inverse(), torch.cat([grid[0], ones], dim=1).t()).t()[:, :3].unsqueeze(0)
    n = k["new_shape"]
    pt = (g.flip(-1) / (n.flip(0) - 1)) * 2 - 1
    sampled = F.grid_sample(disp_p.permute(0, 4, 1, 2, 3), pt.view(1, 1, 1, -1, 3), mode="bilinear", padding_mode="border", align_corners=True)
    sampled = sampled.permute(0, 4, 2, 3, 1).view(1, -1, 3)
    est = (g * k["new_fix_spacing"] + sampled) / k["new_mov_spacing"]
    m = torch.matmul(mov_affine, torch.cat([est[0], ones], dim=1).t()).t()[:, :3].unsqueeze(0)
    disp = (m - grid).view(1, *S, 3)
    for a, ch in enumerate("xyz"):
        if ch in case.flip:
            disp = disp.flip(1 + a)
            disp[..., a] = -disp[..., a]
    disp = disp.permute(0, 4, 1, 2, 3)
    if full_only:
        return disp
    return F.interpolate(disp, scale_factor=0.5, mode="trilinear", align_corners=False)[0].half()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.small:
        case, grid = CropCase((64, 64, 30), (0.75, 0.75, 2.5), (0, 64, 5, 58, -1, 18), (40, 40, 40), (2.0, 2.0, 2.0), (0, 24, 0, 20, 0, 24)), (24, 20, 24)
    else:
        case, grid = CropCase((512, 512, 150), (0.78, 0.78, 2.5), (10, 502, 50, 460, -2, 152), (192, 160, 192), (2.0, 2.0, 2.0),
                              (0, 192, 0, 160, 0, 192)), (192, 160, 192)
    case.check_field_shape(grid)
    gen = torch.Generator().manual_seed(0)
    u = 6.0 * F.interpolate(torch.randn(1, 3, 6, 5, 6, generator=gen), size=grid, mode="trilinear", align_corners=True).to(dev).contiguous()
    pre = ((2.0, 2.0, 2.0), (2.0, 2.0, 2.0))
    disp_p = physical_displacement(u, *pre).contiguous()
    S = case.fix_shape
    out_bytes = 3 * (S[0] // 2) * (S[1] // 2) * (S[2] // 2)
    print("original fixed grid %s @ %s mm, registration grid %s @ %s mm; output 3 x %s: %.1f MB float16; a full-resolution float32 field: %.0f MB"
          % (S, case.fix_spacing, grid, case.ref_spacing, tuple(s // 2 for s in S), out_bytes * 2 / 1e6, 12 * S[0] * S[1] * S[2] / 1e6), flush=True)

    t16 = timed(lambda: convert_crop_field(case, disp_p), args.reps)
    t32 = timed(lambda: convert_crop_field(case, disp_p, out_dtype=torch.float32), args.reps)
    tvox = timed(lambda: submission_field(u, pre[0], pre[1], case), args.reps)
    print("fused launch (device events, resident tensors): convert_crop_field float16 %.3f ms, float32 %.3f ms; submission_field (voxel field) %.3f ms"
          % (t16, t32, tvox), flush=True)
    tchain = timed(lambda: torch_chain(case, disp_p), max(2, args.reps // 2))
    torch.cuda.synchronize()
    print("torch device operations, the reference's chain (full-resolution field materialised): %.2f ms; peak memory %.2f GB"
          % (tchain, torch.cuda.max_memory_allocated() / 1e9), flush=True)

    full = torch_chain(case, disp_p, full_only=True).contiguous()
    thalf = timed(lambda: half_resolution_field(full), args.reps)
    taten = timed(lambda: F.interpolate(full, scale_factor=0.5, mode="trilinear", align_corners=False), args.reps)
    print("halving alone of a resident full-resolution field: half_resolution_field %.3f ms, F.interpolate on the device %.3f ms" % (thalf, taten), flush=True)

    a, b = convert_crop_field(case, disp_p, out_dtype=torch.float32), torch_chain(case, disp_p)
    h = convert_crop_field(case, disp_p)
    print("largest differences: fused float32 - torch chain float16 %.3g (largest value %.3g: half a float16 step there is %.3g); float16 outputs that differ: %d of %d; "
          "submission_field - convert_crop_field(physical_displacement) %.3g"
          % (float((a - b.float()).abs().max()), float(a.abs().max()), 0.5 * 2.0 ** (torch.floor(torch.log2(a.abs().max())).item() - 10),
             int((h != b).sum()), h.numel(), float((submission_field(u, pre[0], pre[1], case).float() - h.float()).abs().max())), flush=True)


if __name__ == "__main__":
    main()
