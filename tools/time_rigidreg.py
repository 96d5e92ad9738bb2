"""Times the rigid registration of the CuRIOUS script at its own size (256 x 256 x 288, two moving modalities = 24 channels, grid_sp 6,
search half-width 6, ellipsoid foreground, 5 inverse-consistency steps, 15 trimming iterations), alternating in ONE process:

  (a) the composition a user can write from the single operators: mind_pooled, correlate, ssd.mul_(mask), coupled_convex,
      inverse_consistency, resize_trilinear, rigid_from_field (eager torch for the masks, the scale and the flips);
  (b) convex_adam_rigid, with its rigid-fit rows taken from the coarse field (what ships) and, through the module switch
      rigid.SAMPLE_FROM_COARSE = False, from the up-sampled field (_field_samples): the same bits, timed side by side.

    python tools/time_rigidreg.py [--reps 5] [--rounds 3] [--once]

Prints per round the median over --reps of each, bracketed by device events after two warm-up calls, then the stages of (b) alone.
--once runs (b) a single time after one warm-up call, for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_rigidreg.py --once"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd.convex_adam_utils import (correlate, coupled_convex, disp_mesh_t, inverse_consistency, mind_pooled,  # noqa: E402
                                              resize_trilinear)
from convexadam_amd.phantom import ellipsoid_mask, phantom  # noqa: E402
from convexadam_amd import rigid  # noqa: E402
from convexadam_amd.rigid import (convex_adam_rigid, convex_stage, least_trimmed_rigid, rigid_from_field, rigid_samples,  # noqa: E402
                                  threshold_pool_mask)

SHAPE, G, HW, IC, LTS, THRESH = (256, 256, 288), 6, 6, 5, 15, 10.0


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


def composition(fixed, movs):
    dev = fixed.device
    ff = mind_pooled(fixed[None, None], 3, 3, G)
    ff = torch.cat([ff] * len(movs), 1)
    fm = torch.cat([mind_pooled(m[None, None], 3, 3, G) for m in movs], 1)
    mf = F.avg_pool3d((fixed > THRESH).float()[None, None], G, stride=G) > .5
    mm = F.avg_pool3d((movs[0] > THRESH).float()[None, None], G, stride=G) > .5
    mesh = disp_mesh_t(HW, dev)
    ssd, am = correlate(ff, fm, HW, G, SHAPE, ch=int(ff.shape[1]))
    ssd.mul_(mf[0])
    soft = coupled_convex(ssd, am, mesh, G, SHAPE)
    del ssd
    ssd, am = correlate(fm, ff, HW, G, SHAPE, ch=int(ff.shape[1]))
    ssd.mul_(mm[0])
    soft_ = coupled_convex(ssd, am, mesh, G, SHAPE)
    del ssd
    scale = torch.tensor([s // G - 1 for s in SHAPE], dtype=torch.float32, device=dev).view(1, 3, 1, 1, 1) / 2
    ice, _ = inverse_consistency((soft / scale).flip(1), (soft_ / scale).flip(1), iter=IC)
    hr = resize_trilinear(ice.flip(1) * scale * G, SHAPE)
    return rigid_from_field(hr, mf[0, 0], G, LTS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    inside = ellipsoid_mask(SHAPE, 0.40)
    fixed = ((40.0 * phantom(SHAPE, 3, 30) + 100.0) * inside).to(dev)
    moved = torch.roll((40.0 * phantom(SHAPE, 3, 31) + 100.0) * inside, (7, -5, 9), (0, 1, 2))
    movs = [moved.to(dev), (300.0 - 0.004 * (moved - 100.0) ** 2).clamp_min(0.0).mul(moved > 0).to(dev)]
    if args.once:
        convex_adam_rigid(fixed, movs, grid_sp=G, disp_hw=HW, mask_thresh=THRESH, ic_iters=IC, lts_iters=LTS)
        torch.cuda.synchronize()
        print(convex_adam_rigid(fixed, movs, grid_sp=G, disp_hw=HW, mask_thresh=THRESH, ic_iters=IC, lts_iters=LTS).T.cpu())
        return
    Ta = composition(fixed, movs)
    Tb = convex_adam_rigid(fixed, movs, grid_sp=G, disp_hw=HW, mask_thresh=THRESH, ic_iters=IC, lts_iters=LTS).T
    print("T of (a) and (b) bit-identical:", bool(torch.equal(Ta.view(torch.int32), Tb.view(torch.int32))))
    for r in range(args.rounds):
        a = timed(lambda: composition(fixed, movs), args.reps)
        b = timed(lambda: convex_adam_rigid(fixed, movs, grid_sp=G, disp_hw=HW, mask_thresh=THRESH, ic_iters=IC, lts_iters=LTS), args.reps)
        rigid.SAMPLE_FROM_COARSE = False
        try:
            bf = timed(lambda: convex_adam_rigid(fixed, movs, grid_sp=G, disp_hw=HW, mask_thresh=THRESH, ic_iters=IC, lts_iters=LTS), args.reps)
        finally:
            rigid.SAMPLE_FROM_COARSE = True
        print("round %d: (a) composition %.2f ms   (b) convex_adam_rigid %.2f ms   (b) with rows from the up-sampled field %.2f ms" % (r, a, b, bf))
    ff = torch.cat([mind_pooled(fixed[None, None], 3, 3, G)] * 2, 1)
    fm = torch.cat([mind_pooled(m[None, None], 3, 3, G) for m in movs], 1)
    mf, mm = threshold_pool_mask(fixed, THRESH, G), threshold_pool_mask(movs[0], THRESH, G)
    coarse, hr = convex_stage(ff, fm, G, HW, SHAPE, mf, mm, IC)
    T1, T2 = rigid_samples(coarse, mf, G, SHAPE)
    print("stages of (b): mind_pooled x 3 %.2f ms, masks x 2 %.3f ms, convex_stage %.2f ms (without disp_hr %.2f ms), rigid_samples %.3f ms, "
          "least_trimmed_rigid %.2f ms (rigid_from_field on disp_hr %.2f ms); masks keep %.0f %% / %.0f %%"
          % (timed(lambda: [mind_pooled(v[None, None], 3, 3, G) for v in [fixed] + movs], args.reps),
             timed(lambda: (threshold_pool_mask(fixed, THRESH, G), threshold_pool_mask(movs[0], THRESH, G)), args.reps),
             timed(lambda: convex_stage(ff, fm, G, HW, SHAPE, mf, mm, IC), args.reps),
             timed(lambda: convex_stage(ff, fm, G, HW, SHAPE, mf, mm, IC, full_res=False), args.reps),
             timed(lambda: rigid_samples(coarse, mf, G, SHAPE), args.reps), timed(lambda: least_trimmed_rigid(T1, T2, LTS), args.reps),
             timed(lambda: rigid_from_field(hr, mf, G, LTS), args.reps), 100 * float(mf.float().mean()), 100 * float(mm.float().mean())))


if __name__ == "__main__":
    main()
