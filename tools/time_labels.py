"""Times the label (nnUNet) path at BASELINE configs[3] -- 160 x 192 x 160, 32 labels (phantom.label_phantom), grid_sp 4, disp_hw 4,
grid_sp_adam 2, 10 Adam iterations -- both ways in ONE process, from device-resident label maps:

  old  extract_features (two weighted one-hot volumes [32][160][192][160]) + register_pair_device(feat_fixed=, feat_moving=)
  new  register_labels_device (cvx_register_label_pair_f32: the pooled features straight from the maps)

and the feature stage alone: extract_features + avg_pool(., 4) + avg_pool(., 2) per image against label_features_pooled(., 4, 2), once
through the public functions (both include the label histograms and the host-side weights) and once as the C entries alone with the
channel list given (cvx_label_features_f32 + 2 x cvx_avgpool_f32 per image against cvx_label_features_pooled_f32 per image).

    timeout -k 10 600 python tools/time_labels.py [--reps 20] [--warmup 3] [--niter 10]

The two ways alternate call by call; each figure is the median over --reps of device events on the stream after --warmup calls.  Prints
ONE JSON line.  --once runs the new feature kernels a single time after one warm-up call, for a kernel trace in a run of its own:
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_labels.py --once"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd import convex_adam_nnUNet as N  # noqa: E402
from convexadam_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from convexadam_amd.convex_adam_MIND import register_pair_device  # noqa: E402
from convexadam_amd.convex_adam_utils import avg_pool  # noqa: E402
from convexadam_amd.phantom import label_phantom  # noqa: E402

SHAPE, LABELS, GS, HW, GSA, MULT = (160, 192, 160), 32, 4, 4, 2, 10.0


def timed_alternating(fns, reps, warmup):
    """Median milliseconds of each function of `fns`, called in turn: warm-up rounds first, then `reps` rounds bracketed by events."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
    return [sorted(t)[len(t) // 2] for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lab = label_phantom(SHAPE, LABELS, 3)
    lf, lm = lab.to(dev), torch.roll(lab, (4, -2, 6), (0, 1, 2)).to(dev)
    H, W, D = SHAPE
    V = H * W * D
    L = lib()
    _, _, present_d, weights_d, Cn = N._label_channels(lf, lm, dev)
    pooled = [torch.empty((Cn, H // g, W // g, D // g), dtype=torch.float32, device=dev) for g in (GS, GSA)]

    def new_kernels():
        for x in (lf, lm):
            check(L.cvx_label_features_pooled_f32(ptr(x), H, W, D, Cn, ptr(present_d), ptr(weights_d), MULT, GS, ptr(pooled[0]), GSA, ptr(pooled[1]),
                                                  stream_ptr(dev)))

    if args.once:
        new_kernels()
        torch.cuda.synchronize()
        new_kernels()
        torch.cuda.synchronize()
        print("label_features_pooled kernels ran once after one warm-up call; C = %d" % Cn)
        return

    kw = dict(lambda_weight=1.25, grid_sp=GS, disp_hw=HW, selected_niter=args.niter, grid_sp_adam=GSA, ic=True)

    def old_pair():
        ff, fm = N.extract_features(lf, lm, mult=MULT, device=dev)
        return register_pair_device(feat_fixed=ff[0], feat_moving=fm[0], **kw)

    def new_pair():
        return N.register_labels_device(lf, lm, mult=MULT, **kw)

    def old_stage():
        ff, fm = N.extract_features(lf, lm, mult=MULT, device=dev)
        return [avg_pool(f, g) for f in (ff, fm) for g in (GS, GSA)]

    def new_stage():
        return N.label_features_pooled(lf, lm, GS, GSA, mult=MULT, device=dev)

    same = bool(torch.equal(old_pair().view(torch.int32), new_pair().view(torch.int32)))
    old_s, new_s = old_stage(), new_stage()
    same = same and all(torch.equal(a[0], b) for a, b in zip(old_s, (new_s[0][0], new_s[1][0], new_s[0][1], new_s[1][1])))
    del old_s, new_s
    onehot = torch.empty((Cn, H, W, D), dtype=torch.float32, device=dev)

    def old_kernels():
        for x in (lf, lm):
            check(L.cvx_label_features_f32(ptr(x), V, Cn, ptr(present_d), ptr(weights_d), MULT, ptr(onehot), stream_ptr(dev)))
            for g, out in zip((GS, GSA), pooled):
                check(L.cvx_avgpool_f32(ptr(onehot), Cn, H, W, D, g, ptr(out), stream_ptr(dev)))

    pair_old, pair_new = timed_alternating([old_pair, new_pair], args.reps, args.warmup)
    stage_old, stage_new = timed_alternating([old_stage, new_stage], args.reps, args.warmup)
    kern_old, kern_new = timed_alternating([old_kernels, new_kernels], args.reps, args.warmup)
    out_bytes = sum(2 * t.numel() * 4 for t in pooled)
    print(json.dumps({
        "tool": "time_labels", "shape": list(SHAPE), "channels": Cn, "grid_sp": GS, "disp_hw": HW, "grid_sp_adam": GSA, "adam_iters": args.niter,
        "reps": args.reps, "warmup": args.warmup, "bit_identical": same,
        "labels_to_field_ms": {"onehot": round(pair_old, 4), "pooled": round(pair_new, 4)},
        "feature_stage_ms": {"onehot": round(stage_old, 4), "pooled": round(stage_new, 4)},
        "feature_kernels_ms": {"onehot": round(kern_old, 4), "pooled": round(kern_new, 4)},
        "pooled_algorithmic_bytes": 2 * V * 4 + out_bytes, "onehot_volume_bytes_each": Cn * V * 4}))


if __name__ == "__main__":
    main()
