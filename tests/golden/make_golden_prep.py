"""Writes tests/golden/prep.npz: inputs, outputs and the reference's own mean / std / lo / hi for the preprocessing helpers
(convex_adam_utils.py:15-21, 142-170, 196-265), captured from the upstream reference on the CPU.

    python tests/golden/make_golden_prep.py

Needs the reference tree (tests/golden/_ref_import.py) and scipy.  Prints, per case, the distance in float32 ulps between the
reference's mean / std (torch's float32 sums) and the restatement's (float64 in a fixed order, rounded once): the figures DESIGN.md 31
quotes and tests/test_prep_reference.py bounds."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from _ref_import import import_reference  # noqa: E402
import prep_restatement as R  # noqa: E402

CT_SHAPES = [(33, 31, 37), (24, 20, 28), (5, 4, 131)]
PROPS = {'mean': 93.25, 'sd': 217.625, 'percentile_00_5': -958.0, 'percentile_99_5': 1203.5}


def ct_like(shape, seed, integer):
    """air around a body: about 40 % of the voxels below the -1000 clamp, soft tissue around 40, a little bone above 1500"""
    g = np.random.default_rng(seed)
    x = g.normal(40.0, 180.0, shape)
    x[g.random(shape) < 0.4] = -1024.0 - 50.0 * g.random()
    x[g.random(shape) < 0.01] = 1700.0 + 800.0 * g.random()
    return (np.round(x) if integer else x).astype(np.float32)


def main():
    utils, _ = import_reference()
    torch.set_num_threads(1)
    out = {}
    for i, shape in enumerate(CT_SHAPES):
        x = ct_like(shape, 100 + i, integer=(i != 1))
        t = torch.from_numpy(x)
        c = t.clamp(min=-1000, max=1500)                                    # torch's own float32 statistics of the clamped volume
        ref = [c.mean(), c.std(), c.quantile(0.005), c.quantile(0.995)]
        out["ct%d_in" % i] = x
        out["ct%d_out" % i] = utils.nnUNetCTnorm(t.clone()).numpy()
        out["ct%d_params" % i] = np.array([float(v) for v in ref], np.float32)
        mine = R.stats(x, clamp_to=(-1000.0, 1500.0), qs=(0.005, 0.995))[0]
        print("ct %-12s mean %d ulp, std %d ulp, lo %s, hi %s" % ("x".join(map(str, shape)), R.ulps(mine[0], ref[0]), R.ulps(mine[1], ref[1]),
                                                                  mine[2] == np.float32(ref[2]), mine[3] == np.float32(ref[3])))
        if i == 0:
            continue
        positive = t[t > 0]
        refn = [positive.mean(), positive.std()]
        out["norm%d_out" % i] = utils.nnUNetNorm(t.clone()).numpy()
        out["norm%d_params" % i] = np.array([float(v) for v in refn], np.float32)
        minen = R.stats(x, positive=True)[0]
        print("norm %-10s mean %d ulp, std %d ulp" % ("x".join(map(str, shape)), R.ulps(minen[0], refn[0]), R.ulps(minen[1], refn[1])))
        out["props%d_out" % i] = utils.nnUNetNormProps(t.clone(), PROPS).numpy()
    out["props"] = np.array(json.dumps(PROPS))

    g = np.random.default_rng(7)
    data = np.zeros((2, 9, 10, 11), np.float32)
    data[0, 2:7, 2:8, 3:9] = g.random((5, 6, 6)) + 0.5
    data[0, 3:6, 3:7, 4:8] = 0                                               # a cavity ...
    data[1, 4, 4, 5] = 3.0                                                   # ... with an island of the other channel inside
    data[1, 7, 8, 9] = -1.0
    mask = utils.create_nonzero_mask(data)
    box = utils.get_bbox_from_mask(mask)
    out.update(mask3_in=data, mask3_out=mask, bbox3=np.array(box), crop3=utils.crop_to_bbox(data[0], box))
    data2 = np.zeros((1, 12, 13), np.float32)
    data2[0, 2:9, 3:11] = 1
    data2[0, 4:7, 5:9] = 0
    data2[0, 5, 6] = 2
    out.update(mask2_in=data2, mask2_out=utils.create_nonzero_mask(data2))

    for name, patch in (("a", (8, 8, 8)), ("b", (5, 6, 7))):
        out["gauss_%s_patch" % name] = np.array(patch)
        out["gauss_%s" % name] = utils.get_gaussian(patch, device='cpu').numpy()
    sw = [((64, 64, 64), (110, 128, 64), 0.5), ((8, 12, 16), (33, 31, 37), 0.5), ((32, 32, 32), (160, 192, 224), 0.25), ((5, 6, 7), (5, 7, 29), 1.0)]
    out["steps"] = np.array(json.dumps([[list(p), list(s), st, utils.compute_steps_for_sliding_window(p, s, st)] for p, s, st in sw]))
    pts = torch.from_numpy(g.random((1, 3, 6)).astype(np.float32))
    out.update(pdist_in=pts.numpy(), pdist_out=utils.pdist_squared(pts).numpy())
    path = os.path.join(HERE, "prep.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
