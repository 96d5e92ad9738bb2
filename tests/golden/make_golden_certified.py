"""Goldens for tests/test_certified_cases_reference.py: the reference's correlate / coupled_convex on the inputs of tests/certified_cases.py,
captured from the reference itself (run ONLY in the build container, the reference tree is not on the other hosts):

    python tests/golden/make_golden_certified.py        # -> tests/golden/certified.npz

The inputs are rebuilt from seeds by tests/certified_cases.py; only the reference's outputs are stored.  Per plain case: the argmin (int16)
and the digest of the cost volume (make_golden_live.digest: equal digests <=> np.array_equal(..., equal_nan=True)).  Per pair case, on the
features pooled by grid_sp as the pipeline pools them: argmin and volume digest as above and the coupled_convex field (float32) of the
forward direction, the field's digest for the backward one.  torch runs with 8 threads, as for every other golden."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import certified_cases as CC  # noqa: E402
from make_golden_live import digest  # noqa: E402


def mesh_of(hw):
    n = 2 * hw + 1
    return torch.nn.functional.affine_grid(hw * torch.eye(3, 4).unsqueeze(0), (1, 1, n, n, n), align_corners=True).permute(0, 4, 1, 2, 3).reshape(3, -1, 1)


def main():
    from _ref_import import import_reference
    utils, _ = import_reference()
    torch.set_num_threads(8)
    out = {}
    for name, C, shape, hw, f, m in CC.CASES:
        ssd, am = utils.correlate(torch.from_numpy(f)[None], torch.from_numpy(m)[None], hw, 1, shape, C)
        out[name + ":ssd_digest"], out[name + ":argmin"] = np.array(digest(ssd.numpy())), am.numpy().astype(np.int16)
    C, full = CC.PAIR_SHAPE
    g, hw = CC.PAIR_KW["grid_sp"], CC.PAIR_KW["disp_hw"]
    shape = tuple(s // g for s in full)
    for name, f, m in CC.PAIRS:
        fs = torch.nn.functional.avg_pool3d(torch.from_numpy(f)[None], g, stride=g)
        ms = torch.nn.functional.avg_pool3d(torch.from_numpy(m)[None], g, stride=g)
        for tag, a, b in (("fwd", fs, ms), ("bwd", ms, fs)):
            ssd, am = utils.correlate(a, b, hw, g, full, C)
            soft = utils.coupled_convex(ssd, am, mesh_of(hw), g, full)[0].numpy()
            out["%s:%s_ssd_digest" % (name, tag)], out["%s:%s_argmin" % (name, tag)] = np.array(digest(ssd.numpy())), am.numpy().astype(np.int16)
            if tag == "fwd":
                out["%s:fwd_soft" % name] = soft
            else:
                out["%s:bwd_soft_digest" % name] = np.array(digest(soft))
        assert soft.shape == (3,) + shape
    path = os.path.join(HERE, "certified.npz")
    np.savez_compressed(path, **out)
    print(len(out), "entries,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
