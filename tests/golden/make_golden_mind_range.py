"""Goldens for tests/test_mind_range_reference.py: the reference's MINDSSC on the inputs of tests/mind_range_cases.py, captured from the
reference itself (run ONLY in the build container, the reference tree is not on the other hosts):

    python tests/golden/make_golden_mind_range.py        # -> tests/golden/mind_range.npz

The inputs are rebuilt from seeds by tests/mind_range_cases.py; only the reference's outputs are stored.  Per case: the number of NaNs, the
number of exact ones, the digest of the descriptor (make_golden_live.digest: equal digests <=> np.array_equal(..., equal_nan=True)) and, for
the volumes of at most ARRAY_VOXELS voxels whose descriptor is not all NaN, the descriptor itself.  A case on which the reference raises
(`mind_var.mean().item() * 1000` beyond float32's range is refused by torch.clamp) stores the flag `raises` instead.  torch runs with 8
threads, as for every other golden, and once more with 1: the captures must not depend on it (asserted)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import mind_range_cases as MC  # noqa: E402
from make_golden_live import digest  # noqa: E402

ARRAY_VOXELS = 1000


def reference_descriptor(mindssc, c):
    """(12, H, W, D) float32, or None where the reference raises on the clamp bounds"""
    try:
        return mindssc(torch.from_numpy(c.img)[None, None], c.radius, c.dilation, device="cpu")[0].numpy()
    except RuntimeError as e:
        assert "overflow" in str(e), e
        return None


def main():
    from _ref_import import import_reference
    import mkl_tables
    from oracle import oracle
    utils, _ = import_reference()
    assert mkl_tables.host_tables(oracle)["matches_golden_host"], "this host's MKL tables differ from the golden host's"
    out = {}
    for threads in (8, 1):
        torch.set_num_threads(threads)
        for c in MC.CASES:
            r = reference_descriptor(utils.MINDSSC, c)
            rec = {}
            if r is None:
                rec["raises"] = np.array(1)
            else:
                rec["nan"], rec["ones"], rec["digest"] = np.array(int(np.isnan(r).sum())), np.array(int((r == 1).sum())), np.array(digest(r))
                if c.img.size <= ARRAY_VOXELS and not np.isnan(r).all():
                    rec["out"] = r
            for k, v in rec.items():
                key = "%s:%s" % (c.name, k)
                if threads == 8:
                    out[key] = v
                else:
                    assert key in out and np.array_equal(out[key], v, equal_nan=(k == "out")), "%s depends on the thread count" % key
    path = os.path.join(HERE, "mind_range.npz")
    np.savez_compressed(path, **out)
    print(len(MC.CASES), "cases,", len(out), "entries,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
