"""Goldens for tests/test_coupled_range_reference.py: the reference's coupled_convex on the cost volumes of tests/coupled_range_cases.py,
captured from the reference itself (run ONLY in the build container, the reference tree is not on the other hosts):

    python tests/golden/make_golden_coupled_range.py        # -> tests/golden/coupled_range.npz

The inputs are rebuilt from seeds by tests/coupled_range_cases.py; only the reference's output fields are stored: '<case name>:<seed>' ->
[3, h, w, d] float32 for both seeds of every case, run in torch CPU float32 on the values the passes see (a masked case: ssd * mask with
clean zeros, the product l2r_2020_convexAdam_CuRIOUS.py:336-338 forms).  The large geometry is captured too unless the file would pass
MAX_BYTES; the cases left out are then pinned by the torch composition of the test alone.  torch runs with 8 threads, as for every other
golden, and once more with 1: the captures must not depend on it (asserted)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import coupled_range_cases as CC  # noqa: E402

MAX_BYTES = 380 * 1024


def mesh_of(hw):
    n = 2 * hw + 1
    return torch.nn.functional.affine_grid(hw * torch.eye(3, 4).unsqueeze(0), (1, 1, n, n, n), align_corners=True).permute(0, 4, 1, 2, 3).reshape(3, -1, 1)


def reference_field(coupled_convex, c, which):
    """[3, h, w, d] float32: the reference on the values the passes see"""
    ssd = torch.from_numpy(np.array(c.seen()))
    am = torch.from_numpy(np.array(c.seed(which)))
    return coupled_convex(ssd, am, mesh_of(c.hw), 1, c.shape)[0].numpy()


def capture(coupled_convex, cases):
    out = {}
    for threads in (8, 1):
        torch.set_num_threads(threads)
        for c in cases:
            for which in CC.SEEDS:
                key, r = "%s:%s" % (c.name, which), reference_field(coupled_convex, c, which)
                assert r.shape == (3,) + c.shape and r.dtype == np.float32
                if threads == 8:
                    out[key] = r
                else:
                    assert np.array_equal(out[key], r, equal_nan=True), "%s depends on the thread count" % key
    return out


def main():
    from _ref_import import import_reference
    from oracle import oracle
    utils, _ = import_reference()
    for _, hw, _ in CC.GEOMETRIES + (CC.LARGE,):
        assert np.array_equal(mesh_of(hw)[:, :, 0].numpy(), oracle.disp_mesh(hw))
    path = os.path.join(HERE, "coupled_range.npz")
    for cases in (CC.CASES, [c for c in CC.CASES if not c.large]):
        out = capture(utils.coupled_convex, cases)
        np.savez_compressed(path, **out)
        if os.path.getsize(path) <= MAX_BYTES:
            break
    print(len(cases), "of", len(CC.CASES), "cases,", len(out), "fields,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= MAX_BYTES


if __name__ == "__main__":
    main()
