#!/usr/bin/env python
"""Prints cvx_mindssc_workspace_bytes, cvx_mindssc_pooled_scratch_bytes and cvx_register_pair_workspace_bytes (images, n_feat = 0) over a fixed grid
of shapes, (radius, dilation), pooling windows and option sets -- every branch of the descriptor stage's kernel selection (mind_plan, mind.hip) --
as digests per option set and (radius, dilation) (--full: one line per case).  No GPU needed.
   python tools/mind_plan_sizes.py > profiles/mind_plan_sizes.txt
Callers cache these sizes: a change of the selection code must leave the listing identical (compare with the parent commit's;
CONVEXADAM_HIP_LIB selects the library)."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd import _lib                                             # noqa: E402

SHAPES = ((7, 6, 8), (6, 6, 6), (13, 19, 92), (12, 12, 20), (24, 20, 16), (36, 32, 32), (24, 24, 84), (9, 17, 33), (3, 4, 63),   # odd D, D % 4 = 0 and 2
          (160, 192, 224))
RD = ((1, 2), (1, 1), (2, 2), (3, 1), (3, 4))
WINDOWS = ((6, 2), (6, 3), (6, 6), (4, 2), (4, 4), (2, 2), (6, 0), (2, 6), (5, 0), (8, 2))     # g2 = 0: one pooling (pair: no Adam stage)
OPTION_SETS = ({}, {"mind_single": 1}, {"mind_single": 2}, {"mind_tiled": 1}, {"mind_blocked": 0}, {"mind_mean_threads": 8},
               {"mind_single": 1, "mind_mean_threads": 8})


def main(full):
    L = _lib.lib()
    print("# per option set and (radius, dilation), over %d shapes: sha256[:16] of the cvx_mindssc_workspace_bytes values | of the\n"
          "# cvx_mindssc_pooled_scratch_bytes values for %d window pairs | of the cvx_register_pair_workspace_bytes values (n_feat 0, ic 1) for the same pairs |\n"
          "# largest of each.  --full prints every case." % (len(SHAPES), len(WINDOWS)))
    for opts in OPTION_SETS:
        old = {k: L.cvx_get_option(k.encode()) for k in opts}
        for k, v in opts.items():
            L.cvx_set_option(k.encode(), v)
        label = ",".join("%s=%d" % kv for kv in opts.items()) or "default"
        try:
            for r, d in RD:
                ws, scratch, pair = [], [], []
                for H, W, D in SHAPES:
                    ws.append(L.cvx_mindssc_workspace_bytes(H, W, D, r, d))
                    for g1, g2 in WINDOWS:
                        scratch.append(L.cvx_mindssc_pooled_scratch_bytes(H, W, D, r, d, g1, g2))
                        p = _lib.PairParams(H, W, D, r, d, 1.25 if g2 else 0.0, g1, 2, 5, 0, g2 or g1, 1, 0, 1.0)
                        pair.append(L.cvx_register_pair_workspace_bytes(C.byref(p)))
                        if full:
                            print("%s | r %d d %d | %d %d %d | %d %d | %d | %d | %d" % (label, r, d, H, W, D, g1, g2, ws[-1], scratch[-1], pair[-1]))
                if not full:
                    sha = lambda v: hashlib.sha256(" ".join(map(str, v)).encode()).hexdigest()[:16]
                    print("%-36s | r %d d %d | %s | %s | %s | %d %d %d" % (label, r, d, sha(ws), sha(scratch), sha(pair), max(ws), max(scratch), max(pair)))
        finally:
            for k, v in old.items():
                L.cvx_set_option(k.encode(), v)


if __name__ == "__main__":
    main("--full" in sys.argv)
