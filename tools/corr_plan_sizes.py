#!/usr/bin/env python
"""Prints cvx_correlate_workspace_bytes and cvx_register_pair_workspace_bytes over a fixed grid of channels, coarse shapes, search radii
and option sets -- every branch of the correlation stage's path selection (corr_plan, correlate.hip) -- as digests per option set and channel
count (--full: one line per case).  No GPU needed.
   python tools/corr_plan_sizes.py > profiles/corr_plan_sizes.txt
   python tools/corr_plan_sizes.py --coupled > profiles/coupled_plan_sizes.txt
--coupled: the same grid for the coupled-convex stage (coupled_plan, convex.hip) -- the option sets that stage reads added, and digests of
cvx_coupled_convex_workspace_bytes and cvx_convex_stage_workspace_bytes (ic_iters 0 and 2) beside the pair query's.
Callers cache these sizes: a change of the selection code must leave the listing identical (compare with the parent commit's)."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd import _lib                                             # noqa: E402

CHANNELS = (1, 4, 12, 15, 16, 20, 32, 33, 64, 128, 129, 255)
SHAPES = ((5, 6, 7), (12, 10, 14), (16, 16, 16), (26, 32, 37), (37, 32, 37), (40, 48, 40),
          (6, 40, 37), (5, 48, 56),                                         # tall planes: y tiles
          (4, 5, 300), (3, 4, 1300))                                        # long rows
HWS = (0, 1, 4, 6, 8, 9, 15)
OPTION_SETS = ({}, {"corr_unfused": 1}, {"corr_fused_all": 1}, {"corr_cert": 0}, {"corr_cert": 2}, {"cert_unfused": 1}, {"cert_unfused": 2}, {"corr_dual": 1})
COUPLED_OPTION_SETS = OPTION_SETS + ({"no_prune": 1}, {"prune_stream_above": 0}, {"prune_refine": 0})
GRID_SP = 2                                                                 # the pair query's volume is GRID_SP x the coarse shape, features given (n_feat = C)


def main(full, coupled):
    L = _lib.lib()
    if coupled:
        print("# --coupled: per option set and channel count, over the same shapes and radii: sha256[:16] of the cvx_coupled_convex_workspace_bytes values | of the\n"
              "# cvx_convex_stage_workspace_bytes values for ic_iters 0, 2 | of the cvx_register_pair_workspace_bytes values as below | largest of each.")
    else:
        print("# per option set and channel count, over %d shapes x %d search radii: sha256[:16] of the cvx_correlate_workspace_bytes values | of the\n"
              "# cvx_register_pair_workspace_bytes values for (ic, fp16_storage) = (0,0) (0,1) (1,0) (1,1) | largest of each.  --full prints every case." % (len(SHAPES), len(HWS)))
    for opts in COUPLED_OPTION_SETS if coupled else OPTION_SETS:
        old = {k: L.cvx_get_option(k.encode()) for k in opts}
        for k, v in opts.items():
            L.cvx_set_option(k.encode(), v)
        label = ",".join("%s=%d" % kv for kv in opts.items()) or "default"
        try:
            for c in CHANNELS:
                corr, pair, stage = [], [], []
                for h, w, d in SHAPES:
                    for hw in HWS:
                        corr.append(L.cvx_coupled_convex_workspace_bytes(h, w, d, hw) if coupled else L.cvx_correlate_workspace_bytes(c, h, w, d, hw))
                        for it in (0, 2) if coupled else ():
                            sp = _lib.StageParams(c, h, w, d, hw, GRID_SP, it, h * GRID_SP, w * GRID_SP, d * GRID_SP)
                            stage.append(L.cvx_convex_stage_workspace_bytes(C.byref(sp)))
                        for ic in (0, 1):
                            for f16 in (0, 1):
                                p = _lib.PairParams(h * GRID_SP, w * GRID_SP, d * GRID_SP, 1, 2, 1.25, GRID_SP, hw, 5, 0, GRID_SP, ic, c, 12.0)
                                p.fp16_storage = f16
                                pair.append(L.cvx_register_pair_workspace_bytes(C.byref(p)))
                        if full:
                            print("%s | %d | %d %d %d | %d | %d | %s" % (label, c, h, w, d, hw, corr[-1], " ".join(map(str, stage[-2:] + pair[-4:]))))
                if not full:
                    sha = lambda v: hashlib.sha256(" ".join(map(str, v)).encode()).hexdigest()[:16]
                    if coupled:
                        print("%-20s | C %3d | %s | %s | %s | %d %d %d" % (label, c, sha(corr), sha(stage), sha(pair), max(corr), max(stage), max(pair)))
                    else:
                        print("%-16s | C %3d | %s | %s | %d %d" % (label, c, sha(corr), sha(pair), max(corr), max(pair)))
        finally:
            for k, v in old.items():
                L.cvx_set_option(k.encode(), v)


if __name__ == "__main__":
    main("--full" in sys.argv, "--coupled" in sys.argv)
