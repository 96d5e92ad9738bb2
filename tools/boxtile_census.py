#!/usr/bin/env python
"""Per-pass clocks of the three-box tiles of the exact Adam loop (option tile_census_ptr, boxtile.hip k_box3_tile), one block per option set:
    python tools/boxtile_census.py "box_tile_sync=0" "box_tile_sync=1"
For each wavefront the kernel records {start, pass 1 done, barrier 1 passed, pass 2 done, barrier 2 passed, pass 3 done} (100 MHz ticks); with
box_tile_sync=1 the "barrier passed" stamps are the end of the wavefront's first flag wait of the next pass.  Printed per kernel, medians over
workgroups, in us from the workgroup's first start: when the last wavefront finished each pass, the mean time a wavefront spent between
finishing a pass and starting the next one, and the workgroup's life."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convexadam_amd import convex_adam_utils as U   # noqa: E402
from convexadam_amd import _lib                     # noqa: E402

NW, SLOT = 16, 8 * 16 * 1024                         # wavefronts per workgroup (kind 2 tiles), words per kernel
L = _lib.lib()
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(3)
h, w, d = 80, 96, 112
F2 = torch.rand(1, 12, h, w, d, generator=g).to(dev)
M2 = torch.rand(1, 12, h, w, d, generator=g).to(dev)
P0 = Fn.interpolate(torch.randn(1, 3, 5, 6, 7, generator=g) * 2.0, size=(h, w, d), mode="trilinear").to(dev)


def report(name, c):
    c = c.reshape(-1, NW, 8).astype(np.int64)
    c = c[c[:, 0, 0] != 0]
    if not len(c):
        print("  %-22s no records" % name)
        return
    t0 = c[:, :, 0].min(1)[:, None]
    rel = (c[:, :, :6] - t0[:, :, None]) / 100.0                     # us from the workgroup's first start
    rel[c[:, :, :6] == 0] = np.nan
    p1, p2, p3 = np.nanmax(rel[:, :, 1], 1), np.nanmax(rel[:, :, 3], 1), np.nanmax(rel[:, :, 5], 1)
    gap1 = np.nanmean(rel[:, :, 2] - rel[:, :, 1], 1)
    gap2 = np.nanmean(rel[:, :, 4] - rel[:, :, 3], 1)
    first1 = np.nanmin(rel[:, :, 1], 1)
    print("  %-22s %4d wg | pass 1 first wave done %.2f, all done %.2f | pass 2 all done %.2f | pass 3 all done (life) %.2f us | "
          "wave idle pass 1 -> 2 %.2f, pass 2 -> 3 %.2f us (medians; life p90 %.2f)" % (
              name, len(c), np.median(first1), np.median(p1), np.median(p2), np.median(p3), np.median(gap1), np.median(gap2),
              np.percentile(p3, 90)))


for spec in sys.argv[1:] or [""]:
    opts = dict(kv.split("=") for kv in spec.split(",") if kv)
    old = {k: L.cvx_get_option(k.encode()) for k in opts}
    for k, v in opts.items():
        assert L.cvx_set_option(k.encode(), int(v)) == 0, k
    try:
        U.adam_run(F2, M2, P0, 1.25, 10, return_state=True)
        torch.cuda.synchronize()
        buf = torch.zeros(2 * SLOT, dtype=torch.int64, device=dev)
        L.cvx_set_option(b"tile_census_ptr", buf.data_ptr())
        U.adam_run(F2, M2, P0, 1.25, 10, return_state=True)       # every launch overwrites: the last iteration's stamps remain
        torch.cuda.synchronize()
        L.cvx_set_option(b"tile_census_ptr", 0)
        c = buf.cpu().numpy()
        print(spec or "(default)")
        report("forward boxes", c[:SLOT])
        report("adjoint boxes + Adam", c[SLOT:])
    finally:
        L.cvx_set_option(b"tile_census_ptr", 0)
        for k, v in old.items():
            L.cvx_set_option(k.encode(), v)
