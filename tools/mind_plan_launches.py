#!/usr/bin/env python
"""Kernel launch lists of the MIND-SSC stage over cases that reach every outcome of its plan (mind_plan, mind.hip).
   python tools/mind_plan_launches.py --case NAME            runs one case: one operator call, or one small whole pair
   python tools/mind_plan_launches.py --collect OUT.json [NAME ..]  every (named) case in a fresh process under `rocprofv3 --kernel-trace` (no counters), one at
                                                             a time, each under its own time limit; stops at the first case that fails
   python tools/mind_plan_launches.py --report A.json B.json > profiles/mind_plan_launch_lists.txt
CONVEXADAM_HIP_LIB selects the library (the parent commit's build for A).  A change of the selection code must leave every list identical.
Collecting and reporting are tools/adam_plan_launches.py's."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import adam_plan_launches as apl                                            # noqa: E402

POOLED = (13, 19, 92)
# name -> (kind, shape, (radius, dilation), (g1, g2), options, fp16_storage)
CASES = {
    "full_3x9x8": ("full", (3, 9, 8), (1, 2), None, {}, 0),
    "full_7x17x68": ("full", (7, 17, 68), (1, 2), None, {}, 0),
    "full_5x8x32_narrow_march": ("full", (5, 8, 32), (1, 2), None, {}, 0),
    "full_4x8x128_wide_march": ("full", (4, 8, 128), (1, 2), None, {}, 0),
    "full_r3d4_9x9x33_k_mind_3_32": ("full", (9, 9, 33), (3, 4), None, {}, 0),
    "full_3x9x8_mind_tiled": ("full", (3, 9, 8), (1, 2), None, {"mind_tiled": 1}, 0),
    "full_36x32x32_mean_threads_8": ("full", (36, 32, 32), (1, 2), None, {"mind_mean_threads": 8}, 0),
}
for _g in ((6, 2), (4, 4), (2, 6)):
    for _tag, _o in (("default", {}), ("single1", {"mind_single": 1}), ("single2", {"mind_single": 2}), ("blocked0", {"mind_blocked": 0})):
        CASES["pooled_%dx%d_%s" % (_g + (_tag,))] = ("pooled", POOLED, (1, 2), _g, _o, 0)
CASES.update({
    "pooled_6x2_r2_planar_two_pass": ("pooled", POOLED, (2, 2), (6, 2), {}, 0),
    "pair_ic_records": ("pair", (24, 28, 20), (1, 2), (2, 2), {"mind_records": 1}, 0),
    "pair_ic_no_records": ("pair", (24, 28, 20), (1, 2), (2, 2), {"mind_records": 0}, 0),
    "pair_ic_fp16_storage": ("pair", (24, 28, 20), (1, 2), (2, 2), {}, 1),
    "pair_ic_single1_records": ("pair", (24, 28, 20), (1, 2), (2, 2), {"mind_single": 1, "mind_records": 1}, 0),      # records written by the marching kernel
    "pair_ic_single1_fp16_storage": ("pair", (24, 28, 20), (1, 2), (2, 2), {"mind_single": 1}, 1),
})


def run_case(name):
    import torch
    from convexadam_amd import _lib
    kind, shape, (r, d), g, opts, f16 = CASES[name]
    L, dev = _lib.lib(), torch.device("cuda", 0)
    for k, v in opts.items():
        assert L.cvx_set_option(k.encode(), v) == 0, k
    H, W, D = shape
    gen = torch.Generator().manual_seed(7)
    img = torch.rand(shape, generator=gen).to(dev)
    nws = L.cvx_mindssc_workspace_bytes(H, W, D, r, d)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
    if kind == "full":
        out = torch.empty((12,) + shape, device=dev)
        rc = L.cvx_mindssc_f32(_lib.ptr(img), H, W, D, r, d, _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream_ptr(dev))
        print("# full %s r %d d %d options %s ws %d rc %d" % (shape, r, d, opts or "default", nws, rc))
    elif kind == "pooled":
        g1, g2 = g
        o1, o2 = torch.empty(12 * (H // g1) * (W // g1) * (D // g1), device=dev), torch.empty(12 * (H // g2) * (W // g2) * (D // g2), device=dev)
        nsc = L.cvx_mindssc_pooled_scratch_bytes(H, W, D, r, d, g1, g2)
        sc = torch.empty(max(nsc, 16), dtype=torch.uint8, device=dev)
        rep = C.c_int(-1)
        rc = L.cvx_mindssc_pooled_f32(_lib.ptr(img), H, W, D, r, d, g1, _lib.ptr(o1), g2, _lib.ptr(o2), _lib.ptr(sc) if nsc else None, nsc, _lib.ptr(ws), nws,
                                      C.byref(rep), _lib.stream_ptr(dev))
        print("# pooled %s r %d d %d windows %s options %s scratch %d ws %d rc %d repaired %d" % (shape, r, d, g, opts or "default", nsc, nws, rc, rep.value))
    else:
        mov = torch.rand(shape, generator=gen).to(dev)
        pp = _lib.PairParams(H, W, D, r, d, 1.25, g[0], 2, 3, 0, g[1], 1, 0, 1.0, 0, 2, 0, 0, f16)
        out, dims = torch.empty((3, H, W, D), device=dev), (C.c_int * 3)()
        n = L.cvx_register_pair_workspace_bytes(C.byref(pp))
        pws = torch.empty(n, dtype=torch.uint8, device=dev)
        rc = L.cvx_register_pair_f32(_lib.ptr(img), _lib.ptr(mov), None, None, C.byref(pp), _lib.ptr(out), C.cast(dims, C.c_void_p), _lib.ptr(pws), n,
                                     _lib.stream_ptr(dev))
        print("# pair %s ic 1 options %s fp16_storage %d ws %d rc %d" % (shape, opts or "default", f16, n, rc))
    torch.cuda.synchronize()
    assert rc == 0, L.cvx_last_error()


if __name__ == "__main__":
    if sys.argv[1:2] == ["--case"]:
        run_case(sys.argv[2])
    elif sys.argv[1:2] == ["--collect"]:
        apl.collect(sys.argv[2], sys.argv[3:], cases=CASES, script=__file__)
    elif sys.argv[1:2] == ["--report"]:
        apl.report(sys.argv[2], sys.argv[3], cases=CASES)
    else:
        sys.exit(__doc__)
