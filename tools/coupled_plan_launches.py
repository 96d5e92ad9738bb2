#!/usr/bin/env python
"""Kernel launch lists of the coupled-convex stage over cases that reach every outcome of its plan (coupled_plan, convex.hip).
   python tools/coupled_plan_launches.py --case NAME            runs one case: one operator call, one masked convex stage, or one small whole pair
   python tools/coupled_plan_launches.py --collect OUT.json [NAME ..]  every (named) case in a fresh process under `rocprofv3 --kernel-trace` (no counters), one
                                                                at a time, each under its own time limit; stops at the first case that fails
   python tools/coupled_plan_launches.py --report A.json B.json > profiles/coupled_plan_launch_lists.txt
CONVEXADAM_HIP_LIB selects the library (the parent commit's build for A).  A change of the selection code must leave every list identical.
Collecting and reporting are tools/adam_plan_launches.py's."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import adam_plan_launches as apl                                            # noqa: E402

HW = 2
SCALAR, VEC4 = (5, 6, 7), (4, 6, 8)                                         # v = 210: the scalar kernels; v = 192: the 16-byte ones
PASSES = {"default": {}, "no_prune": {"no_prune": 1}, "stream_above_0": {"prune_stream_above": 0}, "refine_0": {"prune_refine": 0}}
# name -> (kind, shape, thread options, kind's argument: stage ic_iters / pair (ic, fp16_storage, options of a context in cvx_pair_params.ctx))
CASES = {"f32_%s_%s" % ("x".join(map(str, s)), tag): ("f32", s, o, None) for s in (SCALAR, VEC4) for tag, o in PASSES.items()}
for _tag in ("default", "no_prune"):
    CASES["f16_4x6x8_" + _tag] = ("f16", VEC4, PASSES[_tag], None)
    CASES["masked_5x6x7_" + _tag] = ("masked", SCALAR, PASSES[_tag], None)
    for _it in (0, 2):
        CASES["stage_5x6x7_ic%d_%s" % (_it, _tag)] = ("stage", SCALAR, PASSES[_tag], _it)
for _ic in (1, 0):
    for _tag, _o, _f16, _ctx in (("default_certified", {}, 0, None), ("exact_keys", {"corr_cert": 0}, 0, None),
                                 ("exact_no_prune", {"corr_cert": 0, "no_prune": 1}, 0, None), ("exact_corr_dual", {"corr_cert": 0, "corr_dual": 1}, 0, None),
                                 ("fp16_storage", {}, 1, None), ("no_prune_in_ctx_only", {}, 0, {"no_prune": 1})):
        CASES["pair_ic%d_%s" % (_ic, _tag)] = ("pair", (24, 28, 20), _o, (_ic, _f16, _ctx))


def run_case(name):
    import numpy as np
    import torch
    from convexadam_amd import _lib
    from convexadam_amd.context import Context
    kind, shape, opts, arg = CASES[name]
    L, dev = _lib.lib(), torch.device("cuda", 0)
    for k, v in opts.items():
        assert L.cvx_set_option(k.encode(), v) == 0, k
    h, w, d = shape
    K, sp = (2 * HW + 1) ** 3, _lib.stream_ptr(dev)
    gen = torch.Generator().manual_seed(7)
    if kind == "pair":
        ic, f16, ctx_opts = arg
        fix, mov = torch.rand(shape, generator=gen).to(dev), torch.rand(shape, generator=gen).to(dev)
        pp = _lib.PairParams(h, w, d, 1, 2, 1.25, 2, HW, 3, 0, 2, ic, 0, 1.0, 0, 2, 0, 0, f16)     # tools/adam_plan_launches.py's pair_ic
        ctx = Context(**ctx_opts) if ctx_opts else None
        if ctx:
            pp.ctx = ctx.handle
        out, dims = torch.empty((3, h, w, d), device=dev), (C.c_int * 3)()
        n = L.cvx_register_pair_workspace_bytes(C.byref(pp))
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        rc = L.cvx_register_pair_f32(_lib.ptr(fix), _lib.ptr(mov), None, None, C.byref(pp), _lib.ptr(out), C.cast(dims, C.c_void_p), _lib.ptr(ws), n, sp)
        print("# pair %s ic %d fp16_storage %d options %s ctx %s ws %d rc %d" % (shape, ic, f16, opts or "default", ctx_opts, n, rc))
    elif kind == "stage":
        Cn = 4
        ff, fm = torch.rand((Cn,) + shape, generator=gen).to(dev), torch.rand((Cn,) + shape, generator=gen).to(dev)
        mf, mm = (torch.rand(shape, generator=gen) < 0.6).to(torch.uint8).to(dev), (torch.rand(shape, generator=gen) < 0.6).to(torch.uint8).to(dev)
        p = _lib.StageParams(Cn, h, w, d, HW, 2, arg, 2 * h, 2 * w, 2 * d)
        n = L.cvx_convex_stage_workspace_bytes(C.byref(p))
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        coarse, hr = torch.empty((3,) + shape, device=dev), torch.empty((3, 2 * h, 2 * w, 2 * d), device=dev)
        rc = L.cvx_convex_stage_f32(_lib.ptr(ff), _lib.ptr(fm), _lib.ptr(mf), _lib.ptr(mm), C.byref(p), _lib.ptr(coarse), _lib.ptr(hr), _lib.ptr(ws), n, sp)
        print("# stage %s C %d ic_iters %d options %s ws %d rc %d" % (shape, Cn, arg, opts or "default", n, rc))
    else:
        # a paraboloid around a random displacement per cell plus noise: columns with a basin, so that the pruned passes list some boxes and settle others
        g = torch.stack(torch.meshgrid(*[torch.arange(2 * HW + 1) - float(HW)] * 3, indexing="ij")).reshape(3, K, 1, 1, 1)
        c = (torch.rand((3, 1) + shape, generator=gen) * 2 - 1) * HW
        ssd = ((g - c) ** 2).sum(0) * 1.5 + torch.rand((K,) + shape, generator=gen) * 0.3
        am = ssd.argmin(0).to(dev)
        vol = (ssd.half() if kind == "f16" else ssd).contiguous().to(dev)
        mesh = torch.from_numpy(np.ascontiguousarray(g.reshape(3, K).numpy()[::-1])).to(dev)           # fastest index first
        n = L.cvx_coupled_convex_workspace_bytes(h, w, d, HW)
        ws, out = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty((3,) + shape, device=dev)
        if kind == "masked":
            m = (torch.rand(shape, generator=gen) < 0.6).to(torch.uint8).to(dev)
            rc = L.cvx_coupled_convex_masked_f32(_lib.ptr(vol), _lib.ptr(am), _lib.ptr(mesh), _lib.ptr(m), h, w, d, HW, _lib.ptr(out), _lib.ptr(ws), n, sp)
        else:
            fn = L.cvx_coupled_convex_f16 if kind == "f16" else L.cvx_coupled_convex_f32
            rc = fn(_lib.ptr(vol), _lib.ptr(am), _lib.ptr(mesh), h, w, d, HW, _lib.ptr(out), _lib.ptr(ws), n, sp)
        print("# %s %s hw %d options %s ws %d rc %d" % (kind, shape, HW, opts or "default", n, rc))
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
