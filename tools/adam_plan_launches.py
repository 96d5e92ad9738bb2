#!/usr/bin/env python
"""Kernel launch lists of the Adam loop over cases that reach every outcome of its plan (adam_plan, adam.hip).
   python tools/adam_plan_launches.py --case NAME            runs one case: 3 iterations (the pair case: one small whole pair)
   python tools/adam_plan_launches.py --collect OUT.json [NAME ..]  every (named) case in a fresh process under `rocprofv3 --kernel-trace` (no counters), one at
                                                             a time, each under its own time limit; stops at the first case that fails
   python tools/adam_plan_launches.py --report A.json B.json > profiles/adam_plan_launch_lists.txt
CONVEXADAM_HIP_LIB selects the library (the parent commit's build for A).  A change of the selection code must leave every list identical."""
import csv
import ctypes as C
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SMALL = (6, 9, 30)
SMOOTHERS = {"none": None, "pools33": (0, (3, 3)), "kovesi": (0, (3, 5, 5)), "gauss": (1, (0.05, 0.25, 0.4, 0.25, 0.05))}
TILES = {"box_fwd_tile": 2000, "box_bwd_tile": 2000}
# name -> (mode, smoother, shape, options, grad_out: "given" / "null" / "offset" = one float behind a 16-byte boundary)
CASES = {"%s_%s" % (mode, sm): (mode, sm, SMALL, {}, "given") for mode in ("exact", "fast", "fast_all") for sm in SMOOTHERS}
CASES.update({
    "exact_5x9x124": ("exact", "none", (5, 9, 124), {}, "given"),
    "exact_4x8x132_long_rows_tiles": ("exact", "none", (4, 8, 132), {}, "given"),
    "exact_4x8x130_long_rows_lds": ("exact", "none", (4, 8, 130), {}, "given"),
    "exact_bench_grid_auto_tiles": ("exact", "none", (80, 96, 112), {}, "given"),
    "opt_box_tiled": ("exact", "none", (12, 8, 56), {"box_tiled": 1}, "given"),
    "opt_fwd_tiles_bwd_march": ("exact", "none", (12, 8, 56), {"box_bwd_tile": 0, "box_fwd_tile": 2000}, "given"),
    "opt_bwd_tile_1000": ("exact", "none", (12, 8, 56), {"box_bwd_tile": 1000}, "given"),
    "opt_no_prediv": ("exact", "none", (12, 8, 56), dict(TILES, box_prediv=0), "given"),
    "grad_given_tiles": ("exact", "none", (12, 8, 56), TILES, "given"),
    "grad_null_tiles": ("exact", "none", (12, 8, 56), TILES, "null"),
    "grad_offset_tiles": ("exact", "none", (12, 8, 56), TILES, "offset"),
    "pair_ic": ("pair", "none", (24, 28, 20), {}, "null"),
})


def run_case(name):
    import torch
    from convexadam_amd import _lib
    from convexadam_amd import convex_adam_utils as U
    mode, sm, shape, opts, grad = CASES[name]
    L, dev = _lib.lib(), torch.device("cuda", 0)
    for k, v in opts.items():
        assert L.cvx_set_option(k.encode(), v) == 0, k
    g = torch.Generator().manual_seed(7)
    if mode == "pair":                          # keep_state = false: last gradient skipped; feature records from the MIND pass
        H, W, D = shape
        fix, mov = torch.rand(shape, generator=g).to(dev), torch.rand(shape, generator=g).to(dev)
        pp = _lib.PairParams(H, W, D, 1, 2, 1.25, 2, 2, 3, 0, 2, 1, 0, 1.0, 0, 2, 0, 0, 0)
        out, dims = torch.empty((3, H, W, D), device=dev), (C.c_int * 3)()
        n = L.cvx_register_pair_workspace_bytes(C.byref(pp))
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        rc = L.cvx_register_pair_f32(_lib.ptr(fix), _lib.ptr(mov), None, None, C.byref(pp), _lib.ptr(out), C.cast(dims, C.c_void_p), _lib.ptr(ws), n,
                                     _lib.stream_ptr(dev))
        print("# pair %s ic 1 ws %d rc %d" % (shape, n, rc))
    else:
        h, w, d = shape
        Cn, V3 = 4, 3 * h * w * d
        F2, M2 = torch.rand((Cn,) + shape, generator=g).to(dev), torch.rand((Cn,) + shape, generator=g).to(dev)
        P = (0.7 * torch.randn(V3, generator=g)).to(dev)
        m, v, Ud = torch.zeros(V3, device=dev), torch.zeros(V3, device=dev), torch.zeros(V3, device=dev)
        G = None if grad == "null" else torch.zeros(V3 + 4, device=dev)[(1 if grad == "offset" else 0):][:V3]
        assert G is None or G.data_ptr() % 16 == (4 if grad == "offset" else 0)
        bh, bw, bd = U._base_tables(h, w, d, dev)
        spec = None
        if SMOOTHERS[sm]:
            kind, vals = SMOOTHERS[sm]
            spec = _lib.Smoother(kind, 0 if kind else len(vals), (C.c_int * 4)(*(() if kind else vals)), (C.c_float * 5)(*(vals if kind else ())))
        n = L.cvx_adam_workspace_bytes(Cn, h, w, d)
        ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
        rc = L.cvx_adam_run_mode_f32(_lib.ptr(F2), _lib.ptr(M2), Cn, h, w, d, _lib.ptr(P), _lib.ptr(m), _lib.ptr(v), 1.25, 3, 0, 12.0, _lib.ptr(bh),
                                     _lib.ptr(bw), _lib.ptr(bd), _lib.ptr(Ud), _lib.ptr(G), None, 0, None, C.byref(spec) if spec else None,
                                     ("exact", "fast", "fast_all").index(mode), _lib.ptr(ws), n, _lib.stream_ptr(dev))
        print("# %s smoother %s %s options %s grad_out %s rc %d" % (mode, sm, shape, opts or "default", grad, rc))
    torch.cuda.synchronize()
    assert rc == 0, L.cvx_last_error()


def collect(out_path, names, limit_s=180, cases=None, script=__file__):
    """cases / script: another tool's case table and file (tools/mind_plan_launches.py), run as `script --case NAME`"""
    res = {}
    for name in names or cases or CASES:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["timeout", "-k", "10", str(limit_s), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--",
                   sys.executable, os.path.abspath(script), "--case", name]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:
                sys.exit("case %s: exit status %d -- stopping here\n%s" % (name, r.returncode, r.stdout[-3000:]))
            rows = [row for f in glob.glob(tmp + "/**/*kernel_trace.csv", recursive=True) for row in csv.DictReader(open(f))]
        rows.sort(key=lambda row: int(row.get("Dispatch_Id") or row["Start_Timestamp"]))
        launches = [(row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("cvx::", ""),
                     "x".join(row["Grid_Size_" + a] for a in "XYZ"), "x".join(row["Workgroup_Size_" + a] for a in "XYZ"))
                    for row in rows if "cvx::" in row["Kernel_Name"]]
        res[name] = {"calls": [l for l in r.stdout.splitlines() if l.startswith("# ")], "launches": launches, "other_kernels": len(rows) - len(launches)}
        print("%-34s %4d launches" % (name, len(launches)), flush=True)
        json.dump(res, open(out_path, "w"), indent=0)


def report(a_path, b_path, cases=None):
    cases = cases or CASES
    A, B = json.load(open(a_path)), json.load(open(b_path))
    sha = lambda ls: hashlib.sha256(json.dumps(ls).encode()).hexdigest()[:16]
    names = [n for n in cases if n in A and n in B]
    same = all(A[n]["launches"] == B[n]["launches"] and A[n]["calls"] == B[n]["calls"] for n in names)
    print("# %d of %d cases, parent and new lists %s" % (len(names), len(cases), "IDENTICAL in every case" if same else "DIFFER"))
    for name in names:
        a, b = A[name]["launches"], B[name]["launches"]
        print("== %s: %d launches, sha256 %s (parent) %s %s (new)" % (name, len(b), sha(a), "=" if a == b else "!=", sha(b)))
        for l in B[name]["calls"]:
            print("  " + l)
        runs = []
        for l in b:                              # identical consecutive launches once, with their count
            if runs and runs[-1][0] == l:
                runs[-1][1] += 1
            else:
                runs.append([l, 1])
        for (k, grid, wg), n in runs:
            print("  %s%s grid %s wg %s" % ("%d x " % n if n > 1 else "", k, grid, wg))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--case"]:
        run_case(sys.argv[2])
    elif sys.argv[1:2] == ["--collect"]:
        collect(sys.argv[2], sys.argv[3:])
    elif sys.argv[1:2] == ["--report"]:
        report(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
