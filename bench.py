#!/usr/bin/env python
"""bench.py -- pairs/s of the convexAdam hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one full registration of a 160x192x224 pair (BASELINE.json configs[1]: MIND-SSC r=1 d=2,
grid_sp 6, disp_hw 6, inverse consistency, lambda 1.25, grid_sp_adam 2, 80 Adam iterations, float32)
through the C ABI (cvx_register_pair_f32) in the package's default mode (every operator's result in the reference's evaluation order; the
field is bit-identical to the CPU oracle's), inputs already resident in HBM.  With N GPUs every rank
registers its own pairs (no collective on the data path); the timed region is bracketed by
barrier + synchronize and the slowest rank's time is used: value = N*K / T (weak scaling).

A plain run does what `value` needs and no more: it generates the pair, warms up, times the steps, writes --dump-outputs and prints the
line with the contract keys, stages_ms and roofline (both read from HIP events the timed steps record themselves).  Everything else below
-- cpu_baseline and the parity verdicts, the other modes and storage types, configs, batched, the per-kernel figures -- runs after the
timed steps with --full only (minutes; --no-cpu-baseline / --no-batched leave out its two halves):

    python bench.py --gpus 1 --steps K --warmup W --full

The printed line stays under 8 KB (bench_line): the contract keys, roofline, stages_ms and, with --full, cpu_baseline, the mode values, the
parity verdict and one figure per secondary config.  With --full the whole record, every object below included, goes to --extra-out
(default bench_extra.json next to this script).
  roofline     the SSD correlation stage (k_corr_prep + k_corr_fused of one direction, certified-fast arithmetic): algorithmic bytes
               (n^3*v*4 written + 2*C*v*4 read = 273.5 MB) / its mean duration measured with HIP events on the
               launch stream inside the timed region, against 8 TB/s HBM3E peak; `traffic` = HBM bytes per launch
               from the committed rocprofv3 PMC passes (profiles/pmc_hbm_traffic.json: 2*FETCH_SIZE + WRITE_SIZE).
  cpu_baseline the CPU oracle (kind "port", OpenMP over all host cores) timed on one full pair of the same
               workload, rank 0 / N=1 only.  It is the checker, timed as a baseline -- never the product.
  configs      BASELINE configs[2..4] (224x192x224 masked hw 8; 32-channel nnUNet features; a slice of the two-stage sweep) timed on the same
               GPU outside the timed region of `value`, each with the roofline fraction of its correlation stage.
  batched      pairs/s with 2 / 3 / 4 pairs in flight on one GPU (cvx_register_pairs_f32), exact and fast Adam modes.

--dump-outputs DIR writes the field of the last timed step (rank 0) under DIR as .npy files: a fixed, seeded sample of its voxels and
its whole-field moments (dump_outputs).  The inputs are seeded, so two builds run with the same arguments can be compared file by file.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPE = (160, 192, 224)
CFG = dict(mind_r=1, mind_d=2, lambda_weight=1.25, grid_sp=6, disp_hw=6, selected_niter=80, selected_smooth=0,
           grid_sp_adam=2, ic=True)
# the mode `value` is timed in = what the package ships as its default since round 5: every operator's RESULT in the reference's evaluation
# order (adam_mode="exact"; the field is bit-identical to oracle/cvx_oracle.c -- `parity.bit_identical`).  Since round 6 the convex stage
# reaches those bits through the certified-fast correlation (a cost volume within 2^-17 of ATen's + certified argmin
# decisions; option corr_cert).  The line also carries `value_fast_mode` (opt-in adam_mode="fast": the Adam loop in throughput arithmetic,
# graded by end-point error against four full-size captures of the reference, `parity.fast_mode`) and `value_at_tolerance` (the
# reference-bits mode, the only one inside the literal 1e-3 at 80 iterations).  TIMED_MODE_NAME goes into the JSON line.
EXACT = dict(CFG, adam_mode="exact")            # every operator in the reference's evaluation order (CFG alone takes the package default, which is this)
FAST = dict(CFG, adam_mode="fast")
TIMED = EXACT
TIMED_MODE_NAME = ("adam_mode=exact (the package default: MIND, correlation argmins, coupled convex, inverse consistency and every operator of the Adam loop "
                   "produce the reference's bits; bit-identical to oracle/cvx_oracle.c)")
HBM_PEAK_GBS = 8000.0
TOLERANCE_EPE = 1e-3          # north_star: mean end-point error against the reference's field, voxels
DUMP_SAMPLE = 1 << 22         # voxels of the field written by --dump-outputs: 3 x 4 Mi x 4 B = 48 MiB (the whole field is 79 MiB)
DUMP_SEED = 0


def make_pair(device, idx):
    """multi-octave phantom, moving = other noise realisation warped by a smooth field."""
    from convexadam_amd.phantom import deformed_pair
    fix, mov = deformed_pair(SHAPE, idx, 4.0)
    return fix.to(device).contiguous(), mov.to(device).contiguous()


CORR_SOURCES = ("corrfused.hip", "correlate.hip", "corrbox.hip", "corrcert.hip", "certify.hip")


def corr_sources_sha():
    """sha256 over the sources of the correlation stage: what the committed PMC traffic figure was measured on."""
    import hashlib
    h = hashlib.sha256()
    for name in CORR_SOURCES:
        with open(os.path.join(ROOT, "convexadam_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def pmc_traffic():
    """HBM bytes per correlation-stage launch from the last committed rocprofv3 PMC passes (profiles/pmc_hbm_traffic.json, written by
    tools/make_profiles.py: a PMC pass cannot run inside the timed loop) -> (bytes or None, commit it was measured at, stale flag:
    the kernel sources changed since)."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_hbm_traffic.json")) as f:
            j = json.load(f)
        return float(j["correlate_stage_bytes_per_launch"]), j.get("measured_at_commit"), j.get("corr_sources_sha16") != corr_sources_sha()
    except Exception:
        return None, None, True


def pmc_extra(key):
    """Another figure of profiles/pmc_hbm_traffic.json (None when absent)."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_hbm_traffic.json")) as f:
            v = json.load(f).get(key)
        return float(v) if v is not None else None
    except Exception:
        return None


def reference_bits_check(fix, mov, dev):
    """Outside every timed region of `value`: the same pair in reference-bits mode -- the reference build's exp / sqrt as tables of the
    host that produced tests/golden (fixtures: mkl_vsexp_codes.xz, mkl_vssqrt_low.npz) and torch's 8-thread mean -- compared with the
    field captured from the reference itself (tests/golden/fullsize.npz, every 8th voxel per axis + float64 sums).  Data files only."""
    import lzma
    import numpy as np
    from convexadam_amd import reference_bits as rb
    from convexadam_amd.convex_adam_MIND import register_pair_device
    from convexadam_amd.convex_adam_utils import sqrt_codes_from_low_bitmaps
    gd = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gd, "mkl_vsexp_codes.xz"), "rb") as f:
        exp_tbl = np.frombuffer(lzma.decompress(f.read()), np.uint8)
    q = np.load(os.path.join(gd, "mkl_vssqrt_low.npz"))
    g = np.load(os.path.join(gd, "fullsize.npz"))
    rb.set_mind_exp_table(exp_tbl, device=dev)
    rb.set_adam_sqrt_table(sqrt_codes_from_low_bitmaps(q["normal"], q["denormal"]), device=dev)
    rb.set_mean_threads(8)
    horizons = (20, 40, 80)
    golden_host = {}
    try:
        for _ in range(2):
            f = register_pair_device(fix, mov, **EXACT)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(5):
            f = register_pair_device(fix, mov, **EXACT)
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) / 5 * 1e3
        for n in horizons:
            golden_host[n] = f if n == CFG["selected_niter"] else register_pair_device(fix, mov, **dict(EXACT, selected_niter=n))
    finally:
        rb.disable()
    # the reference's own reproducibility ACROSS HOSTS: the same reference-bits pipeline with the tables of the golden host (a Xeon) and
    # with the tables of THIS host's torch (MKL picks its exp / sqrt code path by CPU model) -- two installs of the reference, one pair
    cross = None
    try:
        rb.enable(dev, threads=8)
        cross = {}
        for n in horizons:
            g2 = register_pair_device(fix, mov, **dict(EXACT, selected_niter=n))
            cross["epe_%dit" % n] = float((g2 - golden_host[n]).square().sum(0).sqrt().mean())
    except Exception as e:                                      # a host whose torch has no MKL path etc.: report, do not fail the bench
        cross = {"error": repr(e)}
    finally:
        rb.disable()
    s = int(g["sub"])
    got_sub = f[:, ::s, ::s, ::s].cpu().numpy()
    sub_equal = bool(np.array_equal(got_sub, g["c1_adam_80_sub"]))
    epe_sub = float(np.sqrt(((got_sub.astype(np.float64) - g["c1_adam_80_sub"].astype(np.float64)) ** 2).sum(0)).mean())
    fd = f.cpu().double()
    sums_equal = bool(np.allclose(fd.sum((1, 2, 3)).numpy(), g["c1_adam_80_sum"], rtol=1e-14, atol=0)
                      and np.allclose(fd.square().sum((1, 2, 3)).numpy(), g["c1_adam_80_sumsq"], rtol=1e-14, atol=0))
    return dict(bit_identical_to_reference_capture=sub_equal and sums_equal, ms_per_pair=ms, pairs_per_s=1e3 / ms,
                epe_vs_reference_80it=epe_sub, tolerance_met=bool(epe_sub < TOLERANCE_EPE),
                reference_cross_host=dict(cross or {}, this_host_cpu=host_cpu_model(), golden_host_cpu="Intel Xeon (AVX-512), the build container that captured tests/golden",
                                          note="mean EPE (whole field, voxels) between the reference-bits pipeline with the GOLDEN host's MKL "
                                          "tables and with THIS host's (reference_bits.enable: built from this host's torch.exp / torch.sqrt), 8-thread mean "
                                          "in both (exact Adam mode): how far two installs of the reference are from each other on this pair.  MKL dispatches on the CPU "
                                          "model, so the figure belongs to THIS host's CPU"),
                note="opt-in mode (convexadam_amd/reference_bits.py): MKL vsExp / vsSqrt of the golden host as tables + torch's 8-thread "
                     "mean; compared with the field captured from the reference at 80 iterations (tests/golden/fullsize.npz: every 8th "
                     "voxel per axis bit for bit, float64 sum and sum of squares of the whole field to 1e-14)")


def epe_vs_reference(hip_field, niter=80):
    """Mean EPE of a HIP field against the field captured from the reference itself after `niter` Adam iterations on this very pair
    (tests/golden/fullsize.npz holds every 8th voxel per axis for 1 / 20 / 40 / 80 iterations)."""
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "fullsize.npz"))
    s = int(g["sub"])
    d = hip_field[:, ::s, ::s, ::s].astype(np.float64) - g["c1_adam_%d_sub" % niter].astype(np.float64)
    return float(np.sqrt((d ** 2).sum(0)).mean())


CAPTURES = ("c1", "c4", "c5", "c6")


def capture_registration(tag, dev):
    """(golden dict, shape, callable(mode, niter) -> (3,H,W,D) device field) for one full-size capture of the reference
    (tests/golden/fullsize.npz: c1 = the benchmark pair; fullsize2.npz: c4 another seed / 6-voxel warp, c5 exact-zero background, c6 18-label
    maps through the nnUNet path).  Inputs are regenerated from seeds (convexadam_amd/phantom.py); data files only."""
    import numpy as np
    from convexadam_amd import phantom as ph
    from convexadam_amd.convex_adam_MIND import register_pair_device
    g = np.load(os.path.join(ROOT, "tests", "golden", "fullsize.npz" if tag == "c1" else "fullsize2.npz"))
    if tag == "c6":
        from convexadam_amd.convex_adam_nnUNet import extract_features
        shape = (160, 192, 160)
        lab, labm = ph.warped_label_pair(shape, 18, 11, 0.05)
        ff, fm = extract_features(lab, labm, device=dev)
        return g, shape, lambda mode, n: register_pair_device(feat_fixed=ff[0], feat_moving=fm[0], **dict(CFG, adam_mode=mode, selected_niter=n))
    shape = SHAPE
    a, b = {"c1": lambda: ph.deformed_pair(shape, 0, 4.0), "c4": lambda: ph.deformed_pair(shape, 2, 6.0), "c5": lambda: ph.zero_background_pair(shape, 0, 4.0)}[tag]()
    a, b = a.to(dev).contiguous(), b.to(dev).contiguous()
    return g, shape, lambda mode, n: register_pair_device(a, b, **dict(CFG, adam_mode=mode, selected_niter=n))


def mode_parity(fix, mov, dev, oracle_fast_field=None):
    """Outside the timed region: the timed (exact, reference-order) mode and the opt-in fast Adam mode against FOUR full-size captures of the
    reference at 1 / 20 / 40 / 80 iterations, next to the reference's distance from a 1-ulp-perturbed copy of itself, and the fast modes' own speed."""
    import numpy as np
    from convexadam_amd.convex_adam_MIND import register_pair_device

    def epe_sub(field, g, tag, n):
        s_ = int(g["sub"])
        d = field[:, ::s_, ::s_, ::s_].cpu().numpy().astype(np.float64) - g["%s_adam_%d_sub" % (tag, n)].astype(np.float64)
        return float(np.sqrt((d ** 2).sum(0)).mean())

    caps = {}
    for tag in CAPTURES:
        g, shape, reg = capture_registration(tag, dev)
        snaps = [int(v) for v in g[tag + "_snaps"]]
        self_p = [float(v) for v in g[tag + "_self_perturbation_epe_sub"]]
        e = {"epe_vs_reference_%dit" % n: epe_sub(reg("fast", n), g, tag, n) for n in snaps}
        e["exact_mode_epe_vs_reference_80it"] = epe_sub(reg("exact", 80), g, tag, 80)
        e["reference_self_perturbation_epe"] = dict(zip(["%dit" % n for n in snaps], self_p))
        e["ratio_to_self_perturbation_80it"] = e["epe_vs_reference_80it"] / self_p[snaps.index(80)]
        e["ratio_to_exact_mode_80it"] = e["epe_vs_reference_80it"] / e["exact_mode_epe_vs_reference_80it"]
        e["criteria_round3"] = dict(epe_1it_le_1em6=bool(e["epe_vs_reference_1it"] <= 1e-6), epe_20it_lt_1em3=bool(e["epe_vs_reference_20it"] < 1e-3),
                                    epe_40it_lt_1em3=bool(e["epe_vs_reference_40it"] < 1e-3),
                                    epe_80it_le_reference_self_perturbation=bool(e["ratio_to_self_perturbation_80it"] <= 1.0),
                                    epe_80it_le_1p15x_exact_mode=bool(e["ratio_to_exact_mode_80it"] <= 1.15))
        caps[tag] = e
        del reg
        torch.cuda.empty_cache()
    out = {"fast_mode": dict(caps["c1"]), "exact_mode": {}}
    for n in (1, 20, 40, 80):
        out["exact_mode"]["epe_vs_reference_%dit" % n] = epe_vs_reference(register_pair_device(fix, mov, **dict(EXACT, selected_niter=n)).cpu().numpy(), n)
    out["exact_mode"]["epe_vs_reference_80it_by_capture"] = {c: caps[c]["exact_mode_epe_vs_reference_80it"] for c in CAPTURES}
    out["exact_mode"]["reference_self_perturbation_epe_80it_by_capture"] = {c: caps[c]["reference_self_perturbation_epe"]["80it"] for c in CAPTURES}
    out["exact_mode"]["tolerance_met_80it"] = bool(out["exact_mode"]["epe_vs_reference_80it"] < TOLERANCE_EPE)
    out["exact_mode"]["note"] = ("the PACKAGE DEFAULT and the mode `value` is timed in: every operator in the reference's evaluation order (library expf / IEEE sqrt / exactly "
                                 "rounded mean); bit-identical to oracle/cvx_oracle.c.  Against the captures of the reference itself: convex stage bit-identical, 0 at one "
                                 "iteration, < 1e-3 at 20 / 40; at 80 iterations 1-3e-3 voxel, the distance the reference has from a 1-ulp-perturbed copy of itself "
                                 "(reference_self_perturbation_epe) -- the literal 1e-3 at 80 iterations is met by reference_bits_mode only")
    # the opt-in fast Adam mode: its own speed (same clock as the timed loop: wall time over 10 pairs after 2 warm-up calls)
    for _ in range(2):
        register_pair_device(fix, mov, **FAST)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(10):
        fast_field = register_pair_device(fix, mov, **FAST)
    torch.cuda.synchronize(dev)
    out["fast_mode"]["ms_per_pair"] = (time.perf_counter() - t0) / 10 * 1e3
    out["fast_mode"]["pairs_per_s"] = 1e3 / out["fast_mode"]["ms_per_pair"]
    if oracle_fast_field is not None:
        gotf = np.moveaxis(fast_field.cpu().numpy(), 0, -1).astype(np.float64)
        out["fast_mode"]["bit_identical_to_oracle_fast_restatement"] = bool(np.array_equal(gotf, oracle_fast_field))
        out["fast_mode"]["epe_vs_oracle_fast_restatement"] = float(np.sqrt(((gotf - oracle_fast_field) ** 2).sum(-1)).mean())
    # adam_mode "fast_all" (forward boxes separable too): faster, further from the reference on every capture at 20 iterations -- reported, never `value`
    fa = {}
    for n in (20, 40, 80):
        fa["epe_vs_reference_%dit" % n] = epe_vs_reference(register_pair_device(fix, mov, **dict(CFG, adam_mode="fast_all", selected_niter=n)).cpu().numpy(), n)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(5):
        register_pair_device(fix, mov, **dict(CFG, adam_mode="fast_all"))
    torch.cuda.synchronize(dev)
    fa["ms_per_pair"] = (time.perf_counter() - t0) / 5 * 1e3
    fa["pairs_per_s"] = 1e3 / fa["ms_per_pair"]
    fa["accepted"] = False
    fa["note"] = ("opt-in adam_mode='fast_all': adam_mode='fast' with the FORWARD boxes in separable arithmetic as well "
                  "(the regulariser differentiates U twice: a 1-2 ulp difference in U moves the trajectory), offered for callers that grade by overlap scores")
    out["fast_all_mode"] = fa
    t = out["fast_mode"]
    t["name"] = "adam_mode=fast (opt-in: FMA / factored warp gradient, separable adjoint boxes; forward boxes, regulariser gradient, Adam update and everything before the loop in the reference's order)"
    t["tolerance_met_80it"] = bool(t["epe_vs_reference_80it"] < TOLERANCE_EPE)
    t["captures"] = caps
    r_self = [caps[c]["ratio_to_self_perturbation_80it"] for c in CAPTURES]
    r_exact = [caps[c]["ratio_to_exact_mode_80it"] for c in CAPTURES]
    t["worst_ratio_to_self_perturbation_80it"] = max(r_self)
    t["worst_ratio_to_exact_mode_80it"] = max(r_exact)
    t["mean_epe_80it"] = dict(fast_mode=float(np.mean([caps[c]["epe_vs_reference_80it"] for c in CAPTURES])),
                              exact_mode=float(np.mean([caps[c]["exact_mode_epe_vs_reference_80it"] for c in CAPTURES])),
                              reference_self_perturbation=float(np.mean([caps[c]["reference_self_perturbation_epe"]["80it"] for c in CAPTURES])))
    t["criteria_round3_all_captures_met"] = bool(all(all(caps[c]["criteria_round3"].values()) for c in CAPTURES))
    t["note"] = ("four full-size captures of the reference (c1 = this benchmark pair, c4 another seed / 6-voxel warp, c5 exact-zero background, c6 18-label maps "
                 "through the nnUNet path).  Convex stage bit-identical, 0 at one iteration and < 1e-3 at 20 / 40 iterations on all four.  At 80 iterations every "
                 "arithmetic -- the reference after a 1-ulp perturbation of its own warped features, the exact-order restatement, this mode -- is 1-3e-3 voxel from the "
                 "reference; the two 80-iteration criteria registered in round 3 on ONE pair (<= the self-perturbation distance, <= 1.15 x the exact mode's) are NOT met "
                 "on all captures (criteria_round3 per capture; the exact mode itself misses the first on c4), so adam_mode='fast' is opt-in and 'exact' the package default")
    out["timed_mode"] = dict(out["exact_mode"], name=TIMED_MODE_NAME)
    return out


def api_path(fix, mov, dev, engine_ms):
    """The drop-in call a user of the reference makes: convex_adam_pt(host array, host array) -> host (H,W,D,3) float64,
    including both uploads, the registration, the device-side packing kernel and the transfer of the 165 MB result -- never part of `value`."""
    import numpy as np
    from convexadam_amd.convex_adam_MIND import convex_adam_pt, convex_adam_pt_many, register_pair_device
    fh, mh = fix.cpu(), mov.cpu()                                   # pageable host tensors, as a caller would hold them
    kw = dict(CFG)                                                  # the package default mode (exact), as a caller who passes nothing gets
    # raw PCIe rates of this box (pinned, 165 MB / 27.5 MB)
    big = torch.empty(SHAPE + (3,), dtype=torch.float64, device=dev)
    pin = torch.empty(SHAPE + (3,), dtype=torch.float64, pin_memory=True)
    pin.copy_(big); torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(3):
        pin.copy_(big, non_blocking=True)
    torch.cuda.synchronize(dev)
    d2h = 3 * big.numel() * 8 / (time.perf_counter() - t0) / 1e9
    t0 = time.perf_counter()
    for _ in range(3):
        big.copy_(pin, non_blocking=True)
    torch.cuda.synchronize(dev)
    h2d = 3 * big.numel() * 8 / (time.perf_counter() - t0) / 1e9
    del big, pin
    out = None
    for _ in range(3):
        out = convex_adam_pt(fh, mh, device=dev, **kw)
    calls = []
    for _ in range(12):
        t0 = time.perf_counter()
        out = convex_adam_pt(fh, mh, device=dev, **kw)
        calls.append((time.perf_counter() - t0) * 1e3)
    seq_ms = float(np.median(calls))
    # the same result through the round-3 path: permute + dtype on the device, pageable download, numpy astype on the host
    t0 = time.perf_counter()
    disp = register_pair_device(fix, mov, **kw)
    old = disp.permute(1, 2, 3, 0).to(torch.float16).cpu().numpy().astype(float)
    old_ms = (time.perf_counter() - t0) * 1e3 + 0.0
    same = bool(np.array_equal(old, out))
    del old
    m = 24
    list(convex_adam_pt_many([(fh, mh)] * 4, device=dev, **kw))          # (pinned result buffers and staging slots exist after this)
    t0 = time.perf_counter()
    last, stamps = None, [t0]
    for last in convex_adam_pt_many([(fh, mh)] * m, device=dev, **kw):
        stamps.append(time.perf_counter())
    many_ms = (time.perf_counter() - t0) / m * 1e3
    gaps = sorted((b - a_) * 1e3 for a_, b in zip(stamps[1:], stamps[2:]))      # between results, the pipeline's fill (first result) left out
    steady_ms = gaps[len(gaps) // 2]
    same = same and bool(np.array_equal(last, out))
    nbytes_out = out.nbytes
    bound = engine_ms + (nbytes_out / (d2h * 1e9) + 2 * fix.numel() * 4 / (h2d * 1e9)) * 1e3
    return dict(ms_per_pair=seq_ms, ms_per_pair_mean=float(np.mean(calls)), ms_per_pair_max=float(np.max(calls)), pairs_per_s=1e3 / seq_ms, ms_per_pair_overlapped=many_ms, pairs_per_s_overlapped=1e3 / many_ms, ms_per_pair_overlapped_steady=steady_ms, overlapped_pairs=m,
                ms_per_pair_round3_path=old_ms, pcie_GBps=dict(d2h_pinned=d2h, h2d_pinned=h2d),
                engine_plus_transfers_ms=bound, within_10pct_of_bound=bool(seq_ms <= 1.1 * bound), field_identical_to_round3_path=same,
                output_bytes=nbytes_out,
                note="convex_adam_pt(host, host) -> host (H,W,D,3) float64 with dtype=float16 (the reference's default) and the default Adam mode (exact): torch "
                     "uploads, cvx_register_pair_f32, cvx_pack_field_f64 writing straight into pooled pinned host memory; ms_per_pair = median of 12 calls; 'overlapped' = "
                     "convex_adam_pt_many (pair i+1 uploaded from pinned staging on its own stream while pair i registers; the field of pair i packed into a device "
                     "buffer and moved by a copy engine on a side stream; 24 pairs including the pipeline's fill -- the first result arrives after upload + registration + download = ~12 ms -- "
                     "ms_per_pair_overlapped_steady = median time between consecutive results); bound = engine time + "
                     "165 MB / measured D2H rate + 2 x 27.5 MB / measured H2D rate")


def dump_outputs(d, field):
    """--dump-outputs DIR: what the timed path returned to its caller in its last step, the (3,H,W,D) float32 displacement field, as
    DIR/displacement_sample.npy  float32 (3, DUMP_SAMPLE): the field at voxels drawn once with seed DUMP_SEED, ascending flat index;
    DIR/displacement_moments.npy float64 (3, 2): sum and sum of squares of each component over the WHOLE field."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    flat = field.reshape(3, -1)
    idx = np.sort(np.random.default_rng(DUMP_SEED).choice(flat.shape[1], size=min(DUMP_SAMPLE, flat.shape[1]), replace=False))
    np.save(os.path.join(d, "displacement_sample.npy"), np.ascontiguousarray(flat[:, idx], dtype=np.float32))
    f64 = flat.astype(np.float64)
    np.save(os.path.join(d, "displacement_moments.npy"), np.stack([f64.sum(1), (f64 * f64).sum(1)], 1))


LINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
             "mode", "config", "roofline", "stages_ms", "cpu_baseline", "tolerance_met", "value_exact_mode", "value_fast_mode", "value_at_tolerance",
             "value_zero_background")
PARITY_LINE_KEYS = ("bit_identical", "epe_vs_oracle", "max_abs_diff", "tolerance_epe")
LINE_MAX_BYTES = 8192


def bench_line(res, extra_path=None):
    """The printed result line: the contract keys of the full record `res`, its parity verdict and one {ms_per_pair, corr_frac} per
    secondary config.  The whole record (every secondary figure) goes to the side file (--extra-out); a line of 24.6 KB did not parse."""
    line = {k: res[k] for k in LINE_KEYS if k in res}
    if "parity" in res:
        line["parity"] = {k: res["parity"][k] for k in PARITY_LINE_KEYS if k in res["parity"]}
    if "configs" in res:
        line["configs"] = {name: {"ms_per_pair": c.get("ms_per_pair"), "corr_frac": (c.get("roofline_correlate") or {}).get("frac")}
                           for name, c in res["configs"].items() if "ms_per_pair" in c}
        if "configs[4]" in res["configs"]:
            line["configs"]["configs[4]"] = {"items_per_s": res["configs"]["configs[4]"].get("items_per_s")}
    line["extra"] = os.path.basename(extra_path) if extra_path else None
    return line


def host_cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def effective_cores():
    """Host cores this process may actually use: the affinity mask capped by the cgroup CPU quota (the round-4 GPU boxes show 256 CPUs
    with cpu.max = 16 cores; 128 OpenMP threads on 16 cores' worth of quota only add throttling stalls)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.999)))
    except Exception:
        pass
    return n


def cpu_baseline(fix, mov, hip_field):
    """Times the C oracle (oracle/, the parity checker) on the host cores for one full pair and -- outside every timed region --
    compares the field the timed HIP loop produced for the same pair with the oracle's field."""
    import numpy as np
    from oracle import oracle
    oracle.build()
    visible = oracle.num_threads()
    cores = min(visible, effective_cores())
    oracle.set_num_threads(cores)
    t0 = time.time()
    ref, st = oracle.convex_adam_pipeline(fix, mov, return_stages=True, **CFG)            # (H,W,D,3) float64; the reference-order restatement is what is timed
    dt = time.time() - t0
    got = np.moveaxis(hip_field, 0, -1).astype(np.float64)
    epe = float(np.sqrt(((got - ref) ** 2).sum(-1)).mean())
    parity = dict(epe_vs_oracle=epe, bit_identical=bool(np.array_equal(got, ref)), max_abs_diff=float(np.abs(got - ref).max()),
                  note="field of the last timed step vs the field of oracle/cvx_oracle.c's whole pipeline (the run timed as cpu_baseline) on the same pair, "
                       "full size: the timed mode is the reference-order mode, so the two must be equal bit for bit; the modes against the reference itself: "
                       "timed_mode (= exact_mode) / fast_mode / reference_bits_mode below")
    # the opt-in fast Adam mode restated on the CPU (outside the baseline's clock), for parity.fast_mode: same loop in the fast arithmetic, from the stages above
    r = oracle.adam_run(st["F2"], st["M2"], st["P0"], CFG["lambda_weight"], CFG["selected_niter"], mode="fast", keep_last_step=False)
    parity["_oracle_fast_field"] = np.moveaxis(oracle.resize_trilinear(r["U"] * np.float32(CFG["grid_sp_adam"]), fix.shape), 0, -1).astype(np.float64)
    base = dict(value=1.0 / dt, unit="pairs/s", cores=cores, kind="port", seconds_per_pair=dt, host_cpu=host_cpu_model(),
                sample="1 full 160x192x224 pair (MIND r1 d2, gs6, hw6, ic, 80 Adam its) with oracle/cvx_oracle.c, "
                       "OpenMP over %d threads (= the cores this container may use: %d CPUs visible, capped by the cgroup CPU quota); "
                       "reference PyTorch-CPU figure from BASELINE.md: 77.4 s/pair on 8 cores" % (cores, visible))
    return base, parity


def secondary_configs(dev):
    """BASELINE configs[2..4] timed on this GPU next to the headline (rank 0 / N = 1, outside the timed region of `value`; the parity of each
    is tests/test_gpu_parity.py's job: test_full_size_masked_large_motion_config3, test_nnunet_*, test_two_stage_sweep_*): wall clock over
    whole registrations from device-resident inputs, hipEvent stage intervals, and the HBM roofline fraction of the correlation stage
    (algorithmic bytes = (2 hw + 1)^3 v 4 written + 2 C v 4 read per direction, as the graded `roofline`)."""
    import tempfile
    from convexadam_amd import phantom as ph
    from convexadam_amd.convex_adam_MIND import extract_features, last_profile, register_pair_device, set_profiling
    from convexadam_amd.convex_adam_nnUNet import extract_features as nn_features

    def timed(reg, reps):
        for _ in range(2):
            reg()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            reg()
        torch.cuda.synchronize(dev)
        wall = (time.perf_counter() - t0) / reps * 1e3
        set_profiling(2)
        for _ in range(3):
            reg()
        torch.cuda.synchronize(dev)
        st = {}
        for name, ms in last_profile():
            st.setdefault(name, []).append(ms)
        set_profiling(0)
        return wall, {k: sum(v) / len(v) for k, v in st.items()}

    def corr_roofline(st, C, grid, hw):
        v = grid[0] * grid[1] * grid[2]
        alg = (2 * hw + 1) ** 3 * v * 4 + 2 * C * v * 4
        c = [st[k] for k in ("correlate", "correlate_rev") if st.get(k)]
        if not c:
            return None
        ms = sum(c) / len(c)
        return {"algorithmic_bytes": alg, "avg_launch_ms": ms, "achieved": alg / (ms * 1e-3) / 1e9, "unit": "GB/s", "frac": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}

    res = {}
    # configs[2]: 224x192x224 with masks, disp_hw 8 (4913 displacements), grid_sp 6, 80 Adam iterations
    shape = (224, 192, 224)
    fix, mov = ph.deformed_pair(shape, 3, 10.0)
    mf, mm = ph.ellipsoid_mask(shape, 0.35), ph.ellipsoid_mask(shape, 0.35, shift=(4, -3, 5))
    fix, mov, mf, mm = (t.to(dev).contiguous() for t in (fix, mov, mf, mm))
    kw = dict(lambda_weight=1.25, grid_sp=6, disp_hw=8, selected_niter=80, selected_smooth=0, grid_sp_adam=2, ic=True)
    feats = {}

    def reg3(mode="exact"):
        ff, fm = extract_features(fix, mov, 1, 2, True, mf, mm, device=dev, dtype=torch.float32)
        feats["out"] = register_pair_device(feat_fixed=ff[0], feat_moving=fm[0], adam_mode=mode, **kw)

    wall, st = timed(reg3, 5)
    exact_field = feats["out"].clone()
    wall_f, _ = timed(lambda: reg3("fast"), 5)
    epe_fast = float((feats["out"] - exact_field).square().sum(0).sqrt().mean())
    res["configs[2]"] = {"workload": "224x192x224 pair with ellipsoid masks (replicate-fill), MIND-SSC r1 d2, grid_sp 6, disp_hw 8 (17^3 = 4913 displacements), ic, lambda 1.25, "
                                     "grid_sp_adam 2, 80 Adam iterations, float32, package default mode",
                         "ms_per_pair": wall, "pairs_per_s": 1e3 / wall, "stages_ms": st, "roofline_correlate": corr_roofline(st, 12, tuple(x // 6 for x in shape), 8),
                         "fast_adam_mode": {"ms_per_pair": wall_f, "pairs_per_s": 1e3 / wall_f, "epe_vs_exact_mode_field": epe_fast},
                         "note": "ms_per_pair = wall clock of masked feature extraction (fill + MIND-SSC, its own launches) + cvx_register_pair_f32 on the features; stages_ms covers the "
                                 "latter only.  The fast Adam mode's field against the default mode's on this pair: 10-voxel warps leave large regions where the warped features are "
                                 "flat (outside the masks), where the trajectories of the two arithmetics separate faster than on configs[1]"}
    del fix, mov, mf, mm, exact_field, feats
    torch.cuda.empty_cache()
    # configs[3]: 32-channel one-hot nnUNet features (convex_adam_nnUNet path), 160x192x160
    shape = (160, 192, 160)
    lab, labm = ph.warped_label_pair(shape, 32, 11, 0.05)
    kw = dict(lambda_weight=1.25, grid_sp=4, disp_hw=4, selected_niter=80, selected_smooth=0, grid_sp_adam=2, ic=True)
    ff, fm = nn_features(lab, labm, device=dev)
    C = int(ff.shape[1])
    wall_feat, _ = timed(lambda: nn_features(lab, labm, device=dev), 3)
    wall, st = timed(lambda: register_pair_device(feat_fixed=ff[0], feat_moving=fm[0], **kw), 5)
    res["configs[3]"] = {"workload": "160x192x160 label maps with %d classes -> %d-channel one-hot features (convex_adam_nnUNet), grid_sp 4, disp_hw 4 (729 displacements), ic, lambda 1.25, "
                                     "grid_sp_adam 2, 80 Adam iterations, float32, package default mode" % (C, C),
                         "ms_per_pair": wall, "pairs_per_s": 1e3 / wall, "feature_extraction_ms": wall_feat, "stages_ms": st,
                         "roofline_correlate": corr_roofline(st, C, tuple(x // 4 for x in shape), 4),
                         "note": "registration from device-resident feature volumes (ms_per_pair); feature_extraction_ms = one-hot + pooling from host label maps, upload included"}
    del ff, fm
    torch.cuda.empty_cache()
    # configs[4]: the self-configuring sweep, a slice of it on one GPU: 16 convex-stage settings x 2 pairs, then 12 Adam-stage settings x 2 pairs, scored on the device
    from convexadam_amd import sweep
    with tempfile.TemporaryDirectory() as td:
        outp = os.path.join(td, "sweep.json")
        argv = ["--pairs", "2", "--shape", "160", "192", "224", "--stage1", "16", "--stage2", "12", "--out", outp, "--adam-mode", "exact"]
        import contextlib
        import io
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):                     # (the sweep prints its own summary line; this script prints exactly one)
            rc = sweep.main(argv)
        dt = time.perf_counter() - t0
        with open(outp) as f:
            j = json.load(f)
    n_items = j["stage1"]["n_items"] + j["stage2"]["n_items"]
    res["configs[4]"] = {"workload": "two-stage hyper-parameter sweep slice on one GPU: 16 convex-stage settings x 2 pairs + 12 Adam-stage settings x 2 pairs at 160x192x224 "
                                     "(each Adam-stage item = MIND + 80-iteration loop with snapshots + 5 smoothers x 3 snapshots scored), label maps scored on the device "
                                     "(Dice / HD95 / SDlogJ), exact Adam mode, %d worker threads" % j.get("workers_per_rank", 0),
                         "items": n_items, "evaluations": j["stage2"].get("evaluations"), "seconds": j["wall_s"], "items_per_s": j["items_per_s"], "seconds_including_data_generation": dt,
                         "return_code": rc, "phases": j.get("phases"),
                         "note": "seconds = the sweep's own clock around both phases (pairs, label maps generated before it); the 8-GPU sweep shards the items over ranks "
                                 "through a shared queue (tests/test_sweep_dist.py, gloo)"}
    return res


def parse_args(argv=None):
    """The command line -> namespace, with what --full decides already applied: without it both halves of the secondary work are off
    (no_cpu_baseline, no_batched) and no side file is written."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true", help="after the timed steps, also run everything else this script measures or checks: the CPU baseline "
                    "and the parity verdicts, the other modes, precisions and configs, batched pairs, the per-kernel figures (minutes instead of seconds; "
                    "never part of `value`).  Without it the run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle, the parity block and the drop-in API timing")
    ap.add_argument("--no-batched", action="store_true", help="with --full: skip the secondary measurements (batched pairs, other configs, modes)")
    ap.add_argument("--adam-mode", default="exact", choices=("exact", "fast"), help="mode of the timed loop: exact = the package default (what `value` "
                    "means); fast = the opt-in throughput arithmetic of the Adam loop (profiling runs; the line then says so in `mode`)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write the field of the last timed step as .npy files under DIR "
                    "(a seeded sample of it and its whole-field moments; see dump_outputs)")
    ap.add_argument("--extra-out", default=None, metavar="FILE",
                    help="where the whole result record goes (every secondary figure; the printed line carries the contract keys); '' = nowhere.  "
                         "Default: bench_extra.json next to this script with --full, nowhere without (a plain run has no secondary figure to keep)")
    a = ap.parse_args(argv)
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not a.full:              # a plain run measures `value` and what the timed steps themselves record (stages_ms, roofline); nothing runs after them
        a.no_cpu_baseline = a.no_batched = True
    if a.extra_out is None:
        a.extra_out = os.path.join(ROOT, "bench_extra.json") if a.full else ""
    return a


def main():
    a = parse_args()
    global TIMED, TIMED_MODE_NAME
    if a.adam_mode == "fast":
        TIMED, TIMED_MODE_NAME = FAST, "adam_mode=fast (OPT-IN, not the package default; run with --adam-mode fast)"

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    # test hooks (tests/test_gpu_parity.py runs the N > 1 path on a one-GPU box): BENCH_SHARE_DEVICE=1 puts every rank on device 0,
    # BENCH_DIST_BACKEND=gloo replaces RCCL, which refuses two ranks on one device; the driver's runs set neither
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    if os.environ.get("BENCH_SHARE_DEVICE") == "1":
        local = 0
    # host threads: the boxes show 256 CPUs behind a 16-core quota; torch's default pool (one thread per visible CPU, per rank) only adds
    # throttling stalls to the synthetic-input generation and the staging copies (nothing inside the timed region runs on the host pool)
    torch.set_num_threads(max(1, min(torch.get_num_threads(), effective_cores() // max(1, world))))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    red_dev = dev if backend == "nccl" else torch.device("cpu")          # where the max-over-ranks reduction of the clock lives
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend=backend, rank=rank, world_size=world)

    from convexadam_amd.convex_adam_MIND import last_profile, register_pair_device, register_pairs_device, set_profiling

    fix, mov = make_pair(dev, rank)
    out = torch.empty((3,) + SHAPE, dtype=torch.float32, device=dev)

    for _ in range(a.warmup):
        register_pair_device(fix, mov, out=out, **TIMED)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
        torch.cuda.synchronize(dev)
    stage_ms = {}
    set_profiling(2)            # stage boundaries = hipEventRecord on the launch stream, read back after the timed region
    t0 = time.perf_counter()
    for _ in range(a.steps):
        register_pair_device(fix, mov, out=out, **TIMED)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
        torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    field_of_timed_loop = out.cpu().numpy() if rank == 0 else None      # read back after the timed region
    for name, ms in last_profile():
        stage_ms.setdefault(name, []).append(ms)
    set_profiling(0)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, field_of_timed_loop)
    # per-kernel durations of the Adam loop (outside the timed region): cvx_set_profiling(3) records one event behind every kernel of the loop
    kernel_ms = {}
    if rank == 0 and not a.no_batched:          # (the rocprofv3 passes of tools/profile_round.sh run with --no-batched: one pair per PMC pass)
        set_profiling(3)
        for _ in range(3):
            register_pair_device(fix, mov, out=out, **TIMED)
        torch.cuda.synchronize(dev)
        for name, ms in last_profile():
            if name.startswith("adam."):
                kernel_ms.setdefault(name, []).append(ms)
        set_profiling(0)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # secondary figures (not `value`): the batch entry point deals independent pairs onto n internal HIP streams (pairs in flight together on one GPU)
    batched = None
    if not a.no_batched:
        batched = {}
        for mode_name, kw in (("exact", TIMED), ("fast", FAST)):
            for ns in (2, 3, 4):
                outs = [out] + [torch.empty_like(out) for _ in range(ns - 1)]
                register_pairs_device([fix] * ns, [mov] * ns, outs=outs, n_streams=ns, **kw)
                torch.cuda.synchronize(dev)
                if world > 1:
                    dist.barrier()
                tb = time.perf_counter()
                for _ in range(a.steps):
                    register_pairs_device([fix] * ns, [mov] * ns, outs=outs, n_streams=ns, **kw)
                torch.cuda.synchronize(dev)
                if world > 1:
                    dist.barrier()
                eb = time.perf_counter() - tb
                if world > 1:
                    t = torch.tensor([eb], dtype=torch.float64, device=red_dev)
                    dist.all_reduce(t, op=dist.ReduceOp.MAX)
                    eb = float(t.item())
                batched["%s_%dstreams" % (mode_name, ns)] = {"pairs_per_call": ns, "n_streams": ns, "value": world * a.steps * ns / eb, "unit": "pairs/s",
                                                            "ms_per_call": eb / a.steps * 1e3}
                del outs
        batched["note"] = ("cvx_register_pairs_f32: n independent pairs per call per GPU, each on its own internal HIP stream and workspace; the kernels of different pairs "
                           "overlap where one pair's launch leaves CUs idle (tail rounds of the Adam-loop kernels, the short convex-stage kernels)")
        register_pair_device(fix, mov, out=out, **TIMED)          # `out` holds the timed mode's field again (compared below)
        torch.cuda.synchronize(dev)

    # data-dependent stage, reported for both ends (not part of `value`): the branch-and-bound coupled-convex passes visit about one
    # candidate per voxel on the textured phantom; on a volume with exact-zero background every background voxel keeps its whole
    # search window and the passes fall back to coalesced scans of the cost volume (bounded worst case)
    cc_worst = None
    corr_exact_ms = pair_exact_ms = corr_exact_same = None
    if rank == 0 and not a.no_batched:
        from convexadam_amd.phantom import ellipsoid_mask
        m = ellipsoid_mask(SHAPE, 0.3).to(dev)
        fz, mz = (fix * m).contiguous(), (mov * m).contiguous()
        set_profiling(0)
        for _ in range(2):
            register_pair_device(fz, mz, **TIMED)
        torch.cuda.synchronize(dev)
        set_profiling(2)
        for _ in range(3):
            register_pair_device(fz, mz, **TIMED)
        torch.cuda.synchronize(dev)
        st = {}
        for name, ms in last_profile():
            st.setdefault(name, []).append(ms)
        set_profiling(0)
        cc_worst = {k: sum(v) / len(v) for k, v in st.items() if k in ("coupled_convex", "argmin", "correlate")}
        cc_worst["ms_per_pair"] = sum(sum(v) / len(v) for v in st.values())
        # opt-in fast correlation mode (FMA + separable sums; same indices and a bit-identical field on this pair, but no proof: not the default)
        for _ in range(2):
            register_pair_device(fix, mov, corr_mode="fast", **TIMED)
        torch.cuda.synchronize(dev)
        set_profiling(2)
        for _ in range(3):
            fast_field = register_pair_device(fix, mov, corr_mode="fast", **TIMED)
        torch.cuda.synchronize(dev)
        st = {}
        for name, ms in last_profile():
            st.setdefault(name, []).append(ms)
        set_profiling(0)
        fc = st.get("correlate", []) + st.get("correlate_rev", [])
        cc_worst["fast_corr_ms"] = sum(fc) / max(len(fc), 1) / (1 if "correlate_rev" in st else 2)      # per direction
        cc_worst["fast_field_identical"] = bool(torch.equal(fast_field, out))
        # the exact-order correlation kernel (option corr_cert = 0, the round-5 default): same field, its own stage time
        from convexadam_amd import _lib
        L = _lib.lib()
        old_cert = L.cvx_get_option(b"corr_cert")
        L.cvx_set_option(b"corr_cert", 0)
        try:
            for _ in range(2):
                register_pair_device(fix, mov, **TIMED)
            torch.cuda.synchronize(dev)
            set_profiling(2)
            for _ in range(3):
                ex_field = register_pair_device(fix, mov, **TIMED)
            torch.cuda.synchronize(dev)
            st = {}
            for name, ms in last_profile():
                st.setdefault(name, []).append(ms)
            set_profiling(0)
        finally:
            L.cvx_set_option(b"corr_cert", old_cert)
        ec = st.get("correlate", []) + st.get("correlate_rev", [])
        corr_exact_ms = sum(ec) / max(len(ec), 1) / (1 if "correlate_rev" in st else 2)
        pair_exact_ms = sum(sum(v_) / len(v_) for v_ in st.values())
        corr_exact_same = bool(torch.equal(ex_field, out))
        # fp16 STORAGE (the reference's GPU default dtype): both cost volumes and the Adam loop's feature records are __half
        for _ in range(2):
            register_pair_device(fix, mov, storage="fp16", **TIMED)
        torch.cuda.synchronize(dev)
        set_profiling(2)
        t16 = time.perf_counter()
        for _ in range(5):
            h16_field = register_pair_device(fix, mov, storage="fp16", **TIMED)
        torch.cuda.synchronize(dev)
        t16 = (time.perf_counter() - t16) / 5
        st = {}
        for name, ms in last_profile():
            st.setdefault(name, []).append(ms)
        set_profiling(0)
        hc = st.get("correlate", []) + st.get("correlate_rev", [])
        if "correlate_rev" not in st:
            hc = [t_ / 2 for t_ in hc]                              # per direction
        conv32 = register_pair_device(fix, mov, **dict(CFG, lambda_weight=0))
        conv16 = register_pair_device(fix, mov, storage="fp16", **dict(CFG, lambda_weight=0))
        out32 = out                                               # the float32 field of the timed mode (fp16 storage runs the same Adam arithmetic since round 5)
        t16_stages = sum(sum(v_) / len(v_) for v_ in st.values()) * 1e-3      # hipEvent stage intervals (as zero_background above): a host hiccup in a 5-pair wall clock was 1 ms per pair in one run
        cc_worst["fp16"] = dict(ms_per_pair=(t16_stages if st else t16) * 1e3, ms_per_pair_wall=t16 * 1e3, corr_ms=sum(hc) / max(len(hc), 1), adam_ms=sum(st.get("adam", [0.0])) / max(len(st.get("adam", [0.0])), 1),
                                argmin_ms=sum(st.get("argmin", [0.0])) / max(len(st.get("argmin", [0.0])), 1),
                                epe_vs_fp32_field=float((h16_field - out32).square().sum(0).sqrt().mean()),
                                convex_stage_voxels_changed=float((conv16 != conv32).any(0).float().mean()),
                                convex_stage_epe=float((conv16 - conv32).square().sum(0).sqrt().mean()))

    # the descriptor stage in ONE stencil pass (option mind_single, off by default because it is slower): both forms timed on the same images through
    # the pooled-descriptor operator (cvx_mindssc_pooled_f32), the repair-list length on the phantom and on the zero-background pair
    mind_single = None
    if rank == 0 and not a.no_batched:
        from convexadam_amd import _lib
        from convexadam_amd.convex_adam_utils import mind_pooled
        from convexadam_amd.phantom import ellipsoid_mask
        L = _lib.lib()
        old_single = L.cvx_get_option(b"mind_single")
        mind_single = {}
        try:
            mz_ = ellipsoid_mask(SHAPE, 0.3).to(dev)
            imgs = {"phantom": (fix, mov), "zero_background": ((fix * mz_).contiguous(), (mov * mz_).contiguous())}
            for tag, pair in imgs.items():
                row = {}
                for name, val in (("two_pass", 0), ("single_pass", 1)):
                    L.cvx_set_option(b"mind_single", val)
                    outs, reps = [], 0
                    for im in pair:
                        r_ = mind_pooled(im[None, None], CFG["mind_r"], CFG["mind_d"], CFG["grid_sp"], CFG["grid_sp_adam"], device=dev, return_repairs=True)
                        outs.append(r_[:2]); reps += r_[2]
                    torch.cuda.synchronize(dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(5):
                        for im in pair:
                            mind_pooled(im[None, None], CFG["mind_r"], CFG["mind_d"], CFG["grid_sp"], CFG["grid_sp_adam"], device=dev)
                    e1.record(); torch.cuda.synchronize(dev)
                    row[name] = {"ms_both_images": e0.elapsed_time(e1) / 5, "blocks_repaired": reps}
                    row["_" + name] = outs
                row["bit_identical"] = all(bool(torch.equal(x_, y_)) for p_, q_ in zip(row.pop("_two_pass"), row.pop("_single_pass")) for x_, y_ in zip(p_, q_))
                mind_single[tag] = row
        finally:
            L.cvx_set_option(b"mind_single", old_single)
        nblk = -(-SHAPE[0] // CFG["grid_sp"]) * -(-SHAPE[1] // CFG["grid_sp"]) * -(-SHAPE[2] // CFG["grid_sp"])
        mind_single["blocks_per_image"] = nblk
        for key in ("mind_two_pass_bytes_per_image", "mind_single_pass_bytes_per_image"):
            if pmc_extra(key) is not None:
                mind_single[key] = pmc_extra(key)
        mind_single["note"] = ("avg_pool3d(MINDSSC(img), 6 | 2) of both images through cvx_mindssc_pooled_f32 (hipEvents, kernels + the 2 tiny statistics launches): two_pass = "
                               "k_mind_march + k_mind_finish_pool through 330 MB of raw patch distances per image (the pipeline's default); single_pass = k_mind_march_pool "
                               "(normalisation with the unclamped variance and both poolings inside the stencil kernel) + k_mind_repair (pooled cells of the blocks where the "
                               "variance clamp binds, recomputed with the global mean); same bits; the single pass moves a fifth of the bytes and is SLOWER: both forms are "
                               "bound by instruction issue (27 additions per patch distance, 12 IEEE divisions + 12 exp per voxel), DESIGN.md 12.11")

    if rank == 0:
        n = world
        h, w, d = (s // CFG["grid_sp"] for s in SHAPE)
        K = (2 * CFG["disp_hw"] + 1) ** 3
        v = h * w * d
        # both directions of the pair go through ONE launch of the fused kernel (option corr_dual, round 5): the stage interval "correlate" then
        # covers 2 x (K v 4 written + 2 C v 4 read) and there is no "correlate_rev" interval
        corr_dual = "correlate_rev" not in stage_ms
        alg_dir = K * v * 4 + 2 * 12 * v * 4
        alg_bytes = (2 if corr_dual else 1) * alg_dir
        corr = stage_ms.get("correlate", []) + stage_ms.get("correlate_rev", [])
        corr_ms = sum(corr) / max(len(corr), 1)
        # since round 6 (second half) the intervals "correlate" / "correlate_rev" are the fused kernel ALONE (an event between the feature copies and the
        # kernel): the dominant kernel's own launch duration, which is what rocprofv3's table shows; the copies (k_corr_prep 7 us; forward direction: + the
        # certification set-up k_cert_arm) are "correlate_prep"
        prep = stage_ms.get("correlate_prep", [])
        prep_ms = sum(prep) / max(len(prep), 1) if prep else 0.0
        achieved = alg_bytes / (corr_ms * 1e-3) / 1e9 if corr_ms > 0 else 0.0
        traffic, traffic_commit, traffic_stale = pmc_traffic()
        res = {
            "metric": "volume-pairs/sec (160x192x224 MIND convex+Adam(80it))",
            "value": n * a.steps / elapsed,
            "unit": "pairs/s",
            "n_gpus": n,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": elapsed / a.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "mode": TIMED_MODE_NAME,
            "config": {"workload": "BASELINE configs[1]: 160x192x224 pair, MIND-SSC r1 d2, grid_sp 6, disp_hw 6, ic, "
                                   "lambda 1.25, grid_sp_adam 2, 80 Adam iterations, float32",
                       "pairs_per_gpu_per_step": 1, "parallelism": "one pair per GPU, no collectives"},
            "roofline": {"kernel": "correlate stage = 2 x k_corr_prep + ONE k_corr_fused launch for both directions of the pair (raw SSD + both boxes in one kernel)" if corr_dual
                                   else "k_corr_fused<5,33>, one direction: the interval between HIP events around the kernel ALONE (the padded feature copies of k_corr_prep are the stage correlate_prep and count in frac_with_feature_copies) (raw SSD + both boxes in one kernel; certified-fast arithmetic: "
                                        "FMA channel sums, separable running box sums, unscaled -- the volume is within 2^-17 of ATen's and every argmin taken on it is certified "
                                        "or re-evaluated exactly by certify.hip, stages argmin / argmin_rev / coupled_convex; option corr_cert = 0 gives the exact-order kernel)",
                         "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_measured_at_commit": traffic_commit,
                         "traffic_stale": traffic_stale, "algorithmic_bytes": alg_bytes, "avg_launch_ms": corr_ms,
                         "stage_ms_with_feature_copies": corr_ms + prep_ms, "frac_with_feature_copies": alg_bytes / ((corr_ms + prep_ms) * 1e-3) / 1e9 / HBM_PEAK_GBS if corr_ms > 0 else 0.0},
            "stages_ms": {k: sum(vs) / len(vs) for k, vs in stage_ms.items()},
        }
        # the same accounting for the other stages and for the pair (every logical tensor touched once per logical pass);
        # the graded `roofline` above stays the correlation kernel, the dominant stage BY TIME is the Adam loop
        sm = res["stages_ms"]
        V, g2 = SHAPE[0] * SHAPE[1] * SHAPE[2], CFG["grid_sp_adam"]
        v2 = (SHAPE[0] // g2) * (SHAPE[1] // g2) * (SHAPE[2] // g2)
        its = CFG["selected_niter"]
        alg = {"mind": 2 * (2 * V * 4 + 12 * v2 * 4 + 12 * v * 4),                        # per image: two reads (global mean), pooled outputs only
               "correlate": alg_bytes, "correlate_rev": alg_dir,
               "adam": its * (2 * 12 * v2 * 4 + 10 * 3 * v2 * 4)}                         # F2 + M2 + p, m, v read+write + U and dU write+read
        by_stage = {}
        for k, bts in alg.items():
            if sm.get(k):
                by_stage[k] = {"algorithmic_bytes": bts, "ms": sm[k], "achieved_GBps": bts / (sm[k] * 1e-3) / 1e9, "frac": bts / (sm[k] * 1e-3) / 1e9 / HBM_PEAK_GBS}
        pair_bytes = alg["mind"] + 2 * (alg_dir + 6 * K * v * 4) + alg["adam"] + 3 * V * 4 * 4
        by_stage["pair"] = {"algorithmic_bytes": pair_bytes, "ms": res["ms_per_step"], "achieved_GBps": pair_bytes / (res["ms_per_step"] * 1e-3) / 1e9,
                            "frac": pair_bytes / (res["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                            "note": "coupled convex counted at 6 full reads of the cost volume per direction (SURVEY 8(d)); the branch-and-bound passes read less"}
        mind_meas = pmc_extra("mind_two_pass_bytes_per_image")
        if mind_meas is not None and "mind" in by_stage:
            by_stage["mind"]["traffic"] = 2 * mind_meas                                 # both images: HBM bytes from the PMC passes (profiles/pmc_hbm_traffic.json)
        res["roofline_by_stage"] = by_stage
        if mind_single is not None:
            res["mind_single_pass"] = mind_single
        # the pair with the coupled-convex stage at its MEASURED bytes (PMC passes of tools/profile_round.sh; the branch-and-bound passes touch ~1 % of
        # the 6 x 270 MB the reference's formulation streams): the figure to quote for "fraction of the HBM roofline of the whole pair"
        cc_meas = pmc_extra("coupled_convex_bytes_per_pair")
        if cc_meas is not None:
            pb = pair_bytes - 2 * 6 * K * v * 4 + cc_meas
            by_stage["pair_measured_coupled_convex"] = {"algorithmic_bytes": pb, "coupled_convex_measured_bytes": cc_meas, "ms": res["ms_per_step"],
                                                        "achieved_GBps": pb / (res["ms_per_step"] * 1e-3) / 1e9, "frac": pb / (res["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                                        "note": "as `pair`, with the coupled-convex stage counted at the HBM bytes its kernels actually move (rocprofv3 FETCH_SIZE / WRITE_SIZE, profiles/pmc_hbm_traffic.json)"}
        if kernel_ms:
            import statistics
            kb = {"adam.forward_boxes": 2 * 3 * v2 * 4,                              # P read, U written
                  "adam.warp_gradient": 2 * 12 * v2 * 4 + 2 * 3 * v2 * 4,            # F2, M2 read (gather: cache-perfect), U read, dU written
                  "adam.adjoint_update": 7 * 3 * v2 * 4}                             # dU read; P, m, v read and written
            rk = {}
            for name, bts in kb.items():
                if kernel_ms.get(name):
                    us = statistics.median(kernel_ms[name]) * 1e3
                    rk[name] = {"algorithmic_bytes": bts, "us": us, "achieved_GBps": bts / (us * 1e-6) / 1e9, "frac": bts / (us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                                "launches_timed": len(kernel_ms[name])}
            rk["iteration"] = {"algorithmic_bytes": sum(kb.values()), "us": sum(r["us"] for r in rk.values()),
                               "note": "median interval between consecutive hipEvents on the launch stream (cvx_set_profiling(3): one event behind every kernel of the "
                                       "loop, 3 pairs x 79 iterations, outside the timed region; an interval = the kernel + its boundary); SURVEY 8(d) bytes: 185.8 MB per iteration"}
            rk["iteration"]["frac"] = rk["iteration"]["algorithmic_bytes"] / (rk["iteration"]["us"] * 1e-6) / 1e9 / HBM_PEAK_GBS
            if "adam.warp_gradient" in rk:
                rk["adam.warp_gradient"]["bound"] = ("L1 miss queue: 2.0 M read requests per launch at 323 clocks mean latency = 55 of 64 in flight per CU "
                                                     "(profiles/r05_adam_loop_memory_counters_fp32.txt, DESIGN.md 11.8)")
            if "adam.forward_boxes" in rk:
                rk["adam.forward_boxes"]["bound"] = "instruction issue: 3 x 27 additions per output in ATen's order (DESIGN.md 11.1)"
            res["roofline_by_kernel"] = rk
        if batched is not None:
            res["batched_2streams"] = dict(batched["exact_2streams"], note=batched["note"])
            res["batched"] = batched
        if cc_worst is not None and cc_worst.get("fast_corr_ms"):
            fa = alg_dir / (cc_worst["fast_corr_ms"] * 1e-3) / 1e9
            res["roofline_fast_mode"] = {"kernel": "k_corr_prep + k_corr_fused<5,1> (corr_mode='fast': FMA, separable box sums; opt-in)", "achieved": fa,
                                         "unit": "GB/s", "frac": fa / HBM_PEAK_GBS, "avg_launch_ms": cc_worst["fast_corr_ms"],
                                         "final_field_bit_identical_to_exact_mode": cc_worst["fast_field_identical"]}
        if cc_worst is not None and cc_worst.get("fp16"):
            h = cc_worst["fp16"]
            hb = K * v * 2 + 2 * 12 * v * 4
            ha = hb / (h["corr_ms"] * 1e-3) / 1e9
            res["fp16_storage_mode"] = {"ms_per_pair": h["ms_per_pair"], "pairs_per_s": 1e3 / h["ms_per_pair"], "ms_per_pair_wall": h.get("ms_per_pair_wall"),
                                        "roofline": {"kernel": "k_corr_prep + k_corr_fused<5,24> (cost volume written as __half)", "algorithmic_bytes": hb,
                                                     "avg_launch_ms": h["corr_ms"], "achieved": ha, "unit": "GB/s", "frac": ha / HBM_PEAK_GBS},
                                        "stages_ms": {"correlate": h["corr_ms"], "argmin": h["argmin_ms"], "adam": h["adam_ms"]},
                                        "epe_vs_fp32_field": h["epe_vs_fp32_field"], "convex_stage_voxels_changed": h["convex_stage_voxels_changed"],
                                        "convex_stage_epe": h["convex_stage_epe"],
                                        "note": "opt-in storage='fp16' (the reference's GPU default dtype, convex_adam_MIND.py:79) with the timed mode's Adam arithmetic: cost volumes and the Adam loop's "
                                                "feature records are real __half buffers (the warp kernel gathers 8-byte records), float32 accumulation; bit-identical to the oracle's fp16 restatement, graded "
                                                "against the float32 field by end-point error and by the fraction of convex-stage voxels whose displacement changed"}
        if cc_worst is not None and cc_worst.get("ms_per_pair"):
            res["value_zero_background"] = 1e3 / cc_worst["ms_per_pair"]          # the timed mode on the same pair with an exact-zero background (skull-stripped-like)
        if cc_worst is not None:
            res["coupled_convex_ms"] = {"phantom": res["stages_ms"].get("coupled_convex"), "zero_background": cc_worst.get("coupled_convex"),
                                        "zero_background_ms_per_pair": cc_worst.get("ms_per_pair"),
                                        "note": "both directions; zero_background = same pair multiplied by an ellipsoid mask (exact zeros outside): flat cost "
                                                "regions, every in-volume displacement of a background voxel ties at 0; the pruning bound then comes from the displacement nearest to the smoothed "
                                                "field (option prune_refine; 0.41 ms without it), and a pass whose large candidate boxes still exceed the cost of a coalesced scan streams the volume instead (bounded worst case)"}
        if corr_exact_ms:
            ea = alg_dir / (corr_exact_ms * 1e-3) / 1e9
            res["roofline_exact_order_kernel"] = {"kernel": "k_corr_prep + k_corr_fused<5,0> (option corr_cert = 0: ATen's evaluation order inside the kernel, the round-5 default)",
                                                  "achieved": ea, "unit": "GB/s", "frac": ea / HBM_PEAK_GBS, "avg_launch_ms": corr_exact_ms, "ms_per_pair": pair_exact_ms,
                                                  "field_identical_to_certified_path": corr_exact_same}
        if n == 1 and not a.no_cpu_baseline:
            res["cpu_baseline"], res["parity"] = cpu_baseline(fix.cpu().numpy(), mov.cpu().numpy(), field_of_timed_loop)
            oracle_fast = res["parity"].pop("_oracle_fast_field")
            if a.adam_mode == "fast":                              # profiling runs of the opt-in mode: the checker is the oracle's restatement of THAT mode
                import numpy as np
                got = np.moveaxis(field_of_timed_loop, 0, -1).astype(np.float64)
                res["parity"].update(bit_identical=bool(np.array_equal(got, oracle_fast)), max_abs_diff=float(np.abs(got - oracle_fast).max()),
                                     epe_vs_oracle=float(np.sqrt(((got - oracle_fast) ** 2).sum(-1)).mean()))
            res["parity"]["tolerance_epe"] = TOLERANCE_EPE
            res["parity"].update(mode_parity(fix, mov, dev, oracle_fast))
            del oracle_fast
            res["parity"]["timed_mode"]["ms_per_pair"] = res["ms_per_step"]
            res["parity"]["exact_mode"]["ms_per_pair"] = res["ms_per_step"]
            res["parity"]["exact_mode"]["pairs_per_s"] = res["value"]
            res["parity"]["reference_bits_mode"] = reference_bits_check(fix, mov, dev)
            # what the line means for someone who asks "pairs/s at < 1e-3 voxel of the reference after 80 iterations"
            res["tolerance_met"] = bool(res["parity"]["timed_mode"]["tolerance_met_80it"])
            res["value_at_tolerance"] = res["parity"]["reference_bits_mode"]["pairs_per_s"] if res["parity"]["reference_bits_mode"]["tolerance_met"] else None
            res["value_exact_mode"] = res["value"]
            res["value_fast_mode"] = res["parity"]["fast_mode"]["pairs_per_s"]
            res["api"] = api_path(fix, mov, dev, res["ms_per_step"])
        if n == 1 and not a.no_batched:
            res["configs"] = secondary_configs(dev)
        extra = a.extra_out
        if extra:
            try:
                with open(extra, "w") as f:
                    f.write(json.dumps(res) + "\n")
            except OSError as e:                                   # (a read-only checkout: the line still goes out)
                print("bench.py: cannot write %s: %s" % (extra, e), file=sys.stderr)
                extra = None
        print(json.dumps(bench_line(res, extra)))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
