"""The L2R-2022 self-configuration of self_configuring/l2r3.py on the device (csrc/ranksum.hip): the ablation over feature
kind x grid spacing x search half-width x lambda x nine (iterations, smoothing) snapshots, and the parameter selection that ends it --
50 noise draws per metric, scipy.stats.ranksums on every ordered pair of the N "teams", rank scores with averaged ties, the geometric
mean over the metrics (:223-375).  The rank-sum decisions are integer counts taken by one kernel launch per metric.

    ranksum_better(samples, means, scale, sign, p_threshold, return_u2)   (R, N, S) device samples -> (R, N) int32 scores [, U2]
    ranksum_statistic(u2, S), critical_u2(S, p_threshold)                 scipy's z of a U2 (host float64); the integer threshold of a decision
    scores_better, rankscore_avgtie, greaters                             the three nested helpers of :262-295
    rank_experiments(data, noise, repeats, p_threshold)                   :227-361 on the dict of ablations_<task>.json
    parse_winner(key)                                                     :363-374
    SAVE_PATHS, experiment_key, options_for, mind_parameters              :22, :123, :56-71, :97-102
    aggregate_cases(values)                                               mean / std / '30' of per-case values (this project's definition)
    self_configure(pairs, expected_shape, ...)                            the ablation loop (:105-220) on the device, then the selection

Device tensors only for everything that compares samples: there is no CPU path.
"""
import ctypes as C
import json
import math
import os
import time

import numpy as np
import torch

from ._lib import call, check, lib, ptr, require_device_tensor

SNAPSHOT_ITERS, SNAPSHOT_SMOOTHS = (40, 60, 80), (0, 3, 5)
# the nine result folders of one Adam run, in the reference's order (:22): the smoothing is the slower index
SAVE_PATHS = ["%d_smoothing%d" % (it, sm) for sm in SNAPSHOT_SMOOTHS for it in SNAPSHOT_ITERS]
MAX_EXTENT = 4096          # N and S of cvx_ranksum_better_f64


# ---- the rank-sum decisions --------------------------------------------------------------------------------------------------------
def critical_u2(S, p_threshold=0.05):
    """The smallest U2 = 2 #{a > b} + #{a == b} of two samples of S values each for which scipy.stats.ranksums gives a positive statistic
    and a p-value below `p_threshold`; 2 S^2 + 1 when no value does (S = 1, S = 2 at 0.05).  Host arithmetic of the library
    (cvx_ranksum_critical_u2); no device."""
    S, p = int(S), float(p_threshold)
    if not 1 <= S <= MAX_EXTENT:
        raise ValueError("S must lie in 1..%d, got %d" % (MAX_EXTENT, S))
    if not 0.0 < p < 1.0:
        raise ValueError("p_threshold must lie inside (0, 1), got %r" % (p_threshold,))
    out = C.c_int(0)
    check(lib().cvx_ranksum_critical_u2(S, p, C.byref(out)))
    return out.value


def ranksum_statistic(u2, S):
    """The `statistic` scipy.stats.ranksums returns for two samples of S values with this U2, bit for bit (host float64)."""
    S = int(S)
    s = np.asarray(u2, dtype=np.float64) / 2.0 + float(S * (S + 1) // 2)
    return (s - S * (2 * S + 1) / 2.0) / np.sqrt(S * S * (2 * S + 1) / 12.0)


def ranksum_better(samples, means=None, scale=0.1, sign=1.0, p_threshold=0.05, return_u2=False):
    """samples: (R, N, S) device tensor, R independent repeats of N teams with S values each.  With `means` ((N,), taken through
    float32) the values compared are sign * (float64(mean_i) + scale * samples[r, i, k]); without, the samples as given.
    Returns scores (R, N) int32 on the device: scores[r, j] = how many teams i are significantly greater than team j in repeat r,
    i.e. statistic > 0 and pvalue < p_threshold of scipy.stats.ranksums(x_i, x_j); with return_u2 also U2 (R, N, N) int32."""
    if not isinstance(samples, torch.Tensor):
        raise TypeError("samples must be a torch.Tensor")
    shape = tuple(int(s) for s in samples.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("samples must be (R, N, S) with no empty axis, got %s" % (shape,))
    R, N, S = shape
    if N > MAX_EXTENT or S > MAX_EXTENT:
        raise ValueError("at most %d teams and %d samples per team, got %d and %d" % (MAX_EXTENT, MAX_EXTENT, N, S))
    if R * N * S > 2 ** 31 - 1 or (return_u2 and R * N * N > 2 ** 31 - 1):
        raise ValueError("more than 2^31 - 1 elements: (R, N, S) = %s" % (shape,))
    if means is not None:
        if not isinstance(means, torch.Tensor):
            raise TypeError("means must be a torch.Tensor or None")
        if tuple(means.shape) != (N,):
            raise ValueError("means must be (%d,), got %s" % (N, tuple(means.shape)))
        if not (math.isfinite(float(scale)) and math.isfinite(float(sign))):
            raise ValueError("scale and sign must be finite, got %r and %r" % (scale, sign))
    crit = critical_u2(S, p_threshold)
    x = require_device_tensor(samples, "samples").detach().to(torch.float64).contiguous()
    dev = x.device
    m = None
    if means is not None:
        m = require_device_tensor(means, "means").detach().to(device=dev, dtype=torch.float32).contiguous()
    scores = torch.empty((R, N), dtype=torch.int32, device=dev)
    u2 = torch.empty((R, N, N), dtype=torch.int32, device=dev) if return_u2 else None
    call(dev, "cvx_ranksum_better_f64", ptr(x), ptr(m), float(scale), float(sign), R, N, S, crit, ptr(scores), ptr(u2))
    return (scores, u2) if return_u2 else scores


def _to_device(a, dtype, device=None):
    if isinstance(a, torch.Tensor):
        return a.to(dtype) if device is None else a.to(device=device, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(device=device or "cuda", dtype=dtype)


def scores_better(task_metric, p_threshold=0.05):
    """scores_better of :262-271: task_metric (N, S), array or tensor -> (N,) float64, entry j the number of teams whose samples are
    significantly greater than team j's.  An array is uploaded; the comparisons run in the kernel."""
    if len(task_metric.shape) != 2:
        raise ValueError("task_metric must be (N, S), got %s" % (tuple(task_metric.shape),))
    x = _to_device(task_metric, torch.float64)
    return ranksum_better(x[None], p_threshold=p_threshold)[0].cpu().numpy().astype(np.float64)


def rankscore_avgtie(scores_int):
    """rankscore_avgtie of :274-292 (host): teams in ascending order of `scores_int` get the rank scores linspace(0.1, 1, N); tied
    teams share the average of theirs.  Called with -scores, whose entries index the accumulator from its end as in the reference;
    the order is a stable argsort and the sums run over ascending i."""
    v = np.asarray(scores_int).astype(np.int64).reshape(-1)
    n = v.size
    if n and (v.min() < -n or v.max() >= n):
        raise IndexError("scores outside [-%d, %d) do not index %d accumulators" % (n, n, n))
    rankscale = np.linspace(.1, 1, n)
    position = np.empty(n, np.int64)
    position[np.argsort(v, kind="stable")] = np.arange(n)
    slot = np.where(v < 0, v + n, v)
    sums, counts = np.zeros(n), np.zeros(n)
    np.add.at(sums, slot, rankscale[position])                  # unbuffered: one addition per team, in ascending i
    np.add.at(counts, slot, 1.0)
    return (sums / np.maximum(counts, 1e-6))[slot]


def greaters(scores):
    """greaters of :294-295: entry j = how many entries of `scores` are smaller than scores[j]."""
    s = np.asarray(scores).reshape(-1)
    return np.sum(s.reshape(1, -1) > s.reshape(-1, 1), 0)


# ---- the selection -----------------------------------------------------------------------------------------------------------------
def _metric_blocks(data):
    """[(name, per-team values, sign, noise scale)] in the reference's order; the team keys"""
    keys = [k for k in data.keys() if k.startswith("MIND") or k.startswith("nnUNet")]
    if not keys:
        raise ValueError("no team keys (starting with 'MIND' or 'nnUNet') in the data")
    metrics = data["metrics"]
    sign = lambda name: 1.0 if "DSC" in name else -1.0          # noqa: E731
    s1 = sign(metrics["sim1"])
    blocks = [("sim1_mean", [data[k]["sim1"]["mean"] for k in keys], s1, 0.1),
              ("sim1_30", [data[k]["sim1"]["30"] for k in keys], s1, 0.1),
              ("smooth", [data[k]["smooth"]["mean"] for k in keys], -1.0, 0.1),
              ("time", [data[k]["time"] for k in keys], -1.0, 0.2)]
    if metrics.get("sim2") is not None:
        blocks.append(("sim2_mean", [data[k]["sim2"]["mean"] for k in keys], sign(metrics["sim2"]), 0.1))
    return blocks, keys


def rank_experiments(data, noise=None, repeats=50, p_threshold=0.05, device=None):
    """The ranking of :227-361 on the dict that ablations_<task>.json holds: data['metrics'] names the metrics, every key starting with
    'MIND' or 'nnUNet' is a team with 'sim1' / 'smooth' (/ 'sim2') aggregates and 'time'.  Per metric block -- sim1 mean, sim1 '30',
    smooth, time, then sim2 mean -- `repeats` times: samples = sign * (float32 mean + scale * randn(N, N)) (sign +1 for a metric whose
    name contains 'DSC', else -1; scale 0.1, 0.2 for time), scores_better, rankscore_avgtie(-scores); the block's column of rank_all is
    the mean over the repeats, the last column power(rank_all[:, 0] * prod(rank_all[:, :n], axis=1), 1 / n) with n = 4 or 5 -- the sim1
    column enters twice, as in the reference.  One kernel launch per block.

    noise: None draws np.random.randn(N, N) from numpy's global state in the reference's order, so np.random.seed(s) before the call
    reproduces a reference run after the same seed; otherwise an array (n_blocks, repeats, N, N).
    data['metrics']['sim2'] absent or None both mean four metrics (the reference raises NameError / KeyError when the key is present
    but None, :239-254; it runs four metrics only with the key absent).
    Returns (rank_all (N, n + 1) float64, team keys, winner key)."""
    blocks, keys = _metric_blocks(data)
    N, nb = len(keys), len(blocks)
    repeats = int(repeats)
    if repeats < 1:
        raise ValueError("repeats must be at least 1, got %d" % repeats)
    if noise is not None:
        noise = np.asarray(noise, dtype=np.float64)
        if noise.shape != (nb, repeats, N, N):
            raise ValueError("noise must be (n_blocks, repeats, N, N) = %s, got %s" % ((nb, repeats, N, N), noise.shape))
    dev = torch.device(device if device is not None else "cuda")
    rank_all = np.zeros((N, nb + 1))
    for b, (_, values, sign, scale) in enumerate(blocks):
        draws = noise[b] if noise is not None else np.stack([np.random.randn(N, N) for _ in range(repeats)])
        means = torch.Tensor(values).to(dev)                     # through float32, as the reference's torch.Tensor(list)
        scores = ranksum_better(torch.from_numpy(np.ascontiguousarray(draws)).to(dev), means, scale, sign, p_threshold).cpu().numpy()
        acc = np.zeros(N)
        for r in range(repeats):
            acc += rankscore_avgtie(-scores[r].astype(np.int64))
        rank_all[:, b] = acc / repeats
    rank_all[:, nb] = np.power(rank_all[:, 0] * np.prod(rank_all[:, :nb], axis=1), 1 / nb)
    return rank_all, keys, keys[int(np.argmax(rank_all[:, nb]))]


def parse_winner(key):
    """:363-374, with its character slicing: the last character of 'gs=..' and 'disp_hwd=..', what follows 'lambda=', the first two
    characters and the last one of the folder name."""
    part = key.replace(" ", "").split(";")
    return dict(semantic_features=part[0] == "nnUNet", grid_sp=int(part[1][-1]), disp_hw=int(part[2][-1]), lambda_weight=float(part[3][7:]),
                selected_niter=int(part[4][:2]), selected_smooth=int(part[4][-1]))


def experiment_key(features, grid_sp, disp_hw, lambda_weight, save_path):
    """The key of one team in ablations_<task>.json (:123, :181); features: 'MIND' or 'nnUNet'."""
    if features not in ("MIND", "nnUNet"):
        raise ValueError("features must be 'MIND' or 'nnUNet', got %r" % (features,))
    return features + "; gs=" + str(grid_sp) + "; disp_hwd=" + str(disp_hw) + "; lambda=" + str(lambda_weight) + "; " + save_path


def options_for(expected_shape):
    """The ablation grid of :56-71: volumes above 10^6 voxels get grid spacing 6 with half-widths 6 and 4, smaller ones 4 with 4 and 2."""
    large = expected_shape[0] * expected_shape[1] * expected_shape[2] > 1000000
    return dict(grid_sp=[6] if large else [4], disp_hw=[6, 4] if large else [4, 2], lambda_weight=[0.75, 1.0, 1.25])


def mind_parameters(modality_fixed, modality_moving):
    """(mind_r, mind_d) of :97-102: (3, 3) when either modality names ultrasound, else (1, 2)."""
    return (3, 3) if ("US" in modality_fixed) or ("US" in modality_moving) else (1, 2)


# ---- the ablation ------------------------------------------------------------------------------------------------------------------
def aggregate_cases(values):
    """{'mean', 'std', '30'} of the per-case values of one metric.  The L2R evaluation package that writes these aggregates for the
    reference is not part of it, so the definitions here are this project's own and pinned to nothing: numpy.mean, numpy.std
    (population) and numpy.quantile(values, 0.3) (linear interpolation)."""
    v = np.asarray(values, dtype=np.float64)
    return {"mean": float(np.mean(v)), "std": float(np.std(v)), "30": float(np.quantile(v, 0.3))}


_EVAL_NAME = {"DSC": "dice", "HD95": "hd95", "TRE": "tre", "LogJacDetStd": "jstd"}


def self_configure(pairs, expected_shape, modality_fixed="MR", modality_moving="MR", semantic_features=False, sim2="auto", options=None,
                   result_path=None, task_name="task", repeats=50, noise=None, p_threshold=0.05, aggregate=aggregate_cases, adam_mode=None):
    """The ablation loop of sc_convex_adam (:105-220) and its selection (:223-374) on the device.

    pairs: validation pairs, each a dict of device tensors: 'fixed', 'moving' (H, W, D) images; 'seg_fixed', 'seg_moving' label maps
    with 'num_labels' labels above the background; optionally 'key_fixed', 'key_moving' (K, 3) key points.
    For every (grid_sp, disp_hw, lambda) of options_for(expected_shape) -- or of `options`, a dict of the same three lists -- and MIND
    features (and label features when `semantic_features`), every pair is registered once by register_pair_snapshots_device (iterations
    40 / 60 / 80 x smoothing 0 / 3 / 5 of one Adam run); each of the nine fields is scored by sweep.evaluate_item and the per-case
    values are aggregated by `aggregate` (aggregate_cases) into the reference's record: sim1 = 'DSC', smooth = 'LogJacDetStd', sim2 =
    'HD95' ('auto': the pairs always carry segmentations here, because sim1 needs them), 'TRE' on request (the pairs then need key
    points), or None, which leaves sim2 out (four metrics).  'time' is the median over the pairs of the wall time of the one run, synchronised, that produced a
    team's field; the nine teams of one run share it.  The dict is written to <result_path>/<task_name>/ablations_<task_name>.json when
    result_path is given.  Returns dict(experiments, rank_all, keys, winner, **parse_winner(winner))."""
    from . import sweep
    from .convex_adam_MIND import register_pair_snapshots_device
    from .convex_adam_nnUNet import extract_features as label_features
    if not pairs:
        raise ValueError("no validation pairs")
    sim2 = "HD95" if sim2 == "auto" else sim2
    if sim2 not in ("HD95", "TRE", None):
        raise ValueError("sim2 must be 'HD95', 'TRE', 'auto' or None, got %r" % (sim2,))
    for p in pairs:
        missing = [k for k in ("fixed", "moving", "seg_fixed", "seg_moving", "num_labels") if k not in p]
        if sim2 == "TRE":
            missing += [k for k in ("key_fixed", "key_moving") if k not in p]
        if missing:
            raise ValueError("a validation pair lacks %s" % ", ".join(missing))
    grid = options_for(expected_shape) if options is None else options
    mind_r, mind_d = mind_parameters(modality_fixed, modality_moving)
    experiments = {"metrics": {"smooth": "LogJacDetStd", "sim1": "DSC", "sim2": sim2}}
    names = [("sim1", "DSC"), ("smooth", "LogJacDetStd")] + ([("sim2", sim2)] if sim2 is not None else [])
    caches = [{} for _ in pairs]
    dev = pairs[0]["fixed"].device
    for grid_sp in grid["grid_sp"]:
        for disp_hw in grid["disp_hw"]:
            for lam in grid["lambda_weight"]:
                for features in ("MIND", "nnUNet") if semantic_features else ("MIND",):
                    values = [{name: [] for _, name in names} for _ in SAVE_PATHS]
                    times = []
                    for p, cache in zip(pairs, caches):
                        torch.cuda.synchronize(dev)
                        t0 = time.time()
                        if features == "MIND":
                            fields = register_pair_snapshots_device(p["fixed"], p["moving"], snapshot_iters=SNAPSHOT_ITERS, smooths=SNAPSHOT_SMOOTHS,
                                                                    mind_r=mind_r, mind_d=mind_d, lambda_weight=lam, grid_sp=grid_sp, disp_hw=disp_hw,
                                                                    adam_mode=adam_mode)
                        else:
                            ff, fm = label_features(p["seg_fixed"], p["seg_moving"], device=dev)
                            fields = register_pair_snapshots_device(feat_fixed=ff[0], feat_moving=fm[0], snapshot_iters=SNAPSHOT_ITERS,
                                                                    smooths=SNAPSHOT_SMOOTHS, lambda_weight=lam, grid_sp=grid_sp, disp_hw=disp_hw,
                                                                    adam_mode=adam_mode)
                        torch.cuda.synchronize(dev)
                        times.append(time.time() - t0)
                        kf = p.get("key_fixed", torch.zeros(1, 3))
                        km = p.get("key_moving", torch.zeros(1, 3))
                        for t, _ in enumerate(SAVE_PATHS):       # folder t: iteration t % 3, smoothing t // 3
                            rec = sweep.evaluate_item(fields[t % 3, t // 3], p["seg_fixed"], p["seg_moving"], kf, km, p["num_labels"], cache=cache)
                            for _, name in names:
                                values[t][name].append(rec[_EVAL_NAME[name]])
                    for t, save_path in enumerate(SAVE_PATHS):
                        team = {"time": float(np.median(times))}
                        for slot, name in names:
                            team[slot] = aggregate(values[t][name])
                        experiments[experiment_key(features, grid_sp, disp_hw, lam, save_path)] = team
    if result_path is not None:
        folder = os.path.join(result_path, task_name)
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, "ablations_" + task_name + ".json"), "w") as fh:
            json.dump(experiments, fh)
    rank_all, keys, winner = rank_experiments(experiments, noise=noise, repeats=repeats, p_threshold=p_threshold, device=dev)
    return dict(experiments=experiments, rank_all=rank_all, keys=keys, winner=winner, **parse_winner(winner))
