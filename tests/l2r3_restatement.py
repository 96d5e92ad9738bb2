"""numpy restatement of the ranking that ends the L2R-2022 self-configuration (self_configuring/l2r3.py:227-361), written independently
of convexadam_amd.l2r3 and of the kernel (csrc/ranksum.hip); the tests hold both to it, and it to scipy and to the reference's own block
(tests/golden/l2r3.npz).

    transform(samples, means, scale, sign)   x = sign * (float64(float32 mean) + scale * samples), every operation rounded
    u2_brute(x)                              U2[r, i, j] = 2 #{a > b} + #{a == b} over a in x[r, i], b in x[r, j], by broadcasting
    statistic(u2, S)                         z of scipy.stats.ranksums for n1 = n2 = S
    critical_u2(S, p)                        the smallest U2 above S^2 with z > 0 and erfc(|z| / sqrt 2) < p, by a scan; 2 S^2 + 1 if none
    scores(u2, crit)                         column sums of U2 >= crit
    scores_better / rankscore_avgtie / greaters / rank_all     the reference's helpers and ranking block
    golden_data(g, case) / golden_noise(...)                   the dict and the noise of a golden case
"""
import math

import numpy as np

SAVE_PATHS = ["%d_smoothing%d" % (it, sm) for sm in (0, 3, 5) for it in (40, 60, 80)]
CASES = {
    # case: (feature kinds, gs, hw, lambdas, metric names)
    "with_sim2": (("MIND",), 6, 6, (0.75, 1.25), dict(smooth="LogJacDetStd", sim1="DSC", sim2="HD95")),
    "four_metrics": (("MIND", "nnUNet"), 4, 4, (1.0,), dict(smooth="LogJacDetStd", sim1="DSC")),
}
SEED = 11


def transform(samples, means=None, scale=0.1, sign=1.0):
    s = np.asarray(samples, np.float64)
    if means is None:
        return s
    m = np.asarray(means, np.float32).astype(np.float64)
    return sign * (m[:, None] + scale * s)


def u2_brute(x):
    """x (R, N, S) -> (R, N, N) int64"""
    x = np.asarray(x, np.float64)
    out = np.empty((x.shape[0], x.shape[1], x.shape[1]), np.int64)
    with np.errstate(invalid="ignore"):
        for r in range(x.shape[0]):
            for j in range(x.shape[1]):
                a, b = x[r][:, :, None], x[r, j][None, None, :]
                out[r, :, j] = 2 * (a > b).sum((1, 2)) + (a == b).sum((1, 2))
    return out


def statistic(u2, S):
    s = np.asarray(u2, np.float64) / 2.0 + S * (S + 1) / 2
    expected = S * (2 * S + 1) / 2.0
    return (s - expected) / np.sqrt(S * S * (2 * S + 1) / 12.0)


def pvalue_erfc(z):
    return math.erfc(abs(z) / math.sqrt(2.0))


def critical_u2(S, p_threshold=0.05):
    for u2 in range(S * S + 1, 2 * S * S + 1):
        z = float(statistic(u2, S))
        if z > 0 and pvalue_erfc(z) < p_threshold:
            return u2
    return 2 * S * S + 1


def scores(u2, crit):
    return (np.asarray(u2) >= crit).sum(-2)


def scores_better(task_metric, p_threshold=0.05):
    x = np.asarray(task_metric, np.float64)
    return scores(u2_brute(x[None])[0], critical_u2(x.shape[1], p_threshold)).astype(np.float64)


def rankscore_avgtie(scores_int):
    n = len(scores_int)
    scale = np.linspace(.1, 1, n)
    place = np.empty(n, np.int64)
    place[np.argsort(scores_int, kind="stable")] = np.arange(n)
    total, count = [0.0] * n, [0] * n
    for i in range(n):                                           # a negative score indexes from the end, as numpy does
        total[int(scores_int[i]) % n] += scale[place[i]]
        count[int(scores_int[i]) % n] += 1
    return np.array([total[int(v) % n] / max(count[int(v) % n], 1e-6) for v in scores_int])


def greaters(s):
    s = np.asarray(s)
    return np.array([int((s[j] > s).sum()) for j in range(len(s))])


def team_keys(data):
    return [k for k in data if k.startswith("MIND") or k.startswith("nnUNet")]


def blocks_of(data):
    """[(values per team, sign, noise scale)] in the reference's order: sim1 mean, sim1 '30', smooth, time, sim2 mean"""
    keys = team_keys(data)
    sgn = lambda name: 1.0 if "DSC" in name else -1.0          # noqa: E731
    s1 = sgn(data["metrics"]["sim1"])
    out = [([data[k]["sim1"]["mean"] for k in keys], s1, 0.1), ([data[k]["sim1"]["30"] for k in keys], s1, 0.1),
           ([data[k]["smooth"]["mean"] for k in keys], -1.0, 0.1), ([data[k]["time"] for k in keys], -1.0, 0.2)]
    if data["metrics"].get("sim2") is not None:
        out.append(([data[k]["sim2"]["mean"] for k in keys], sgn(data["metrics"]["sim2"]), 0.1))
    return out


def rank_all(data, noise, score_fn=None):
    """noise (n_blocks, repeats, N, N) -> (rank_all (N, n_blocks + 1), keys, winner).  score_fn(x (R, N, S)) -> (R, N) scores; the brute
    force when None."""
    keys = team_keys(data)
    blocks = blocks_of(data)
    n, nb = len(keys), len(blocks)
    out = np.zeros((n, nb + 1))
    for b, (values, sign, scale) in enumerate(blocks):
        x = np.stack([transform(noise[b, r], values, scale, sign) for r in range(noise.shape[1])])
        sc = score_fn(x) if score_fn is not None else scores(u2_brute(x), critical_u2(n))
        acc = np.zeros(n)
        for r in range(noise.shape[1]):
            acc += rankscore_avgtie(-np.asarray(sc[r]).astype(np.int64))
        out[:, b] = acc / noise.shape[1]
    out[:, nb] = np.power(out[:, 0] * np.prod(out[:, :nb], axis=1), 1 / nb)
    return out, keys, keys[int(np.argmax(out[:, nb]))]


# ---- the golden cases ------------------------------------------------------------------------------------------------------------
def case_keys(case):
    kinds, gs, hw, lams, _ = CASES[case]
    return ["%s; gs=%d; disp_hwd=%d; lambda=%s; %s" % (kind, gs, hw, lam, sp) for lam in lams for kind in kinds for sp in SAVE_PATHS]


def synthetic_means(case):
    """per-team aggregates of a made-up ablation: RandomState(7), one draw of five columns per case in the order of CASES"""
    rng = np.random.RandomState(7)
    cols = {}
    for name in CASES:
        u = rng.rand(18, 5)
        cols[name] = dict(sim1_mean=0.55 + 0.3 * u[:, 0], sim1_30=0.35 + 0.3 * u[:, 1], smooth=0.05 + 0.3 * u[:, 2], time=1.0 + 0.6 * u[:, 3],
                          sim2=2.0 + 1.0 * u[:, 4])
    return cols[case]


def data_of(case, cols):
    """the dict ablations_<task>.json holds, from per-team columns"""
    metrics = CASES[case][4]
    data = {"metrics": dict(metrics)}
    for t, key in enumerate(case_keys(case)):
        rec = {"time": float(cols["time"][t]),
               "sim1": {"mean": float(cols["sim1_mean"][t]), "std": 0.0, "30": float(cols["sim1_30"][t])},
               "smooth": {"mean": float(cols["smooth"][t]), "std": 0.0, "30": 0.0}}
        if "sim2" in metrics:
            rec["sim2"] = {"mean": float(cols["sim2"][t]), "std": 0.0, "30": 0.0}
        data[key] = rec
    return data


def golden_data(g, case):
    return data_of(case, {c: g["%s_%s" % (case, c)] for c in ("sim1_mean", "sim1_30", "smooth", "time", "sim2")})


def golden_noise(case, repeats=50, n=18):
    """what np.random.seed(SEED) followed by the block's consecutive randn(N, N) draws gives"""
    nb = 5 if "sim2" in CASES[case][4] else 4
    rng = np.random.RandomState(SEED)
    return np.stack([np.stack([rng.randn(n, n) for _ in range(repeats)]) for _ in range(nb)])


def first_noisy_subset(g, case):
    data = golden_data(g, case)
    values, sign, scale = blocks_of(data)[0]
    return transform(np.random.RandomState(SEED).randn(18, 18), values, scale, sign)
