"""The rank-sum kernel (csrc/ranksum.hip) and the L2R-2022 selection built on it (convexadam_amd/l2r3.py) on the device: U2 and scores
equal the numpy restatement (tests/l2r3_restatement.py) exactly -- they are integer counts -- at every sample count at which the kernel
changes its path (one, two, four values per lane: S <= 64, <= 128, above; rows that overhang the wavefront; more rows than wavefronts;
x_j longer than one pass of the group), on ties, NaN, infinities and signed zeros; the selection equals the reference's own block
(tests/golden/l2r3.npz) within the 1e-12 that tests/test_l2r3_reference.py derives; self_configure joins the registration, the
evaluation and the selection."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import l2r3_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 2, 2), (3, 3, 3), (2, 5, 63), (2, 5, 64), (2, 5, 65), (1, 65, 7), (1, 3, 128), (1, 3, 129), (2, 9, 257), (1, 4, 1024),
          (50, 18, 18), (1, 108, 108)]
SENTINEL, PAD = 0x5A5A5A5A, 64


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def raw_call(dev, samples, means, scale, sign, crit, want_u2=True):
    """cvx_ranksum_better_f64 on guarded buffers -> (scores, u2 or None) as numpy; asserts the guards around both outputs are intact"""
    from convexadam_amd._lib import check, lib, ptr, stream_ptr
    Rn, N, S = samples.shape
    x = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float64)).to(dev)
    m = torch.from_numpy(np.asarray(means, dtype=np.float32)).to(dev) if means is not None else None
    sc = torch.full((PAD + Rn * N + PAD,), SENTINEL, dtype=torch.int32, device=dev)
    u = torch.full((PAD + Rn * N * N + PAD,), SENTINEL, dtype=torch.int32, device=dev) if want_u2 else None
    with torch.cuda.device(dev):
        check(lib().cvx_ranksum_better_f64(ptr(x), ptr(m), float(scale), float(sign), Rn, N, S, int(crit), C.c_void_p(sc.data_ptr() + 4 * PAD),
                                           C.c_void_p(u.data_ptr() + 4 * PAD) if want_u2 else None, stream_ptr(dev)))
    out = []
    for buf, n, shape in ((sc, Rn * N, (Rn, N)), (u, Rn * N * N, (Rn, N, N))):
        if buf is None:
            out.append(None)
            continue
        h = buf.cpu().numpy()
        assert np.all(h[:PAD] == SENTINEL) and np.all(h[PAD + n:] == SENTINEL), "a guard word was overwritten"
        out.append(h[PAD:PAD + n].reshape(shape))
    return out


def check_case(dev, samples, means=None, scale=0.1, sign=1.0):
    S = samples.shape[2]
    crit = R.critical_u2(S)
    want_u2 = R.u2_brute(R.transform(samples, means, scale, sign) if means is not None else samples)
    want_scores = R.scores(want_u2, crit)
    scores, u2 = raw_call(dev, samples, means, scale, sign, crit)
    assert np.array_equal(u2, want_u2), "U2 differs at %s" % (np.argwhere(u2 != want_u2)[:4],)
    assert np.array_equal(scores, want_scores)
    scores_alone, none = raw_call(dev, samples, means, scale, sign, crit, want_u2=False)
    assert none is None and np.array_equal(scores_alone, scores)                 # u2 = NULL gives the same scores
    return want_u2, want_scores


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_u2_and_scores_equal_the_restatement(dev, shape):
    Rn, N, S = shape
    rng = np.random.default_rng(Rn * 10007 + N * 101 + S)
    noise = rng.standard_normal(shape)
    means = (0.5 + 0.2 * rng.random(N)).astype(np.float32)
    check_case(dev, noise, means, 0.1, 1.0)
    check_case(dev, noise, means, 0.2, -1.0)
    _, sc = check_case(dev, noise + 0.3 * np.arange(N)[None, :, None])           # raw rows, means = NULL: shifted, so that scores are not all 0
    assert N < 5 or S < 5 or sc.max() > 0
    check_case(dev, rng.integers(0, 4, shape).astype(np.float64))                 # the a == b path
    u2, sc = check_case(dev, np.full(shape, 1.25))                                # all equal
    assert np.all(u2 == S * S) and np.all(sc == 0)
    special = noise.copy()
    for i, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0)[:N]):
        special[:, i, :] = v
    u2, sc = check_case(dev, special)
    assert np.all(u2[:, 0, :] == 0) and np.all(u2[:, :, 0] == 0)                  # a NaN team is never better, nothing is better than it
    if N >= 5:
        assert np.all(u2[:, 3, 4] == S * S) and np.all(u2[:, 4, 3] == S * S)      # -0.0 == 0.0
        assert np.all(u2[:, 1, 2:] == 2 * S * S) and np.all(u2[:, 2, 1] == 0) and np.all(u2[:, 1, 1] == S * S)   # +-inf are ordinary values
    special_means = rng.standard_normal(N).astype(np.float32)
    check_case(dev, special, special_means, 0.1, -1.0)


def test_threshold_special_values(dev):
    Rn, N, S = 2, 5, 65
    rng = np.random.default_rng(3)
    x = rng.standard_normal((Rn, N, S)) + 0.4 * np.arange(N)[None, :, None]
    u2 = R.u2_brute(x)
    every, _ = raw_call(dev, x, None, 0.0, 0.0, 0)
    assert np.all(every == N)
    none, _ = raw_call(dev, x, None, 0.0, 0.0, 2 * S * S + 1)
    assert np.all(none == 0)
    real, got_u2 = raw_call(dev, x, None, 0.0, 0.0, R.critical_u2(S))
    assert np.array_equal(got_u2, u2) and np.array_equal(real, R.scores(u2, R.critical_u2(S))) and 0 < real.max() < N
    from convexadam_amd.l2r3 import ranksum_better
    xd = torch.from_numpy(x).to(dev)
    sc, ud = ranksum_better(xd, return_u2=True)
    assert sc.dtype == torch.int32 and sc.shape == (Rn, N) and ud.shape == (Rn, N, N) and sc.device == xd.device
    assert np.array_equal(sc.cpu().numpy(), real) and np.array_equal(ud.cpu().numpy(), u2)
    loose = ranksum_better(xd, p_threshold=0.5).cpu().numpy()
    assert np.array_equal(loose, R.scores(u2, R.critical_u2(S, 0.5))) and loose.sum() > real.sum()
    assert np.array_equal(ranksum_better(xd.float()).cpu().numpy(), R.scores(R.u2_brute(x.astype(np.float32)), R.critical_u2(S)))


def test_scores_better_equals_the_reference(dev, golden):
    from convexadam_amd.l2r3 import scores_better
    g = golden("l2r3")
    for case in R.CASES:
        got = scores_better(R.first_noisy_subset(g, case))
        assert got.dtype == np.float64 and np.array_equal(got, g[case + "_first_scores"])
    assert np.array_equal(scores_better(g["ties_subset"]), g["ties_scores"])
    assert np.array_equal(scores_better(torch.from_numpy(g["nan_subset"]).to(dev)), g["nan_scores"])


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_rank_experiments_equals_the_reference(dev, golden, case):
    from convexadam_amd.l2r3 import rank_experiments
    g = golden("l2r3")
    data = R.golden_data(g, case)
    state = np.random.get_state()
    try:
        np.random.seed(R.SEED)
        rank_all, keys, winner = rank_experiments(data)
    finally:
        np.random.set_state(state)
    want = g[case + "_rank_all"]
    worst = np.abs(rank_all - want).max(0)
    print(case, "max |delta| per column", worst)
    assert rank_all.shape == want.shape and np.all(worst <= 1e-12), worst
    assert keys == R.case_keys(case) and winner == g[case + "_winner"].item().decode()
    again, _, winner2 = rank_experiments(data, noise=R.golden_noise(case))
    assert np.array_equal(again, rank_all) and winner2 == winner
    mine, _, winner3 = R.rank_all(data, R.golden_noise(case))
    assert np.array_equal(mine, rank_all) and winner3 == winner                  # restatement and device path: the same scores, the same host sums
    if case == "four_metrics":                                                    # 'sim2': None is four metrics too
        data["metrics"]["sim2"] = None
        assert np.array_equal(rank_experiments(data, noise=R.golden_noise(case))[0], rank_all)


def test_self_configure(dev, tmp_path):
    from convexadam_amd import l2r3, sweep
    from convexadam_amd.convex_adam_MIND import register_pair_snapshots_device
    shape = (32, 40, 48)
    pairs = []
    for idx in range(2):
        fix, mov = sweep._make_pair(shape, idx, dev)
        seg_f, seg_m, key_f, key_m, nl = sweep._make_labels(shape, idx, dev)
        pairs.append(dict(fixed=fix, moving=mov, seg_fixed=seg_f, seg_moving=seg_m, key_fixed=key_f, key_moving=key_m, num_labels=nl))
    options = dict(grid_sp=[4], disp_hw=[2], lambda_weight=[0.75, 1.25])
    noise = np.random.RandomState(4).randn(5, 50, 18, 18)
    out = l2r3.self_configure(pairs, shape, options=options, result_path=str(tmp_path), task_name="phantom", noise=noise)
    want_keys = [l2r3.experiment_key("MIND", 4, 2, lam, sp) for lam in (0.75, 1.25) for sp in l2r3.SAVE_PATHS]
    assert out["keys"] == want_keys and len(want_keys) == 18
    assert out["keys"][0] == "MIND; gs=4; disp_hwd=2; lambda=0.75; 40_smoothing0"
    exp = out["experiments"]
    assert list(exp) == ["metrics"] + want_keys and exp["metrics"] == {"smooth": "LogJacDetStd", "sim1": "DSC", "sim2": "HD95"}
    for k in want_keys:
        assert sorted(exp[k]) == ["sim1", "sim2", "smooth", "time"] and exp[k]["time"] > 0
        for slot in ("sim1", "sim2", "smooth"):
            assert sorted(exp[k][slot]) == ["30", "mean", "std"] and all(np.isfinite(v) for v in exp[k][slot].values())
    # the winner lies in the grid, and its fields are what parse_winner reads off the key
    assert out["winner"] in want_keys and out["rank_all"].shape == (18, 6)
    assert out["semantic_features"] is False and out["grid_sp"] == 4 and out["disp_hw"] == 2 and out["lambda_weight"] in (0.75, 1.25)
    assert out["selected_niter"] in (40, 60, 80) and out["selected_smooth"] in (0, 3, 5)
    assert out["winner"] == l2r3.experiment_key("MIND", out["grid_sp"], out["disp_hw"], out["lambda_weight"],
                                                "%d_smoothing%d" % (out["selected_niter"], out["selected_smooth"]))
    # the JSON round-trips and re-ranks to the same winner with the same noise
    with open(os.path.join(str(tmp_path), "phantom", "ablations_phantom.json")) as fh:
        loaded = json.load(fh)
    assert loaded == exp
    rank_all, keys, winner = l2r3.rank_experiments(loaded, noise=noise)
    assert np.array_equal(rank_all, out["rank_all"]) and keys == want_keys and winner == out["winner"]
    # one record recomputed: 80 iterations, smoothing 3, lambda 1.25
    dice = []
    for p in pairs:
        fields = register_pair_snapshots_device(p["fixed"], p["moving"], snapshot_iters=(40, 60, 80), smooths=(0, 3, 5), mind_r=1, mind_d=2,
                                                lambda_weight=1.25, grid_sp=4, disp_hw=2)
        dice.append(sweep.evaluate_item(fields[2, 1], p["seg_fixed"], p["seg_moving"], p["key_fixed"], p["key_moving"], p["num_labels"])["dice"])
    rec = exp[l2r3.experiment_key("MIND", 4, 2, 1.25, "80_smoothing3")]
    assert rec["sim1"] == l2r3.aggregate_cases(dice) and rec["sim1"]["mean"] == float(np.mean(dice))
