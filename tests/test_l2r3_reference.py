"""The restatement of the L2R-2022 ranking (tests/l2r3_restatement.py) against scipy itself and against the reference's own block, whose
results tests/golden/l2r3.npz holds (captured by tests/golden/make_golden_l2r3.py); the library's host-side threshold and the small
helpers of convexadam_amd.l2r3 against the restatement and against literals read off self_configuring/l2r3.py.  No kernel runs here.

rank_all criterion: |delta| <= 1e-12 absolute on every column.  The values lie in [0.1, 1]; the only freedom is the summation order inside
a tie group of rankscore_avgtie (numpy's default argsort is not stable across CPUs), at most (N + 50) 2^-53 = 8e-15, and a few ulp of the
final power.  Observed: 2.2e-16 (with_sim2), 1.1e-16 (four_metrics)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import l2r3_restatement as R  # noqa: E402

SIZES = (1, 2, 3, 5, 18, 64, 108)


def sample_pairs(S, rng):
    """(name, x, y) rows of S values: random, tie-heavy, with infinities"""
    rows = [("normal", rng.standard_normal(S), rng.standard_normal(S) - 0.4),
            ("shifted", rng.standard_normal(S) + 1.5, rng.standard_normal(S)),
            ("ties", rng.integers(0, 4, S).astype(np.float64), rng.integers(0, 4, S).astype(np.float64)),
            ("ties_high", rng.integers(1, 5, S).astype(np.float64), rng.integers(0, 3, S).astype(np.float64)),
            ("equal", np.full(S, 2.5), np.full(S, 2.5))]
    x, y = rng.standard_normal(S), rng.standard_normal(S)
    x[0], y[-1] = np.inf, -np.inf
    rows.append(("inf", x, y))
    rows.append(("inf_both", np.where(np.arange(S) % 2 == 0, np.inf, x), np.where(np.arange(S) % 3 == 0, np.inf, y)))
    return rows


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("S", SIZES)
def test_statistic_and_decision_equal_scipy(S):
    from convexadam_amd.l2r3 import ranksum_statistic
    rng = np.random.default_rng(100 + S)
    crit = R.critical_u2(S)
    for name, x, y in sample_pairs(S, rng):
        u2 = int(R.u2_brute(np.stack([x, y])[None])[0, 0, 1])
        ref = scipy.stats.ranksums(x, y)
        z = R.statistic(u2, S)
        assert z == ref.statistic and ranksum_statistic(u2, S) == ref.statistic, (name, S, u2, z, ref.statistic)
        assert (u2 >= crit) == bool((ref.statistic > 0) & (ref.pvalue < 0.05)), (name, S, u2, crit, ref)
    assert ranksum_statistic(np.arange(4), S).shape == (4,)


def test_critical_u2_against_a_scan_with_scipys_p_value():
    """for every S in 2..256: the first U2 above S^2 whose 2 norm.sf(|z|) is below 0.05 is the restatement's threshold -- zero disagreements"""
    wrong = []
    for S in range(2, 257):
        u2 = np.arange(S * S + 1, 2 * S * S + 1)
        z = R.statistic(u2, S)
        ok = (z > 0) & (2 * scipy.stats.norm.sf(np.abs(z)) < 0.05)
        first = int(u2[np.argmax(ok)]) if ok.any() else 2 * S * S + 1
        assert not ok.any() or ok[np.argmax(ok):].all()               # the significant values are one upper stretch
        if first != R.critical_u2(S):
            wrong.append((S, first, R.critical_u2(S)))
    assert wrong == []
    assert R.critical_u2(2) == 9 and R.critical_u2(1) == 3          # S = 1 and S = 2: no attainable significance


def test_library_threshold_equals_the_restatement(L):
    from convexadam_amd.l2r3 import critical_u2
    out = C.c_int(-1)
    for p in (0.01, 0.05, 0.5):
        for S in range(1, 257):
            assert L.cvx_ranksum_critical_u2(S, p, C.byref(out)) == 0
            assert out.value == R.critical_u2(S, p), (S, p, out.value)
    assert critical_u2(108) == R.critical_u2(108) and critical_u2(18, 0.01) == R.critical_u2(18, 0.01)
    assert L.cvx_ranksum_critical_u2(4096, 0.05, C.byref(out)) == 0 and 4096 ** 2 < out.value <= 2 * 4096 ** 2
    z = R.statistic(np.array([out.value - 1, out.value]), 4096)
    assert R.pvalue_erfc(z[0]) >= 0.05 > R.pvalue_erfc(z[1])


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_restatement_rank_all_equals_the_reference(golden, case):
    g = golden("l2r3")
    assert int(g["seed"]) == R.SEED
    data = R.golden_data(g, case)
    assert [k.decode() for k in g[case + "_keys"]] == R.case_keys(case) == R.team_keys(data)
    rank_all, keys, winner = R.rank_all(data, R.golden_noise(case))
    want = g[case + "_rank_all"]
    assert rank_all.shape == want.shape == (18, 6 if case == "with_sim2" else 5)
    worst = np.abs(rank_all - want).max(0)
    print(case, "max |delta| per column", worst)
    assert np.all(worst <= 1e-12), worst
    assert winner == g[case + "_winner"].item().decode()
    assert want.min() >= 0.1 and want.max() <= 1.0
    for t, col in enumerate(("sim1_mean", "sim1_30", "smooth", "time", "sim2")):          # the golden's columns are the generator's
        assert np.array_equal(g["%s_%s" % (case, col)], R.synthetic_means(case)[col])


def test_restatement_scores_better_equals_the_reference(golden):
    g = golden("l2r3")
    for case in R.CASES:
        assert np.array_equal(R.scores_better(R.first_noisy_subset(g, case)), g[case + "_first_scores"])
    assert np.array_equal(R.scores_better(g["ties_subset"]), g["ties_scores"]) and g["ties_scores"].max() > 0
    assert np.array_equal(R.scores_better(g["nan_subset"]), g["nan_scores"])
    assert np.all(np.isnan(g["nan_subset"][5])) and g["nan_scores"][5] == 0


def test_host_helpers_equal_the_restatement():
    from convexadam_amd import l2r3
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 18, 108):
        for hi in (1, 3, n):
            s = rng.integers(0, min(hi, n) + 1, n)                       # scores 0..N: -N indexes slot 0, as -0 does
            got, want = l2r3.rankscore_avgtie(-s.astype(np.int64)), R.rankscore_avgtie(-s.astype(np.int64))
            assert got.dtype == np.float64 and np.array_equal(got, want), (n, hi)
            assert np.array_equal(l2r3.greaters(s), R.greaters(s))
    # ties share the average of the rank scores their places hold: scores (2, 0, 2, 1) -> -scores sorted: teams 0, 2 | 3 | 1
    assert np.allclose(l2r3.rankscore_avgtie(np.array([-2, 0, -2, -1])), [0.25, 1.0, 0.25, 0.7], rtol=0, atol=1e-15)
    assert list(l2r3.greaters(np.array([3.0, 1.0, 3.0, 2.0]))) == [2, 0, 2, 1]
    with pytest.raises(IndexError):
        l2r3.rankscore_avgtie(np.array([0, -3]))


def test_literals_of_the_reference():
    from convexadam_amd import convexAdam_hyper_util as HU
    from convexadam_amd import l2r3
    for name in ("SAVE_PATHS", "aggregate_cases", "critical_u2", "experiment_key", "greaters", "mind_parameters", "options_for", "parse_winner",
                 "rank_experiments", "rankscore_avgtie", "ranksum_better", "ranksum_statistic", "scores_better", "self_configure"):
        assert getattr(HU, name) is getattr(l2r3, name)
    assert l2r3.SAVE_PATHS == ["40_smoothing0", "60_smoothing0", "80_smoothing0", "40_smoothing3", "60_smoothing3", "80_smoothing3",
                               "40_smoothing5", "60_smoothing5", "80_smoothing5"]                                             # :22
    assert l2r3.experiment_key("MIND", 6, 4, 0.75, "40_smoothing3") == "MIND; gs=6; disp_hwd=4; lambda=0.75; 40_smoothing3"     # :123
    assert l2r3.experiment_key("nnUNet", 4, 2, 1.0, "80_smoothing5") == "nnUNet; gs=4; disp_hwd=2; lambda=1.0; 80_smoothing5"   # :181
    with pytest.raises(ValueError):
        l2r3.experiment_key("mind", 4, 2, 1.0, "80_smoothing5")
    assert l2r3.options_for((192, 192, 208)) == dict(grid_sp=[6], disp_hw=[6, 4], lambda_weight=[0.75, 1.0, 1.25])             # :56-71
    assert l2r3.options_for((100, 100, 100)) == dict(grid_sp=[4], disp_hw=[4, 2], lambda_weight=[0.75, 1.0, 1.25])             # 10^6: not above
    assert l2r3.options_for((101, 100, 100))["grid_sp"] == [6]
    assert l2r3.mind_parameters("MR", "CT") == (1, 2) and l2r3.mind_parameters("MR", "US") == (3, 3)                           # :97-102
    assert l2r3.mind_parameters("US", "US") == (3, 3) and l2r3.mind_parameters("CT", "CT") == (1, 2)
    assert l2r3.parse_winner("nnUNet; gs=6; disp_hwd=4; lambda=1.25; 60_smoothing5") == dict(
        semantic_features=True, grid_sp=6, disp_hw=4, lambda_weight=1.25, selected_niter=60, selected_smooth=5)                # :363-374
    assert l2r3.parse_winner("MIND; gs=4; disp_hwd=2; lambda=0.75; 40_smoothing0") == dict(
        semantic_features=False, grid_sp=4, disp_hw=2, lambda_weight=0.75, selected_niter=40, selected_smooth=0)
    assert l2r3.parse_winner("MIND; gs=12; disp_hwd=10; lambda=1.0; 80_smoothing3")["grid_sp"] == 2                            # the last character only
    for case in R.CASES:                                          # every key the golden cases use is one experiment_key builds
        kinds, gs, hw, lams, _ = R.CASES[case]
        assert R.case_keys(case) == [l2r3.experiment_key(k, gs, hw, lam, sp) for lam in lams for k in kinds for sp in l2r3.SAVE_PATHS]
    agg = l2r3.aggregate_cases([0.5, 0.7, 0.9, 0.3])
    assert agg == {"mean": float(np.mean([0.5, 0.7, 0.9, 0.3])), "std": float(np.std([0.5, 0.7, 0.9, 0.3])), "30": float(np.quantile([0.5, 0.7, 0.9, 0.3], 0.3))}
