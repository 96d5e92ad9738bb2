"""Goldens for the ranking that ends the L2R-2022 self-configuration, captured by EXECUTING the reference's own statements (run ONLY
where the reference tree is present; about 90 s of scipy.stats.ranksums):

    python tests/golden/make_golden_l2r3.py        # -> tests/golden/l2r3.npz

self_configuring/l2r3.py imports the four registration mains and reads a challenge directory, so sc_convex_adam cannot be called; the
statements of its body on lines 227..361 -- the three nested helpers and the ranking block -- are lifted out of the parsed file with `ast`,
compiled as they stand and executed in a namespace that supplies `data`, `np`, `torch`, `scipy` and a silent `print`.  No reference text
is stored.

Two made-up ablations of N = 18 teams (tests/l2r3_restatement.py: CASES, synthetic_means), np.random.seed(11) before each block:
  with_sim2      MIND x gs 6 x hw 6 x lambda {0.75, 1.25} x 9 folders, sim1 = DSC, sim2 = HD95       five metric blocks
  four_metrics   MIND and nnUNet x gs 4 x hw 4 x lambda 1.0 x 9 folders, no sim2 key                  four metric blocks
Stored per case: the per-team columns, rank_all, the team keys (fixed-width bytes), the winner key; the seed; and the lifted
scores_better's output on four (18, S) subsets: the first noisy subset of each case (regenerated from the seed by the tests), one of
integers out of {0..3} and one with a NaN team (both stored).  The noise is not stored: np.random.seed(11) regenerates it.
"""
import ast
import os
import sys

import numpy as np
import scipy.stats
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_import import REF_ROOT  # noqa: E402
import l2r3_restatement as R  # noqa: E402

SCRIPT = os.path.join("self_configuring", "l2r3.py")
FIRST, LAST = 227, 361


def run_block(data):
    tree = ast.parse(open(os.path.join(REF_ROOT, SCRIPT)).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "sc_convex_adam"][0]
    body = [s for s in fn.body if FIRST <= s.lineno <= LAST]
    assert len(body) == 45, len(body)
    ns = dict(data=data, np=np, torch=torch, scipy=scipy, print=lambda *a, **k: None)
    exec(compile(ast.Module(body=body, type_ignores=[]), SCRIPT, "exec"), ns)
    return ns


def main():
    out = {"seed": np.array(R.SEED)}
    rng = np.random.RandomState(2022)
    ties = rng.randint(0, 4, size=(18, 12)).astype(np.float64)
    with_nan = rng.randn(18, 18) + 0.15 * np.arange(18)[:, None]
    with_nan[5] = np.nan
    out["ties_subset"], out["nan_subset"] = ties, with_nan
    for case in R.CASES:
        cols = R.synthetic_means(case)
        data = R.data_of(case, cols)
        np.random.seed(R.SEED)
        ns = run_block(data)
        assert ns["keys_team"] == R.case_keys(case) and ns["N"] == 18
        for c, v in cols.items():
            out["%s_%s" % (case, c)] = v
        out[case + "_rank_all"] = ns["rank_all"]
        out[case + "_keys"] = np.array(ns["keys_team"], dtype="S")
        out[case + "_winner"] = np.array(ns["winner_key"], dtype="S")
        final = np.sort(ns["rank_all"][:, -1])
        print(case, "winner", ns["winner_key"], "margin over the runner-up %.3f" % (final[-1] - final[-2]), flush=True)
        g = {k: v for k, v in out.items()}
        out[case + "_first_scores"] = ns["scores_better"](R.first_noisy_subset(g, case))
        if case == "with_sim2":
            with np.errstate(invalid="ignore"):
                out["ties_scores"] = ns["scores_better"](ties)
                out["nan_scores"] = ns["scores_better"](with_nan)
    path = os.path.join(HERE, "l2r3.npz")
    np.savez_compressed(path, **out)
    print("wrote l2r3.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
