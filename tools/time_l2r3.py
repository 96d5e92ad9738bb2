"""Times the parameter selection that ends the L2R-2022 self-configuration (self_configuring/l2r3.py:227-361) at the size of a full
ablation with label features: N = S = 108 teams, five metric blocks of 50 noise draws each -- 250 x 108^2 rank-sum tests of 108 samples a
side, 3.4e10 comparisons.

    python tools/time_l2r3.py [--reps 10] [--small] [--cpu-repeats 2]

Prints, in ms, medians of --reps after two warm-up calls:
  (a) the five launches of cvx_ranksum_better_f64 alone, samples and means resident, bracketed by device events;
  (b) rank_experiments end to end on a host dict and a host noise array (23 MB at full size): upload, launches, download of the scores, the
      host rank scores -- wall clock around a synchronised call;
  (c) the tests' numpy restatement (tests/l2r3_restatement.py: brute-force U2 by broadcasting) on this host's CPU, timed once on
      --cpu-repeats noise draws of one block and scaled to the 250 draws of a run (0 skips it).
Then checks that (b) and the restatement agree on the draws that (c) used.  --small: N = S = 18, for a quick check."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from convexadam_amd import l2r3  # noqa: E402
import l2r3_restatement as R  # noqa: E402


def median_ms(fn, reps, events):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        else:
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cpu-repeats", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, repeats = (18, 50) if args.small else (108, 50)
    rng = np.random.RandomState(0)
    kinds = ("MIND", "nnUNet")
    keys = [l2r3.experiment_key(kinds[t % 2], 6, 6, 0.75 + 0.01 * (t // 18), l2r3.SAVE_PATHS[(t // 2) % 9]) for t in range(N)]
    data = {"metrics": {"smooth": "LogJacDetStd", "sim1": "DSC", "sim2": "HD95"}}
    for k in keys:
        u = rng.rand(5)
        data[k] = {"time": 1.0 + 0.6 * u[3], "sim1": {"mean": 0.55 + 0.3 * u[0], "std": 0.0, "30": 0.35 + 0.3 * u[1]},
                   "smooth": {"mean": 0.05 + 0.3 * u[2], "std": 0.0, "30": 0.0}, "sim2": {"mean": 2.0 + u[4], "std": 0.0, "30": 0.0}}
    assert len(set(keys)) == N
    noise = rng.randn(5, repeats, N, N)
    print("N = S = %d teams, 5 metric blocks x %d repeats: %.3g comparisons, noise %.1f MB" % (N, repeats, 5.0 * repeats * N ** 4, noise.nbytes / 1e6), flush=True)

    blocks = R.blocks_of(data)
    resident = [(torch.from_numpy(noise[b]).to(dev), torch.Tensor(values).to(dev), scale, sign) for b, (values, sign, scale) in enumerate(blocks)]

    def launches():
        for x, m, scale, sign in resident:
            l2r3.ranksum_better(x, m, scale, sign)

    ta = median_ms(launches, args.reps, events=True)
    print("(a) five kernel launches, resident samples (device events): %.3f ms" % ta, flush=True)
    tb = median_ms(lambda: l2r3.rank_experiments(data, noise=noise, repeats=repeats), args.reps, events=False)
    print("(b) rank_experiments end to end (upload, launches, host rank scores; wall clock): %.2f ms" % tb, flush=True)
    if args.cpu_repeats > 0:
        n = min(args.cpu_repeats, repeats)
        values, sign, scale = blocks[0]
        x = np.stack([R.transform(noise[0, r], values, scale, sign) for r in range(n)])
        t = time.perf_counter()
        want = R.scores(R.u2_brute(x), R.critical_u2(N))
        tc = (time.perf_counter() - t) / n
        print("(c) numpy restatement on this host's CPU: %.2f s per noise draw (timed once on %d), %.0f s scaled to the %d draws of a run"
              % (tc, n, tc * 5 * repeats, 5 * repeats), flush=True)
        got = l2r3.ranksum_better(resident[0][0][:n].contiguous(), resident[0][1], scale, sign).cpu().numpy()
        print("scores of those draws equal the restatement's:", bool(np.array_equal(got, want)), flush=True)
    rank_all, _, winner = l2r3.rank_experiments(data, noise=noise, repeats=repeats)
    print("winner:", winner, "| final rank score %.4f" % rank_all[:, -1].max(), flush=True)


if __name__ == "__main__":
    main()
