"""numpy restatement of convexadam_amd/csrc/softstats_core.h: the soft reading of a cost volume, per coarse cell the
Boltzmann-weighted mean displacement, its covariance, the partition sum and the mean excess energy.

A plain module that test files import (like fieldops_restatement.py).  Every float32 operation is a numpy float32 operation, every sum an
explicit loop over k in the header's order -- one D-shift plane (chunk) after the other, each from 0.0, the chunk sums then added in dD
order from 0.0 -- because numpy's own pairwise sum would break that order.  The cells are the vector axis.  The exponential is oracle.expf,
the C oracle's statement of the library's expf.  Also here: the cases the host program and the device are held to, and an independent
float64 evaluation with the error bound derived in reference_bound()."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

F = np.float32
QNAN = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]


def deltas(hw):
    """(K, 3) integer displacements in k order: k = (dD + hw) n^2 + (dW + hw) n + (dH + hw) -> (dH, dW, dD)"""
    r = np.arange(-hw, hw + 1)
    dD, dW, dH = np.meshgrid(r, r, r, indexing="ij")
    return np.stack([dH.ravel(), dW.ravel(), dD.ravel()], 1)


def energies(ssd, hw, field=None, coupling=0.0):
    """(K, V) float32 entry energies"""
    K = (2 * hw + 1) ** 3
    e = np.ascontiguousarray(ssd).reshape(K, -1).astype(F)            # a half is widened exactly
    if field is None:
        return e
    u = np.ascontiguousarray(field, F).reshape(3, -1)
    c = F(coupling)
    out = np.empty_like(e)
    with np.errstate(all="ignore"):
        for k, (d0, d1, d2) in enumerate(deltas(hw)):
            a, b, g = F(d0) - u[0], F(d1) - u[1], F(d2) - u[2]
            q = (a * a + b * b) + g * g
            out[k] = e[k] + c * q
    return out


def soft_stats(ssd, hw, beta, field=None, coupling=0.0):
    """-> (out (12,) + ssd.shape[1:] float32, number of non-finite columns)"""
    n = 2 * hw + 1
    grid = tuple(ssd.shape[1:])
    e = energies(ssd, hw, field, coupling)
    K, V = e.shape
    assert K == n ** 3
    D = deltas(hw).astype(np.float64)
    beta = F(beta)
    m = np.full(V, np.inf, F)
    for k in range(K):                                                 # pass A: the NaN-keeping min
        m = np.where((e[k] < m) | (e[k] != e[k]), e[k], m)
    total = np.zeros((11, V))
    with np.errstate(all="ignore"):
        for c in range(n):                                             # pass B, chunk by chunk
            s = np.zeros((11, V))
            for k in range(c * n * n, (c + 1) * n * n):
                r = e[k] - m
                t = -(beta * r)
                kept = t >= F(-104.0)
                w = np.where(kept, oracle.expf(np.where(kept, t, F(0.0)).astype(F)), F(0.0)).astype(np.float64)
                r64 = np.where(kept, r, F(0.0)).astype(np.float64)
                d0, d1, d2 = D[k]
                a0, a1, a2 = w * d0, w * d1, w * d2
                s[0] += w
                s[1] += a0
                s[2] += a1
                s[3] += a2
                s[4] += a0 * d0
                s[5] += a0 * d1
                s[6] += a0 * d2
                s[7] += a1 * d1
                s[8] += a1 * d2
                s[9] += a2 * d2
                s[10] += w * r64
            total += s
        Z = total[0]
        mean = total[1:4] / Z
        out = np.empty((12, V), F)
        out[0:3] = mean.astype(F)
        i = 4
        for a in range(3):
            for b in range(a, 3):
                cov = total[i] / Z - mean[a] * mean[b]
                if a == b:
                    cov = np.where(cov < 0.0, 0.0, cov)
                out[i - 1] = cov.astype(F)
                i += 1
        out[9] = Z.astype(F)
        out[10] = (total[10] / Z).astype(F)
        out[11] = m
    bad = ~np.isfinite(m)
    out[:, bad] = QNAN
    return out.reshape((12,) + grid), int(bad.sum())


def entropy(out, beta):
    """ln Z + beta E / Z in float64 from the stored float32 channels (what soft_entropy computes)"""
    return np.log(out[9].astype(np.float64)) + float(F(beta)) * out[10].astype(np.float64)


# ---- an independent float64 evaluation and its bound ------------------------------------------------------------------------------------
def reference64(ssd, hw, beta, field=None, coupling=0.0):
    """The same quantities from the float32 ENERGIES (the contract's e_k, so that the comparison isolates the weights and the sums) with
    float64 exponentials, numpy's own sums and no dropping: (mean (3, V), cov (6, V), Z, excess)."""
    e = energies(ssd, hw, field, coupling).astype(np.float64)
    r = e - e.min(0)
    w = np.exp(-float(F(beta)) * r)
    r = np.where(np.isfinite(r), r, 0.0)
    D = deltas(hw).astype(np.float64)
    Z = w.sum(0)
    mean = (w[:, None, :] * D[:, :, None]).sum(0) / Z
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    cov = np.stack([(w * (D[:, a] * D[:, b])[:, None]).sum(0) / Z - mean[a] * mean[b] for a, b in pairs])
    return mean, cov, Z, (w * r).sum(0) / Z


def reference_bound(hw, beta, K):
    """The derived bounds on |restatement - reference64|, before the output cast (absolute for mean, cov and excess, relative for Z); the
    caller adds CAST = 2^-24 times the reference value's magnitude for the one rounding to float32.

      Weights.  A kept weight is w_k = expf(t_k) with t_k = -(beta * r_k), r_k = e_k - m, in float32.  The subtraction and the product
      are each rounded once, 2^-24 relative each, so t_k is off by at most 2^-23 |t_k| <= 104 * 2^-23 in absolute terms, and that is the
      relative change of its exponential; expf itself is within one ulp, 2^-23 relative.  With another 2^-23 for the second-order terms:
          eps = 104 * 2^-23 + 2^-22 ~ 1.27e-5      relative error of every kept weight.
      A weight below 2^-126 (t < -87.3) is a denormal float: it is off by up to 2^-149 in absolute terms instead; an entry dropped for
      t < -104 is missing with at most e^-104.  Both are counted against Z >= 1:  tail = K (e^-104 + 2^-149), below 1e-41 here.
      The float64 sums contribute K 2^-53, which no bound below can see.
      Averages.  With weights w_k (1 + eta_k), |eta_k| <= eps, the average of f moves by  sum w_k eta_k (f_k - E f) / sum w_k (1 + eta_k),
      at most eps (1 + eps) E|f - E f|, and E|f - E f| <= sqrt(var f) <= max|f|.
          mean_a    f = delta_a, |f| <= hw                       -> hw eps (1 + eps), inside  2 hw eps
          cov_ab    about the unperturbed mean mu (a covariance does not depend on the origin): f = (delta_a - mu_a)(delta_b - mu_b),
                    E|f - E f| <= 2 E|f| <= 2 sqrt(var_a var_b) <= 2 hw^2, and the product of the two mean shifts is of order eps^2
                                                                 -> 2 hw^2 eps + O(eps^2), inside  4 hw^2 eps
          Z         a sum of positive terms                      -> eps relative
          excess    f = r_k in [0, 104 / beta] over kept entries -> inside  2 eps * 104 / beta"""
    eps = 104 * 2.0 ** -23 + 2.0 ** -22
    tail = K * (np.exp(-104.0) + 2.0 ** -149)
    return dict(mean=2 * hw * eps + hw * tail, cov=4 * hw * hw * eps + hw * hw * tail, Z=eps + tail, excess=2 * eps * 104 / beta + (104 / beta) * tail)


CAST = 2.0 ** -24


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
GRIDS = ((1, 1, 1), (3, 5, 7), (2, 3, 67), (4, 9, 33))
HWS = (0, 1, 2, 3, 5)


def random_volume(hw, grid, seed, half=False):
    """a volume like correlate's: non-negative costs with a smooth bowl around a per-cell centre plus noise"""
    rng = np.random.default_rng(seed)
    K, V = (2 * hw + 1) ** 3, int(np.prod(grid))
    c = rng.uniform(-hw, hw, (3, V)) * 0.6
    D = deltas(hw).astype(np.float64)
    bowl = ((D[:, :, None] - c[None]) ** 2).sum(1) * rng.uniform(0.02, 0.3, V)
    v = (bowl + rng.uniform(0.0, 0.5, (K, V))).astype(F)
    v = v.reshape((K,) + tuple(grid))
    return v.astype(np.float16) if half else v


def random_field(hw, grid, seed):
    rng = np.random.default_rng(seed + 1000)
    return (rng.uniform(-1.0, 1.0, (3,) + tuple(grid)) * max(hw, 1) * 0.7).astype(F)


def beta_for(half):
    return 6.0 if half else 9.5


def bit_cases():
    """(name, ssd, hw, beta, field, coupling): every hw x grid x {float32, float16} x {no field, field}"""
    out = []
    for hw in HWS:
        for gi, grid in enumerate(GRIDS):
            for half in (False, True):
                for with_field in (False, True):
                    seed = 100 * hw + 10 * gi + 2 * half + with_field
                    ssd = random_volume(hw, grid, seed, half)
                    field = random_field(hw, grid, seed) if with_field else None
                    out.append(("hw%d-%s-%s-%s" % (hw, "x".join(map(str, grid)), "f16" if half else "f32", "field" if with_field else "data"),
                                ssd, hw, beta_for(half), field, (1.0 if gi % 2 else 0.25) if with_field else 0.0))
    return out


def flat_column(hw, grid=(1, 1, 1), value=3.25):
    return np.full(((2 * hw + 1) ** 3,) + grid, value, F)


def spike_column(hw, beta, k, grid=(1, 1, 1)):
    """one entry 0 and all others >= 105 / beta"""
    v = np.full(((2 * hw + 1) ** 3,) + grid, F(106.0) / F(beta), F) + np.arange((2 * hw + 1) ** 3, dtype=F).reshape((-1,) + (1,) * len(grid))
    v[k] = 0.0
    return v


def poisoned(hw=2, grid=(3, 5, 7), half=False):
    """a volume with a planted NaN, an all-Inf column and a -Inf -> (ssd, the three flat cell indices)"""
    ssd = random_volume(hw, grid, 321, half).copy()
    flat = ssd.reshape(ssd.shape[0], -1)
    cells = (5, 41, 77)
    flat[17, cells[0]] = np.nan
    flat[:, cells[1]] = np.inf
    flat[3, cells[2]] = -np.inf
    return ssd, cells


def half_with_inf(hw=2, grid=(3, 5, 7)):
    """a float16 volume whose costs overflow half's range in places: +Inf entries beside finite ones in most columns"""
    v = random_volume(hw, grid, 55).astype(np.float64) * 9000.0
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    assert np.isinf(h).any() and np.isfinite(h.reshape(h.shape[0], -1).min(0)).all()
    return h
