"""numpy float64 restatement of the arithmetic contract of csrc/affine.hip (include/convexadam_affine.h) and the shared inputs
of the affine tests.  Test infrastructure only: the product never imports it.

field()   the float64 sequence of affine_core.h::affine_field_voxel on all voxels at once, operation for operation: numpy's float64
          multiplies, adds and divisions are the IEEE operations the header writes, so the result is the kernel's bit for bit.
fit64()   the solution of one fit's equation in float64 through numpy.linalg (solve on the normal equations the kernel forms, and lstsq
          as a second opinion for normal = 0); lts64() the whole trimmed loop.  The kernel sums its moments in another order and solves
          by its own elimination, so these agree with it to rounding, not bit for bit: x_bound() states how far.
"""
import functools

import numpy as np

EPS64 = 2.0 ** -53


def field(theta, shape, u=None):
    """restatement of cvx_affine_field_f64: theta (3, 4) or (4, 4) float32, shape (H, W, D), u None or (H, W, D, 3) float32 / float64
    -> (H, W, D, 3) float64 (cast with .astype for a float output)"""
    th = np.asarray(theta, np.float32).reshape(-1, 4)[:3].astype(np.float64)
    H, W, D = shape
    S = [np.float64(H), np.float64(W), np.float64(D)]
    x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        n = []
        for a in range(3):
            p = x[a] + np.asarray(u)[..., a].astype(np.float64) if u is not None else x[a]
            n.append((2.0 * p + 1.0) / S[a] - 1.0)
        out = []
        for a in range(3):
            r = 2 - a
            g = ((th[r, 0] * n[2] + th[r, 1] * n[1]) + th[r, 2] * n[0]) + th[r, 3]
            out.append(((g + 1.0) * S[a] - 1.0) * 0.5 - x[a])
    return np.ascontiguousarray(np.stack(out, -1))


def identity_bound(shape):
    """theta = identity returns u within this: n = (2 p + 1) / S - 1 carries at most three roundings of values below 2 (3 * 2^-53), which
    (n + 1) S turns into 3 S 2^-53; that product, the -1 and the final subtraction round once more each, at magnitude <= 2 S, i.e.
    2 S 2^-53 each.  3 + 3 * 2 = 9 <= 16 halves of an ulp of S."""
    return 16.0 * max(shape) * EPS64


def homogeneous(p):
    """(N, 3) -> (N, 4) with the ones column; (N, k >= 4) -> its first four columns"""
    p = np.asarray(p, np.float64)
    return np.c_[p[:, :3], np.ones(p.shape[0])] if p.shape[1] == 3 else p[:, :4]


def system(F, M, normal):
    """(A, B) of one fit's equation A X = B over the rows F, M (float64, (n, 4))"""
    L = M if normal else F
    return L.T @ F, L.T @ M


def fit64(F, M, normal):
    """-> (X (4, 4) float64, condition number of the system matrix).  normal = 0: the last column is exactly (0, 0, 0, 1)."""
    F, M = homogeneous(F), homogeneous(M)
    A, B = system(F, M, normal)
    X = np.linalg.solve(A, B) if normal else np.c_[np.linalg.solve(A, B[:, :3]), [0.0, 0.0, 0.0, 1.0]]      # (column 3 of M is not read)
    return X, float(np.linalg.cond(A))


def resid64(X, F, M):
    return np.sqrt(((homogeneous(M) - homogeneous(F) @ X) ** 2).sum(1))


def lts64(F, M, iters, normal):
    idx = np.arange(F.shape[0])
    for _ in range(iters):
        X, _ = fit64(F[idx], M[idx], normal)
        idx = np.argsort(resid64(X, F, M), kind="stable")[:F.shape[0] // 2]
    return X


def x_bound(X64, cond):
    """How far a float32 X may lie from the float64 solution X64 of a system of condition number `cond`, per element: one float32 ulp of the
    element (the kernel rounds its float64 solution once: half an ulp; a float64 solution that differs in its last bits may round to the
    neighbour: one ulp), plus the error of a backward-stable float64 solve of a 4 x 4 system, for the kernel's solution and for numpy's:
    2 * 8 * cond * 2^-53 of the largest element."""
    X64 = np.asarray(X64, np.float64)
    return np.spacing(np.abs(X64).astype(np.float32)).astype(np.float64) + 16.0 * cond * EPS64 * np.abs(X64).max()


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
X_TRUE = np.array([[1.06, 0.03, -0.02, 0.0], [-0.04, 0.95, 0.05, 0.0], [0.02, -0.03, 1.0, 0.0], [0.05, -0.08, 0.03, 1.0]])


@functools.lru_cache(maxsize=None)
def points(n, seed=0, noise=1e-3, outliers=0.0, ld=4):
    """(fixed, moving) float32, (n, ld): coordinates uniform in [-1, 1]^3, moving = fixed X_TRUE + noise; the first `outliers` share of a
    random permutation is moved by up to half the extent.  Columns beyond the fourth (ld > 4) hold NaN: nothing may read them."""
    g = np.random.default_rng(1000 * seed + n)
    f = np.c_[g.uniform(-1.0, 1.0, (n, 3)), np.ones(n)]
    m = f @ X_TRUE
    m[:, :3] += noise * g.standard_normal((n, 3))
    bad = g.permutation(n)[:int(round(outliers * n))]
    m[bad, :3] += g.uniform(0.25, 0.5, (bad.size, 3)) * g.choice([-1.0, 1.0], (bad.size, 3))
    good = np.ones(n, bool)
    good[bad] = False
    pad = np.full((n, max(ld - 4, 0)), np.nan)
    f, m = np.c_[f, pad][:, :ld].astype(np.float32), np.c_[m, pad][:, :ld].astype(np.float32)
    for a in (f, m, good):
        a.setflags(write=False)
    return f, m, good


FIELD_SHAPES = ((1, 1, 1), (2, 3, 5), (7, 1, 9), (33, 17, 65))
THETA = np.array([[1.05, 0.04, -0.03, 0.02], [-0.02, 0.96, 0.05, -0.04], [0.03, -0.01, 1.02, 0.01]], np.float32)


@functools.lru_cache(maxsize=None)
def smooth_field(shape, seed=3):
    """a displacement field of a few voxels with an irrational look: (H, W, D, 3) float64, read-only"""
    g = np.random.default_rng(seed)
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)
    ph = g.uniform(0.0, 6.0, (3, 3))
    u = np.stack([2.5 * np.sin(0.31 * x[..., 0] + ph[a, 0]) * np.cos(0.23 * x[..., 1] + ph[a, 1]) + 0.7 * np.sin(0.17 * x[..., 2] + ph[a, 2])
                  for a in range(3)], -1)
    u.setflags(write=False)
    return u


def layouts(f, dtype, planar):
    """a (H, W, D, 3) array as the contiguous array of one layout and element type"""
    f = np.asarray(f).astype(dtype)
    return np.ascontiguousarray(np.moveaxis(f, -1, 0)) if planar else np.ascontiguousarray(f)
