"""numpy float64 restatement of the arithmetic contract of csrc/fieldops.hip (include/convexadam_field.h) and the shared
inputs of the field-operator tests.  Test infrastructure only: the product never imports it.

The restatement runs the float64 sequence of fieldops_core.h on all voxels at once: v = -u, then v <- -taps(u, clamp(y + v)) on the voxels
that are still iterating, then the residual.  The taps go through scipy.ndimage.map_coordinates(order=1, mode='nearest') on the clamped
coordinate, the same eight-tap sum as taps_linear_f64 (geometry_restatement.py does the same).  Clamp, the NaN-keeping max and the
finiteness test are written as in the header: where(r < 0, 0, r), where(r > n - 1, n - 1, r); m = where(d > m or d != d, d, m).
"""
import functools

import numpy as np
from scipy.ndimage import gaussian_filter, map_coordinates

DBL_MAX = np.finfo(np.float64).max
EPS = 2.0 ** -52

SMOOTH_SHAPES = ((12, 10, 14), (7, 9, 11), (5, 4, 131), (1, 6, 9), (3, 3, 3), (1, 1, 1), (6, 7, 70))
# the last shape: every extent exceeds the kernels' workgroup footprint (a brick of 4 x 4 x 16 voxels) by a non-multiple, the last one
# also the 64 of the row footprint that was measured against it; sigma is 2.0, 1.5, 1.5, 1.5, 1.0 for the first five shapes, 1.0 for the
# single voxel and 2.0 for the last shape
SMOOTH_SIGMAS = (2.0, 1.5, 1.5, 1.5, 1.0, 1.0, 2.0)
SMOOTH_OFFSET = (2.3, -1.6, 0.9)
FOLDED_SHAPE = (6, 5, 16)
AFFINE_SHAPE = (16, 14, 18)
AFFINE_T = (0.7, -0.4, 0.3)


def _grid(shape):
    """(3, N) float64 voxel indices, axis 0 slowest"""
    return np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), 0).reshape(3, -1)


def _nanmax(m, d):
    return np.where((d > m) | (d != d), d, m)


def _clamp(r, hi):
    """r (3, n) -> (finite (n,), clamped coordinates of the finite columns (3, n_finite))"""
    fin = np.all((r >= -DBL_MAX) & (r <= DBL_MAX), axis=0)
    r = r[:, fin]
    r = np.where(r < 0.0, 0.0, r)
    r = np.where(r > hi, hi, r)
    return fin, r


def _taps(f64, c):
    """f64 (H, W, D, 3) float64, c (3, n) clamped -> (3, n)"""
    if c.shape[1] == 0:
        return np.zeros((3, 0), np.float64)
    return np.stack([map_coordinates(f64[..., a], c, order=1, mode="nearest") for a in range(3)], 0)


def invert(u, max_iters=50, tol=1e-4):
    """restatement of cvx_field_invert_f64.  u (H, W, D, 3), float32 or float64 -> dict: v (H, W, D, 3) float64 (cast with .astype for a
    float output), residual (H, W, D) float64, iters (H, W, D) uint8, stats int64[3] = not converged, non-finite, bits of the largest
    finite residual"""
    u = np.asarray(u)
    shape = u.shape[:3]
    u64 = u.astype(np.float64)
    y = _grid(shape)
    N = y.shape[1]
    hi = np.array(shape, np.float64).reshape(3, 1) - 1.0
    v = -(u64.reshape(N, 3).T.copy())
    it = np.zeros(N, np.int64)
    met = np.zeros(N, bool)
    finite = np.ones(N, bool)
    active = np.arange(N)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, max_iters + 1):
            if active.size == 0:
                break
            it[active] = k
            fin, c = _clamp(y[:, active] + v[:, active], hi)
            finite[active[~fin]] = False
            active = active[fin]
            vn = -_taps(u64, c)
            d = np.abs(vn - v[:, active])
            step = np.zeros(active.size)
            for a in range(3):
                step = _nanmax(step, d[a])
            v[:, active] = vn
            if tol > 0.0:
                done = step <= tol
                met[active[done]] = True
                active = active[~done]
        idx = np.nonzero(finite)[0]
        fin, c = _clamp(y[:, idx] + v[:, idx], hi)
        finite[idx[~fin]] = False
        idx = idx[fin]
        d = np.abs(v[:, idx] + _taps(u64, c))
        r = np.zeros(idx.size)
        for a in range(3):
            r = _nanmax(r, d[a])
        finite[idx[~(r <= DBL_MAX)]] = False
    residual = np.full(N, np.nan)
    residual[idx] = r
    residual[~finite] = np.nan
    v[:, ~finite] = np.nan
    stats = np.zeros(3, np.int64)
    stats[0] = int((finite & ~met).sum()) if tol > 0.0 else 0
    stats[1] = int((~finite).sum())
    if finite.any():
        stats[2] = residual[finite].view(np.int64).max()
    return dict(v=np.ascontiguousarray(v.T).reshape(shape + (3,)), residual=residual.reshape(shape),
                iters=np.minimum(it, 255).astype(np.uint8).reshape(shape), stats=stats)


def compose(a, b):
    """restatement of cvx_field_compose_f64: out(x) = b(x) + a(clamp(x + b(x))), (H, W, D, 3) float64"""
    a, b = np.asarray(a), np.asarray(b)
    shape = a.shape[:3]
    y = _grid(shape)
    N = y.shape[1]
    hi = np.array(shape, np.float64).reshape(3, 1) - 1.0
    bv = b.astype(np.float64).reshape(N, 3).T
    out = np.full((3, N), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        fin, c = _clamp(y + bv, hi)
        out[:, fin] = bv[:, fin] + _taps(a.astype(np.float64), c)
    return np.ascontiguousarray(out.T).reshape(shape + (3,))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs():
    g = np.random.default_rng(5)
    smooth = []
    for shape, sigma in zip(SMOOTH_SHAPES, SMOOTH_SIGMAS):
        f = np.stack([gaussian_filter(g.standard_normal(shape), sigma) for _ in range(3)], -1)
        steps = [float(np.abs(np.diff(f, axis=ax)).max()) for ax in range(3) if shape[ax] > 1]
        if steps and max(steps) > 0.0:
            f = f * (0.25 / max(steps))
        f = f + np.array(SMOOTH_OFFSET)
        f.setflags(write=False)
        smooth.append(f)
    A = np.eye(3) + 0.08 * g.standard_normal((3, 3))
    return tuple(smooth), A


def smooth_set():
    """the seven smooth fields (read-only float64): neighbour differences of at most 0.25 voxel, shifted by (2.3, -1.6, 0.9)"""
    return _inputs()[0]


def folded_field():
    """u_2 = -2 (i2 - 7.5) where |i2 - 7.5| < 3: x + u(x) folds over, the iteration cannot converge there"""
    u = np.zeros(FOLDED_SHAPE + (3,), np.float64)
    i2 = np.arange(FOLDED_SHAPE[2], dtype=np.float64) - 7.5
    u[..., 2] = np.where(np.abs(i2) < 3.0, -2.0 * i2, 0.0)
    u.setflags(write=False)
    return u


def affine_field():
    """u = A (x - c) + c + t - x on AFFINE_SHAPE -> (u, true inverse v, inside mask, L = ||A - I||_2): v = inv(A) (y - c - t) + c - y,
    inside = the pre-image y + v(y) lies in the grid"""
    A = _inputs()[1]
    shape = AFFINE_SHAPE
    x = _grid(shape)
    c = (np.array(shape, np.float64).reshape(3, 1) - 1.0) / 2.0
    t = np.array(AFFINE_T).reshape(3, 1)
    u = A @ (x - c) + c + t - x
    v = np.linalg.solve(A, x - c - t) + c - x
    pre = x + v
    inside = np.all((pre >= 0.0) & (pre <= 2.0 * c), axis=0)
    L = float(np.linalg.norm(A - np.eye(3), 2))
    return (np.ascontiguousarray(u.T).reshape(shape + (3,)), np.ascontiguousarray(v.T).reshape(shape + (3,)), inside.reshape(shape), L)


def affine_bound(u, L, k):
    """2 L^k max|u| + 64 eps max extent / (1 - L): the contraction's remainder after k iterations plus the rounding of one evaluation,
    amplified by the fixed point's conditioning"""
    return 2.0 * L ** k * float(np.abs(u).max()) + 64.0 * EPS * max(u.shape[:3]) / (1.0 - L)


def layouts(f, dtype, planar):
    """a (H, W, D, 3) array as the contiguous array of one layout and element type"""
    f = np.asarray(f).astype(dtype)
    return np.ascontiguousarray(np.moveaxis(f, -1, 0)) if planar else np.ascontiguousarray(f)
