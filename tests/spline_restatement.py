"""numpy restatement of convexadam_amd/csrc/spline_core.h and the case list of the spline tests.

A plain module that test files import (like simhist_restatement.py).  Every function performs the header's float64 operations in the
header's order, one numpy ufunc per operation, so that the host program (tools/spline_host.cpp) and the kernels (csrc/spline.hip) can be
compared with it bit for bit.  scipy.ndimage (spline_filter, map_coordinates, order=3, mode='constant') evaluates the same mathematics in
another order of operations: the two agree inside SCIPY_BOUND_*, see below."""
import numpy as np

F64 = np.float64
POLE = -0.2679491924311228          # sqrt(3) - 2, SPLINE_POLE
GAIN = (1.0 - POLE) * (1.0 - 1.0 / POLE)
ANTI = POLE / (POLE * POLE - 1.0)

# lengths 1, 2 (empty start loop) and 3; extents that fill no tile; a contiguous line longer than a wavefront and than one staged chunk of
# the contiguous-axis kernel (32 samples: 131 = 4 chunks + 3); strided lines longer than 64
SHAPES = [(1, 1, 1), (1, 4, 5), (4, 1, 5), (4, 5, 1), (2, 3, 4), (3, 3, 3), (5, 6, 7), (9, 8, 12), (3, 5, 131), (67, 3, 5), (3, 67, 5)]
N_RANDOM = 256
MAGNITUDE = 300.0

# max |restatement - scipy| / max |volume| over SHAPES as tests/test_spline_reference.py measures it (scipy 1.15.3, numpy 2.2.6, x86-64):
# two float64 evaluations that differ only in the order of their operations.  The tests' bound is 64 times the figure: the prefilter
# amplifies a rounding by up to 6 per axis and the cases are random -- and it stays far below what a wrong tap, weight or boundary rule
# produces (of the order of the volume's magnitude times 1e-2 and more).
MEASURED_COEF = 1.52e-14
MEASURED_VALUE = 1.91e-15
SCIPY_BOUND_COEF = 64 * MEASURED_COEF
SCIPY_BOUND_VALUE = 64 * MEASURED_VALUE


def volume(shape, seed=0, dtype=np.float64):
    """a random volume of magnitude ~300 without zeros"""
    rng = np.random.default_rng(1000 + seed + 17 * int(np.prod(shape)))
    v = rng.uniform(0.25, 1.0, shape) * rng.choice([-1.0, 1.0], shape) * MAGNITUDE
    return np.ascontiguousarray(v.astype(dtype))


def coordinates(shape, seed=0):
    """(N, 3) float64: 256 random points -- three quarters inside [0, n - 1] on every axis (exactly 0.0 on an axis of length 1), one quarter
    in [-0.7, n - 0.3] -- and the fixed points on top: the corners 0 and n - 1, interior integers, -1e-9, n - 1 + 1e-9, NaN, +-Inf, 1e300."""
    rng = np.random.default_rng(2000 + seed + 31 * int(np.prod(shape)))
    n = np.array(shape, F64)
    inside = rng.uniform(0.0, 1.0, (3 * N_RANDOM // 4, 3)) * (n - 1.0)
    around = -0.7 + rng.uniform(0.0, 1.0, (N_RANDOM - len(inside), 3)) * ((n - 0.3) + 0.7)
    centre = np.floor((n - 1.0) / 2.0)
    fixed = [np.zeros(3), n - 1.0, centre, np.minimum(centre + 1.0, n - 1.0), np.array([0.0, shape[1] - 1.0, 0.0])]
    for a in range(3):
        for bad in (-1e-9, shape[a] - 1 + 1e-9, np.nan, np.inf, -np.inf, 1e300):
            p = centre.copy()
            p[a] = bad
            fixed.append(p)
        p = centre.copy()                       # an integer on one axis, a fraction on the others
        p[(a + 1) % 3] = min(centre[(a + 1) % 3] + 0.5, shape[(a + 1) % 3] - 1.0)
        fixed.append(p)
    return np.ascontiguousarray(np.concatenate([inside, around, np.array(fixed, F64)], 0))


def is_inside(shape, c):
    with np.errstate(invalid="ignore"):
        return np.all((c >= 0.0) & (c <= np.array(shape, F64) - 1.0), axis=1)


def _prefilter_axis(c, axis):
    """spline_prefilter_line on every line of `axis` at once; c float64, a new array"""
    c = np.moveaxis(c, axis, 0).copy()
    n = c.shape[0]
    if n == 1:
        return np.moveaxis(c, 0, axis)
    zn1 = 1.0
    for _ in range(n - 1):
        zn1 *= POLE
    s = c[0] * GAIN + zn1 * (c[n - 1] * GAIN)
    zi = POLE
    for i in range(1, n - 1):
        s = s + zi * (c[i] * GAIN + zn1 * (c[n - 1 - i] * GAIN))
        zi *= POLE
    prev = s / (1.0 - zn1 * zn1)
    before = prev
    c[0] = prev
    for i in range(1, n):
        v = c[i] * GAIN + POLE * prev
        c[i] = v
        before, prev = prev, v
    nxt = ANTI * (prev + POLE * before)
    c[n - 1] = nxt
    for i in range(n - 2, -1, -1):
        nxt = POLE * (nxt - c[i])
        c[i] = nxt
    return np.moveaxis(c, 0, axis)


def prefilter(vol):
    """spline_prefilter_all: float32 or float64 in, float64 coefficients out, axes 0, 1, 2"""
    c = np.asarray(vol).astype(F64)
    assert c.ndim == 3
    with np.errstate(under="ignore"):
        for axis in range(3):
            c = _prefilter_axis(c, axis)
    return np.ascontiguousarray(c)


def weights(t):
    u = 1.0 - t
    w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
    w0 = u * u * u / 6.0
    w3 = 1.0 - w0 - w1 - w2
    return [w0, w1, w2, w3]


def mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    r = np.mod(i, period)
    return np.where(r > n - 1, period - r, r)


def taps(coef, c):
    """taps_cubic_f64 at the (N, 3) coordinates c, all inside [0, n - 1]"""
    f = np.floor(c)
    first = f.astype(np.int64) - 1
    w = [weights(c[:, a] - f[:, a]) for a in range(3)]
    idx = [[mirror(first[:, a] + k, coef.shape[a]) for k in range(4)] for a in range(3)]
    r = np.zeros(len(c), F64)
    for i in range(4):
        for j in range(4):
            for k in range(4):
                r = r + ((coef[idx[0][i], idx[1][j], idx[2][k]] * w[0][i]) * w[1][j]) * w[2][k]
    return r


def map_cubic(coef, c):
    """map_cubic_f64: scipy's mode='constant', cval=0"""
    c = np.asarray(c, F64)
    ok = is_inside(coef.shape, c)
    out = np.zeros(len(c), F64)
    if ok.any():
        out[ok] = taps(coef, c[ok])
    return out


def itk_cubic(coef, c, default=0.0):
    """itk_cubic_f64: inside means -0.5 <= c <= n - 0.5, a coordinate beyond the last sample is clamped onto it"""
    c = np.asarray(c, F64)
    n = np.array(coef.shape, F64)
    with np.errstate(invalid="ignore"):
        ok = np.all((c >= -0.5) & (c <= n - 0.5), axis=1)
    out = np.full(len(c), float(default), F64)
    if ok.any():
        out[ok] = taps(coef, np.minimum(np.maximum(c[ok], 0.0), n - 1.0))
    return out


def warp_coordinates(shape, disp):
    """identity + field as the kernels form it: (double)u + (double)index, per component; disp (H, W, D, 3) -> (V, 3)"""
    grid = np.stack(np.meshgrid(*[np.arange(s, dtype=F64) for s in shape], indexing="ij"), -1)
    return (np.asarray(disp).astype(F64) + grid).reshape(-1, 3)


def field_through(shape, targets, start=0, dtype=np.float64):
    """An (H, W, D, 3) field whose voxel q aims at targets[(start + q) % N]: what lets a warp visit a list of points.  The point the
    warp then samples is warp_coordinates(shape, field), which rounding may move by an ulp from the target."""
    V = int(np.prod(shape))
    t = targets[(start + np.arange(V)) % len(targets)].reshape(shape + (3,))
    grid = np.stack(np.meshgrid(*[np.arange(s, dtype=F64) for s in shape], indexing="ij"), -1)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray((t - grid).astype(dtype))


def index_grid(out_shape, M, t):
    """source coordinates (z, y, x order, (V, 3)) of every voxel of an output grid under the index map of interp_f64.h:
    source (x, y, z) = ((m0 i + m1 j) + m2 k) + t with (i, j, k) the output index in x, y, z order"""
    M, t = np.asarray(M, F64).reshape(3, 3), np.asarray(t, F64)
    k, j, i = [g.reshape(-1) for g in np.meshgrid(*[np.arange(s, dtype=F64) for s in out_shape], indexing="ij")]
    c = [((M[a, 0] * i + M[a, 1] * j) + M[a, 2] * k) + t[a] for a in range(3)]
    return np.stack([c[2], c[1], c[0]], 1)
