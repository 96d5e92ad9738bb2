"""numpy restatement of the preprocessing operators, in the operation order include/convexadam_prep.h states.

A plain module that test files import (like geometry_restatement.py).  Nothing here calls the library; every function follows the header
addition by addition, so that `device == restatement` can be asked bit for bit."""
import numpy as np

THREADS, K = 256, 16
SPAN = THREADS * K


# ---- fixed-order float64 sums ------------------------------------------------------------------------------------------------------
def _tree(acc):
    """acc [..., 256]: s = 128, 64, .., 1: acc[t] += acc[t + s] for t < s; returns acc[..., 0]"""
    acc = acc.copy()
    s = THREADS // 2
    while s >= 1:
        acc[..., :s] = acc[..., :s] + acc[..., s:2 * s]
        s //= 2
    return acc[..., 0]


def ordered_sum(terms):
    """terms: float64 [n], 0.0 where an element does not count (adding +0.0 to an accumulator that started at +0.0 changes nothing).
    span b: thread t adds b S + k 256 + t, k = 0 .. 15; tree; the finish: thread t adds partials t, t + 256, ..; tree."""
    n = terms.shape[0]
    nspans = -(-n // SPAN)
    pad = np.zeros(nspans * SPAN, np.float64)
    pad[:n] = terms
    pad = pad.reshape(nspans, K, THREADS)
    acc = np.zeros((nspans, THREADS), np.float64)
    for k in range(K):
        acc = acc + pad[:, k, :]
    partial = _tree(acc)
    rows = -(-nspans // THREADS)
    p = np.zeros(rows * THREADS, np.float64)
    p[:nspans] = partial
    p = p.reshape(rows, THREADS)
    acc = np.zeros(THREADS, np.float64)
    for r in range(rows):
        acc = acc + p[r]
    return _tree(acc)


def clamp(x, lo, hi):
    """t = x < lo ? lo : x;  t = t > hi ? hi : t   (a NaN stays)"""
    lo, hi = np.float32(lo), np.float32(hi)
    t = np.where(x < lo, lo, x)
    return np.where(t > hi, hi, t).astype(np.float32)


def moments(x, clamp_to=None, positive=False):
    """x float32 [n] -> (count, mean float64, ss float64)"""
    y = np.asarray(x, np.float32).ravel()
    if clamp_to is not None:
        y = clamp(y, *clamp_to)
    inn = (y > 0) if positive else np.ones(y.shape, bool)
    count = int(inn.sum())
    yd = y.astype(np.float64)
    with np.errstate(all="ignore"):
        mean = ordered_sum(np.where(inn, yd, 0.0)) / np.float64(count)
        d = yd - mean
        ss = ordered_sum(np.where(inn, d * d, 0.0))
    return count, mean, ss


def mean_std(count, mean, ss):
    with np.errstate(all="ignore"):
        return np.float32(mean), np.float32(np.sqrt(ss / np.float64(count - 1))) if count > 1 else np.float32(np.nan)


# ---- quantiles ---------------------------------------------------------------------------------------------------------------------
def rank_of(q, n):
    """-> (below, above, weight float32): float32 arithmetic up to 2^24 elements (torch.quantile's), float64 above"""
    q = np.float32(q)
    if n <= 1 << 24:
        rank = np.float32(q * np.float32(n - 1))
        below = np.floor(rank)
        return int(below), int(np.ceil(rank)), np.float32(rank - below)
    rank = np.float64(q) * np.float64(n - 1)
    below = np.floor(rank)
    return int(below), int(np.ceil(rank)), np.float32(rank - below)


def lerp(a, b, w):
    a, b, w = np.float32(a), np.float32(b), np.float32(w)
    with np.errstate(all="ignore"):
        if w < np.float32(0.5):
            return np.float32(a + np.float32(w * np.float32(b - a)))
        return np.float32(b - np.float32(np.float32(b - a) * np.float32(np.float32(1) - w)))


def quantiles(y, qs):
    """y float32 [n] (already clamped) -> [float32]: exact order statistics (-0.0 counts as +0.0), torch's lerp; any NaN -> NaN"""
    y = np.asarray(y, np.float32).ravel()
    if np.isnan(y).any():
        return [np.float32(np.nan) for _ in qs]
    s = np.sort(np.where(y == 0, np.float32(0), y))
    out = []
    for q in qs:
        below, above, w = rank_of(q, s.shape[0])
        out.append(lerp(s[below], s[above], w))
    return out


def stats(x, clamp_to=None, positive=False, qs=None):
    """the parameter block {mean, std, lo, hi} of cvx_prep_stats_f32 as four float32, and (count, mean, ss)"""
    count, mean, ss = moments(x, clamp_to, positive)
    m32, s32 = mean_std(count, mean, ss)
    if qs:
        y = np.asarray(x, np.float32).ravel()
        lo, hi = quantiles(clamp(y, *clamp_to) if clamp_to is not None else y, qs)
    else:
        lo, hi = np.float32(-np.inf), np.float32(np.inf)
    return np.array([m32, s32, lo, hi], np.float32), (count, mean, ss)


# ---- the elementwise step ----------------------------------------------------------------------------------------------------------
def normalise(x, params, mode=0):
    """mode 0: (clamp(x, lo, hi) - mean) / std;  mode 1: x > 0 ? (x - mean) / (std + 1e-8f) : 0   -- float32, true division"""
    x = np.asarray(x, np.float32)
    mean, std, lo, hi = [np.float32(v) for v in params]
    with np.errstate(all="ignore"):
        if mode == 0:
            return ((clamp(x, lo, hi) - mean) / std).astype(np.float32)
        y = (x - mean) / np.float32(std + np.float32(1e-8))
        return np.where(x > 0, y, np.float32(0)).astype(np.float32)


def nnunet_norm(x):
    return normalise(x, stats(x, positive=True)[0], 1)


def nnunet_ct_norm(x):
    return normalise(x, stats(x, clamp_to=(-1000.0, 1500.0), qs=(0.005, 0.995))[0], 0)


def nnunet_norm_props(x, props):
    return normalise(x, [props['mean'], props['sd'], props['percentile_00_5'], props['percentile_99_5']], 0)


# ---- mask, hole filling, box -------------------------------------------------------------------------------------------------------
def _sweep(mask, reached, axis):
    """forward then backward along `axis`: carry = !mask[i] && (carry || reached[i]); reached[i] |= carry.  -> changed"""
    m = np.moveaxis(mask, axis, 0)
    r = np.moveaxis(reached, axis, 0)           # a view: writes land in `reached`
    changed = False
    for order in (range(m.shape[0]), range(m.shape[0] - 1, -1, -1)):
        carry = np.zeros(m.shape[1:], bool)
        for i in order:
            carry = ~m[i] & (carry | r[i])
            new = carry & ~r[i]
            if new.any():
                changed = True
                r[i] |= carry
    return changed


def fill_holes(mask):
    """mask bool, 2-d or 3-d -> (mask | !reached, rounds): the complement seeded on the array faces, swept along every axis until a round
    changes nothing (the last, unchanged round counts)"""
    mask = np.asarray(mask, bool)
    reached = np.zeros(mask.shape, bool)
    for a in range(mask.ndim):
        idx = [slice(None)] * mask.ndim
        for side in (0, -1):
            idx[a] = side
            reached[tuple(idx)] = True
    reached &= ~mask
    rounds = 0
    while True:
        rounds += 1
        assert rounds <= mask.size + 1
        changed = False
        for a in range(mask.ndim):
            changed |= _sweep(mask, reached, a)
        if not changed:
            break
    return mask | ~reached, rounds


def nonzero_mask(data):
    return fill_holes((np.asarray(data) != 0).any(axis=0))


def bbox(mask, outside_value=0):
    c = np.where(np.asarray(mask) != outside_value)
    if c[0].size == 0:
        raise ValueError("empty mask")
    return [[int(c[a].min()), int(c[a].max()) + 1] for a in range(3)]


def crop(image, box):
    return image[box[0][0]:box[0][1], box[1][0]:box[1][1], box[2][0]:box[2][1]]


def serpentine(sealed):
    """a 3 x 11 x 11 solid block whose middle plane holds a one-voxel tunnel winding through every other row; its single entrance on the
    array face is open (the sweeps need several rounds, nothing is a hole) or sealed (the whole tunnel is a hole)"""
    m = np.ones((3, 11, 11), bool)
    for row in range(1, 10, 2):
        m[1, row, 1:10] = False
    for j, row in enumerate(range(2, 9, 2)):
        m[1, row, 9 if j % 2 == 0 else 1] = False
    if not sealed:
        m[1, 0, 1] = False                        # the entrance, on the face y = 0
    return m


# ---- host tables -------------------------------------------------------------------------------------------------------------------
def steps(patch_size, image_size, step_size=0.5):
    out = []
    for p, n in zip(patch_size, image_size):
        num = int(np.ceil((n - p) / (p * step_size))) + 1
        actual = (n - p) / (num - 1) if num > 1 else 0.0          # one window, at 0
        out.append([int(np.round(actual * i)) for i in range(num)])
    return out


def gaussian_table(patch_size, sigma_scale=1.0 / 8):
    """fl(fl(k0[i] k1[j]) k2[k]) in float64, / max, float32, zeros -> smallest non-zero, half"""
    ks = []
    for n in patch_size:
        sigma = n * sigma_scale
        radius = int(4.0 * sigma + 0.5)
        xs = np.arange(-radius, radius + 1)
        phi = np.exp(-0.5 / (sigma * sigma) * xs ** 2)
        phi = phi / phi.sum()
        k = np.zeros(n)
        for i in range(n):
            if abs(i - n // 2) <= radius:
                k[i] = phi[i - n // 2 + radius]
        ks.append(k)
    g = ks[0]
    for k in ks[1:]:
        g = np.multiply.outer(g, k)
    return finish_gaussian(g)


def finish_gaussian(g):
    """the three fix-ups behind the float64 table: / max and float32; zeros -> smallest non-zero value; half, (1, 1, *patch)"""
    g = (np.asarray(g, np.float64) / g.max()).astype(np.float32)
    g[g == 0] = g[g != 0].min()
    return g.astype(np.float16)[None, None]


def ulps(a, b):
    """distance of two float32 in units of the last place (same sign, finite)"""
    ia = int(np.array(a, np.float32).view(np.int32))
    ib = int(np.array(b, np.float32).view(np.int32))
    return abs(ia - ib)
