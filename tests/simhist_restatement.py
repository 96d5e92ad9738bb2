"""A numpy restatement of convexadam_amd/csrc/simhist_core.h: the class of every voxel, the float64 taps of the fused
warp, the float32 bin arithmetic, the key-ordered range and the five counters -- written from the header's text, vectorised over the
voxels, sharing no code with it.  tests/test_simhist_reference.py holds the host program (the header itself under sanitizers) against
it bit for bit, tests/test_gpu_simhist.py and tests/test_gpu_simhist_fences.py the device.

Also here, because the tests need them stated once: the float64 numpy entropies, the bound on the difference between two float64
evaluations of an entropy (entropy_bound), the chance level of the mutual information of independent images (independence_factor),
and the case matrix."""
import numpy as np

F = np.float32
KEPT, MASKED, NON_FINITE, OUTSIDE, CLAMPED = range(5)


# ---- keys ---------------------------------------------------------------------------------------------------------------------------
def key(x):
    b = np.ascontiguousarray(x, F).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.uint32(k)
    b = (k & np.uint32(0x7FFFFFFF)) if (k & np.uint32(0x80000000)) else np.uint32(~k)
    return np.array([b], np.uint32).view(F)[0]


# ---- one voxel's pair and class -----------------------------------------------------------------------------------------------------
def components(field, shape):
    """the three float64 component planes of a (3, H, W, D) or (H, W, D, 3) field, flattened; elements widen exactly"""
    field = np.asarray(field)
    assert field.dtype in (np.float32, np.float64)
    if field.shape == tuple(shape) + (3,):
        return [field[..., a].reshape(-1).astype(np.float64) for a in range(3)]
    assert field.shape == (3,) + tuple(shape), field.shape
    return [field[a].reshape(-1).astype(np.float64) for a in range(3)]


def taps(moving, c0, c1, c2):
    """taps_linear_f64 of interp_f64.h for coordinates that are inside: the sum over the 8 taps (axis 0 slowest) of ((v * w0) * w1) * w2
    from 0.0, weights {1 - t, 1 - (1 - t)}, upper taps clamped to the last index"""
    H, W, D = moving.shape
    f = [np.floor(c) for c in (c0, c1, c2)]
    t = [c - fl for c, fl in zip((c0, c1, c2), f)]
    lo = [fl.astype(np.int64) for fl in f]
    hi = [np.minimum(l + 1, n - 1) for l, n in zip(lo, (H, W, D))]
    w = [(1.0 - tt, 1.0 - (1.0 - tt)) for tt in t]
    idx = [(l, h) for l, h in zip(lo, hi)]
    mov = moving.astype(np.float64)
    r = np.zeros(c0.shape, np.float64)
    for i in range(2):
        for j in range(2):
            for k in range(2):
                r = r + ((mov[idx[0][i], idx[1][j], idx[2][k]] * w[0][i]) * w[1][j]) * w[2][k]
    return r


def sample(fixed, moving, field=None, mask=None, drop_outside=False):
    """(class, a, b) of every voxel, flattened; a and b are meaningful where the class is KEPT"""
    fixed, moving = np.ascontiguousarray(fixed, F), np.ascontiguousarray(moving, F)
    shape = fixed.shape
    V = fixed.size
    cls = np.full(V, -1, np.int64)
    a = fixed.reshape(-1).copy()
    b = np.zeros(V, F)
    if mask is not None:
        cls[np.asarray(mask).reshape(-1) == 0] = MASKED
    cls[(cls < 0) & ~np.isfinite(a)] = NON_FINITE
    if field is None:
        b = moving.reshape(-1).copy()
    else:
        H, W, D = shape
        q = np.arange(V)
        i = [(q // (W * D)).astype(np.float64), ((q // D) % W).astype(np.float64), (q % D).astype(np.float64)]
        with np.errstate(invalid="ignore", over="ignore"):
            c = [ii + uu for ii, uu in zip(i, components(field, shape))]
        finite = np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2])
        cls[(cls < 0) & ~finite] = NON_FINITE
        with np.errstate(invalid="ignore"):
            inside = finite & (c[0] >= 0) & (c[0] <= H - 1) & (c[1] >= 0) & (c[1] <= W - 1) & (c[2] >= 0) & (c[2] <= D - 1)
        if drop_outside:
            cls[(cls < 0) & ~inside] = OUTSIDE
        r = np.zeros(V, np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            r[inside] = taps(moving, c[0][inside], c[1][inside], c[2][inside])
            b = r.astype(F)
    cls[(cls < 0) & ~np.isfinite(b)] = NON_FINITE
    cls[cls < 0] = KEPT
    return cls, a, b


def _class_counts(cls):
    stats = np.zeros(5, np.int64)
    for k in (KEPT, MASKED, NON_FINITE, OUTSIDE):
        stats[k] = int((cls == k).sum())
    return stats


def value_range(fixed, moving, field=None, mask=None, drop_outside=False, sampled=None):
    """-> (range float32[4], stats int64[5]); sampled: what sample() returned for these arguments, to share it among calls"""
    cls, a, b = sampled if sampled is not None else sample(fixed, moving, field, mask, drop_outside)
    kept = cls == KEPT
    out = np.array([np.inf, -np.inf, np.inf, -np.inf], F)
    if kept.any():
        ka, kb = key(a[kept]), key(b[kept])
        out = np.array([unkey(ka.min()), unkey(ka.max()), unkey(kb.min()), unkey(kb.max())], F)
    return out, _class_counts(cls)


def scale(lo, hi, nb):
    lo, hi = F(lo), F(hi)
    if not hi > lo:
        return F(0.0)
    with np.errstate(over="ignore", divide="ignore"):
        s = F(nb) / F(hi - lo)
    return s if np.isfinite(s) else F(0.0)


def bins_of(x, lo, hi, nb):
    x = np.asarray(x, F)
    s = scale(lo, hi, nb)
    with np.errstate(over="ignore", invalid="ignore"):
        t = ((x - F(lo)).astype(F) * s).astype(F)
    out = np.zeros(x.shape, np.int64)
    top = t >= F(nb)
    mid = ~top & (t >= 0)                      # a NaN t fails both comparisons and stays in bin 0
    out[top] = nb - 1
    out[mid] = t[mid].astype(np.int64)
    return out


def joint_hist(fixed, moving, bins, rng, field=None, mask=None, drop_outside=False, sampled=None):
    """-> (hist int64[bins_a][bins_b], stats int64[5])"""
    ba, bb = (bins, bins) if isinstance(bins, int) else bins
    rng = np.asarray(rng, F)
    cls, a, b = sampled if sampled is not None else sample(fixed, moving, field, mask, drop_outside)
    kept = cls == KEPT
    a, b = a[kept], b[kept]
    cell = bins_of(a, rng[0], rng[1], ba) * bb + bins_of(b, rng[2], rng[3], bb)
    hist = np.bincount(cell, minlength=ba * bb).astype(np.int64).reshape(ba, bb)
    stats = _class_counts(cls)
    with np.errstate(invalid="ignore"):
        stats[CLAMPED] = int(((a < rng[0]) | (a > rng[1]) | (b < rng[2]) | (b > rng[3])).sum())
    return hist, stats


# ---- entropies in float64 numpy -----------------------------------------------------------------------------------------------------
def entropy(counts):
    c = np.asarray(counts, np.int64).reshape(-1)
    n = int(c.sum())
    if n == 0:
        return float("nan")
    p = c[c > 0].astype(np.float64) / float(n)
    return float(-(p * np.log(p)).sum())


def entropies(hist):
    hist = np.asarray(hist, np.int64)
    return entropy(hist.sum(1)), entropy(hist.sum(0)), entropy(hist)


def mutual_information(hist):
    ha, hb, hab = entropies(hist)
    return ha + hb - hab


def normalized_mutual_information(hist):
    ha, hb, hab = entropies(hist)
    return float("nan") if hab == 0 else (ha + hb) / hab


def entropy_bound(counts):
    """A bound on |H' - H''| for two float64 evaluations of H = -sum p ln p over the K non-zero bins of `counts`, whatever the order of
    their sums and whichever correctly implemented logarithm they call:  (K + 8) * 2^-52 * sum |p ln p|.
      p = c / n is one IEEE division of two exactly represented integers: the SAME double in both evaluations, no difference.
      ln p: each library's logarithm is within one ulp of the true value, |error| <= 2^-52 |ln p|; two evaluations differ by <= 2 * 2^-52.
      p * ln p: one rounding each, 2^-53 relative; the two differ by <= 2^-52 (relative to |p ln p|, to first order).
      the sum of K terms in ANY order carries at most (K - 1) * 2^-53 * sum |terms| (Higham, Accuracy and Stability, (4.4)); two sums
      differ by <= (K - 1) * 2^-52 * sum |p ln p|.
    Together (K + 2) * 2^-52 * sum |p ln p| to first order; the 6 on top of that covers every second-order term ((K + 2)^2 * 2^-104 is
    below 6 * 2^-52 for any K up to 2^26) and the final negation, which is exact."""
    c = np.asarray(counts, np.int64).reshape(-1)
    n = int(c.sum())
    p = c[c > 0].astype(np.float64) / float(n)
    return (p.size + 8) * 2.0 ** -52 * float(np.abs(p * np.log(p)).sum())


def independence_factor(dof, miss=1e-6):
    """The factor f in  MI <= f * dof / (2 n)  for the plug-in mutual information of n independent draws, dof = (bins_a - 1)(bins_b - 1).
    2 n MI is the G statistic of the independence test, asymptotically chi-square with `dof` degrees of freedom (Wilks), whose mean is
    dof: hence the issue's (bins_a - 1)(bins_b - 1) / (2 n).  Laurent and Massart (2000, Lemma 1):  P(chi2_k >= k + 2 sqrt(k x) + 2 x)
    <= exp(-x).  With x = ln(1 / miss) the bound fails for fewer than `miss` of all draws:  f = 1 + 2 sqrt(x / dof) + 2 x / dof.
    The chi-square limit needs well-filled cells; the tests that use it keep n / (bins_a bins_b) >= 50 expected counts per cell."""
    x = float(np.log(1.0 / miss))
    return 1.0 + 2.0 * np.sqrt(x / dof) + 2.0 * x / dof


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def remap(x):
    """the issue's non-monotone intensity map exp(-1.3 x) + 0.1 x^2, float32 in and out"""
    x = np.asarray(x, np.float64)
    return (np.exp(-1.3 * x) + 0.1 * x * x).astype(F)


def volume(shape, seed, spread=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * spread).astype(F)


def field_for(shape, seed, planar, f64):
    """A field of a few voxels whose first voxels are planted: coordinates exactly on n - 1 and on 0, just outside on either side, far
    outside, and fractional ones; the rest is random, so that some voxels of every shape with an axis > 1 leave the volume"""
    H, W, D = shape
    rng = np.random.default_rng(seed)
    u = rng.uniform(-2.5, 2.5, (H, W, D, 3))
    u[rng.uniform(size=(H, W, D)) < 0.25] = 0.0                                   # exactly on the grid
    flat = u.reshape(-1, 3)
    V = flat.shape[0]
    q = np.arange(V)
    i = np.stack([q // (W * D), (q // D) % W, q % D], 1).astype(np.float64)
    n1 = np.array([H - 1, W - 1, D - 1], np.float64)
    plant = [n1, np.zeros(3), n1 + 0.5, np.full(3, -0.25), n1 - 0.5, np.full(3, 1e6), n1 + 2.0 ** -20]
    for k, target in enumerate(plant):
        if k < V:
            flat[k] = target - i[k]                                                # exact in float64; the float32 cast below may move it
    u = flat.reshape(H, W, D, 3).astype(np.float64 if f64 else F)
    return np.ascontiguousarray(u.transpose(3, 0, 1, 2)) if planar else u


def mask_for(shape, seed):
    m = (np.random.default_rng(seed).uniform(size=shape) < 0.7).astype(np.uint8)
    m[m != 0] = np.random.default_rng(seed + 1).integers(1, 256, int(m.sum()), dtype=np.uint8)      # any non-zero value keeps
    return m


SHAPES = [(1, 1, 1), (2, 3, 67), (3, 5, 7), (5, 4, 130), (24, 20, 33)]
BINS = [(2, 2), (32, 32), (64, 64), (7, 130), (128, 128), (129, 128), (256, 256)]
FIELDS = [None, ("planar", "f32"), ("planar", "f64"), ("interleaved", "f32"), ("interleaved", "f64")]


def case(shape, bins, with_mask, field_kind, drop_outside, seed=0):
    """one case of the matrix -> dict(fixed, moving, field, mask, drop_outside, bins)"""
    s = 1000 + 17 * seed + sum(shape)
    fixed, moving = volume(shape, s, 2.0), remap(volume(shape, s + 1))
    field = None if field_kind is None else field_for(shape, s + 2, field_kind[0] == "planar", field_kind[1] == "f64")
    return dict(fixed=fixed, moving=moving, field=field, mask=mask_for(shape, s + 3) if with_mask else None, drop_outside=bool(drop_outside),
                bins=bins)


def matrix(shapes=SHAPES, bins=BINS):
    """the whole matrix as (name, case): every shape x bins x mask x field (layout, element) x drop_outside (with a field)"""
    out = []
    for si, shape in enumerate(shapes):
        for bi, b in enumerate(bins):
            for with_mask in (False, True):
                for fk in FIELDS:
                    for drop in ((0, 1) if fk is not None else (0,)):
                        name = "%s-b%dx%d-%s-%s-drop%d" % ("x".join(map(str, shape)), b[0], b[1], "mask" if with_mask else "nomask",
                                                           "-".join(fk) if fk else "nofield", drop)
                        out.append((name, case(shape, b, with_mask, fk, drop, seed=si * 7 + bi)))
    return out


def planted_non_finite(shape=(5, 4, 130), seed=5):
    """fixed, moving and an interleaved float64 field with NaN and +-Inf planted in each"""
    c = case(shape, (32, 32), False, ("interleaved", "f64"), 0, seed=seed)
    f, m, u = c["fixed"], c["moving"], c["field"]
    f.reshape(-1)[[3, 70, 900]] = [np.nan, np.inf, -np.inf]
    m.reshape(-1)[[5, 71, 901, 1300]] = [np.nan, -np.inf, np.inf, np.nan]
    u.reshape(-1, 3)[[11, 200, 1500, 2000], [0, 1, 2, 0]] = [np.nan, np.inf, -np.inf, np.nan]
    return c


def expected(c, rng=None):
    """(range, range stats, hist, hist stats) of a case by this restatement; rng: a given range instead of the case's own"""
    r, rs = value_range(c["fixed"], c["moving"], c["field"], c["mask"], c["drop_outside"])
    h, hs = joint_hist(c["fixed"], c["moving"], c["bins"], r if rng is None else rng, c["field"], c["mask"], c["drop_outside"])
    return r, rs, h, hs
