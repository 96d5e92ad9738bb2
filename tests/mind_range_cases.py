"""Inputs that take MIND-SSC (convex_adam_utils.py:24-68) across float32's range and to non-finite voxels: numpy only, seeded, shared by
tests/test_mind_range_reference.py (CPU: the cases do what they claim, the oracle equals the reference on them),
tests/test_gpu_mind_range.py (the kernels) and tests/golden/make_golden_mind_range.py (the reference's captures).

The input contract: voxels finite with K^3 (max - min)^2 <= 2^127, K = 2 radius + 1 -- no patch sum can overflow -- or
non-finite; any NaN or +-Inf voxel gives an all-NaN descriptor (the NaN reaches `mind_var.mean()`, torch.clamp with a NaN bound returns NaN).

A case is Case(name, shape, radius, dilation, img, cls); name = '<kind>/<H>x<W>x<D>'.  `base` of a shape is white noise of sigma 10 (the
issue's `base` at 12x14x16).  Kinds, by class:
  control       base
  pow2          base 2^-40, base 2^40: exact multiples, nothing under- or overflows -- the descriptor is that of base bit for bit
  denormal      base 2^-62 (squared differences partly denormal), base 1e-22, base 1e-23 (denormal variances, exact zeros, lo rounds to 0)
  zero_mean     base 1e-24: the patch sums round to 0 (all of them at the small shapes, all but a handful at the two large ones), the mean is
                0 or a denormal with lo = 0: 0 / 0, NaN on every voxel whose variance is 0 -- at least 99.9 % of the descriptor
  top           base scaled so that K^3 (max - min)^2 sits just below 2^127.  At the two large shapes V mean(variance) is then beyond 2^128:
                these are sum-overflow cases too (sum_overflows)
  clamp         a 4x4x4 block of base times 1e17 (the lower clamp bound binds on most of the volume, 35 orders of magnitude below the mean);
                1e-3 base with one voxel at 1e18 (the same, from one voxel).
                These two leave the K^3 (max - min)^2 bound but not the range in which every patch sum is finite (held by the CPU test).
                At 6x6x6 the block is 30 % of the volume and 1000 mean exceeds float32: the reference RAISES there (torch.clamp refuses the
                bound), the library and the oracle clamp with hi = Inf
  sum_overflow  base scaled so that every patch sum is finite while V mean(variance) = 2^128.5: torch's float32 sum of the variances is
                Inf, the mean Inf, lo = hi = Inf and every value exp(-x / Inf) = 1; the exactly rounded mean gives proper descriptors.
                Only at shapes with enough voxels (largest patch sum / mean variance < V / 2^1.5, see sum_overflow_scale)
  nonfinite     one interior NaN, NaN at voxel [0,0,0], at the very last voxel, on a face, an all-NaN image, one +Inf, one -Inf voxel

Shapes: the smallest that select each plan of DESIGN 30.1 (the reason stands beside each); 36x32x32 carries the sum-overflow case only (V >= 32768:
the two-pass mean kernels of mind_mean_threads = 8).  Every extent is at least 2 dilation: each voxel is read by some shifted tap."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name shape radius dilation img cls")

# (shape, radius, dilation, plan)
SHAPES = (((12, 14, 64), 1, 2, "wide march: D % 64 == 0"),
          ((13, 19, 92), 1, 2, "narrow march (D % 64 = 28), partial tiles and blocks"),
          ((7, 9, 15), 1, 2, "odd D: k_mind<1,64> + k_mind_finish<1>, not pooled"),
          ((6, 6, 6), 1, 2, "D % 4 == 2: k_mind<1,64>, pooled through the planar k_mind_finish_pool"),
          ((9, 10, 12), 2, 2, "k_mind<2,64>"),
          ((9, 9, 33), 3, 4, "k_mind<3,32>"))
OVERFLOW_ONLY = ((36, 32, 32), 1, 2, "two-pass mean kernels (V >= 32768)")
CLASSES = ("control", "pow2", "denormal", "zero_mean", "top", "clamp", "sum_overflow", "nonfinite")
CONTRACT_LOG2 = 127
SUM_TARGET_LOG2 = 128.5          # V mean(variance) of the sum-overflow case: beyond float32 (max < 2^128) by more than any rounding of the sum

O1 = ((0, 0, -1), (0, -1, 0), (0, -1, 0), (0, 0, 1), (0, 0, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 1, 0), (0, 1, 0), (0, 1, 0))
O2 = ((-1, 0, 0), (-1, 0, 0), (0, 0, -1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, -1, 0), (0, 0, 1), (-1, 0, 0), (0, 0, -1), (0, 0, 1), (1, 0, 0))


def tag(shape):
    return "%dx%dx%d" % shape


def base(shape):
    return (np.random.default_rng(0).standard_normal(shape) * 10).astype(np.float32)


def times(img, s):
    with np.errstate(over="ignore", under="ignore"):
        return (img * np.float32(s)).astype(np.float32)


def patch_sums(img, radius, dilation):
    """float64 restatement of the twelve patch sums BEFORE their division by K^3, (12, H, W, D): both replicate paddings of the reference
    (the shifts clamp, the box clamps the position first).  Only used to place cases; the tests compare against the oracle."""
    H, W, D = img.shape
    d, r = dilation, radius
    P = np.pad(img.astype(np.float64), d, mode="edge")
    out = np.empty((12, H, W, D))
    for c in range(12):
        a = P[d + O1[c][0] * d: d + O1[c][0] * d + H, d + O1[c][1] * d: d + O1[c][1] * d + W, d + O1[c][2] * d: d + O1[c][2] * d + D]
        b = P[d + O2[c][0] * d: d + O2[c][0] * d + H, d + O2[c][1] * d: d + O2[c][1] * d + W, d + O2[c][2] * d: d + O2[c][2] * d + D]
        with np.errstate(over="ignore", invalid="ignore"):
            sq = np.pad((a - b) ** 2, r, mode="edge")
            s = np.zeros((H, W, D))
            for z in range(2 * r + 1):
                for y in range(2 * r + 1):
                    for x in range(2 * r + 1):
                        s += sq[z: z + H, y: y + W, x: x + D]
        out[c] = s
    return out


def mean_variance(sums, radius):
    """mean over the volume of mean_c(ssd_c - min_c ssd), in float64"""
    ssd = sums / float((2 * radius + 1) ** 3)
    return float((ssd - ssd.min(0)).mean())


def contract_log2(img, radius):
    """log2 of K^3 (max - min)^2"""
    rng = float(img.max()) - float(img.min())
    return float(np.log2((2 * radius + 1) ** 3) + 2 * np.log2(rng))


def top_scale(img, radius):
    """the largest float32 s (searched downwards from the real solution) with K^3 (max - min)^2 of s img still <= 2^127"""
    rng = float(img.max()) - float(img.min())
    s = np.float32(np.sqrt(2.0 ** CONTRACT_LOG2 / (2 * radius + 1) ** 3) / rng)
    while contract_log2(times(img, s), radius) > CONTRACT_LOG2:
        s = np.nextafter(s, np.float32(0))
    return s


def sum_overflow_scale(img, radius, dilation):
    """s with V mean(variance of s img) = 2^128.5, or None where a patch sum of s img would reach 2^127.5 (the shape has too few voxels for
    the sum of the variances to overflow before a patch does)"""
    sums = patch_sums(img, radius, dilation)
    s2 = 2.0 ** SUM_TARGET_LOG2 / (img.size * mean_variance(sums, radius))
    if float(sums.max()) * s2 >= 2.0 ** 127.5:
        return None
    return np.float32(np.sqrt(s2))


def nonfinite_layouts(shape):
    H, W, D = shape
    mid = (H // 2, W // 2, D // 2)
    return (("nan_interior", mid, np.nan), ("nan_first", (0, 0, 0), np.nan), ("nan_last", (H - 1, W - 1, D - 1), np.nan),
            ("nan_face", (0, W // 2, D // 2), np.nan), ("nan_all", (slice(None),) * 3, np.nan), ("pos_inf", mid, np.inf), ("neg_inf", mid, -np.inf))


def _cases_of(shape, radius, dilation, only=None):
    b = base(shape)
    out = []

    def add(kind, img, cls):
        if only is None or cls in only:
            out.append(Case("%s/%s" % (kind, tag(shape)), shape, radius, dilation, np.ascontiguousarray(img, np.float32), cls))

    add("base", b, "control")
    add("base@e-40", times(b, 2.0 ** -40), "pow2")
    add("base@e40", times(b, 2.0 ** 40), "pow2")
    add("base@e-62", times(b, 2.0 ** -62), "denormal")
    add("base@x1e-22", times(b, 1e-22), "denormal")
    add("base@x1e-23", times(b, 1e-23), "denormal")
    add("base@x1e-24", times(b, 1e-24), "zero_mean")
    add("top", times(b, top_scale(b, radius)), "top")
    blk = b.copy()
    blk[1:5, 1:5, 1:5] *= np.float32(1e17)
    add("block@x1e17", blk, "clamp")
    vox = times(b, 1e-3)
    vox[shape[0] // 2, shape[1] // 2, shape[2] // 2] = np.float32(1e18)
    add("voxel_1e18", vox, "clamp")
    s = sum_overflow_scale(b, radius, dilation)
    if s is not None:
        add("sum_overflow", times(b, s), "sum_overflow")
    for kind, at, v in nonfinite_layouts(shape):
        img = b.copy()
        img[at] = v
        add(kind, img, "nonfinite")
    return out


def _build():
    cases = []
    for shape, r, d, _ in SHAPES:
        cases += _cases_of(shape, r, d)
    cases += _cases_of(*OVERFLOW_ONLY[:3], only=("sum_overflow",))
    return cases


CASES = _build()
NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def case(name):
    return CASES[NAMES.index(name)]


def base_name(name):
    """the control case of the same shape"""
    return "base/" + name.split("/")[1]
