"""Inputs that take the certified correlation path across float32's range and to NaNs: numpy only, seeded, shared by
tests/test_certified_cases_reference.py (CPU: the cases do what they claim, the oracle equals the reference's captures on them),
tests/test_gpu_certified_range.py (the kernels) and tests/golden/make_golden_certified.py (the captures).

A plain case is (name, C, shape, hw, f, m) with f, m float32 (C,) + shape; a pair case is (name, f, m) at PAIR_SHAPE for the whole-pair entry
point.  Every case is INSIDE the input contract of INTEGRATION.md: finite or NaN features with 729 C max|f - m|^2 <= 2^127.

Base kinds are the constructions of test_gpu_certified.py::test_certified_argmin_on_near_ties, for any shape; value transforms on top:
  @e<k>        both tensors times 2^k (exact: no feature leaves the normal range), so that ssd scales by 4^k -- into the denormal range from
               k = -64 down (729 ssd crosses certify.hip's 1e-36 flag at k = -64, ssd itself is denormal there; from k = -68 down ATen's
               denormal roundings create and break ties) and up to the contract's bound
  @x<s>        times a scale that is no power of two (values round: the argmin need not be the unscaled one)
  signed       values in [-1, 1)
  mirror       a moving image mirrored in z under a fixed image that is constant along z: pairs of displacements whose costs are the same
               sum in another order (mirror_perm: added for the mutation 2^-16 -> 2^-24 of the interval, which every other case survives:
               DESIGN 12.17)
  mixed        channel c times 2^(-30 + 5c)
  outlier      one voxel of one channel 2^20 times larger, at a corner, on a face, on an edge, one voxel inside a face, in the interior
               (the separable fast boxes subtract the term that leaves the window: the large term must leave nothing behind)
  nan          NaNs in the layouts of test_gpu_parity.py::test_nan_in_the_cost_volume, at the first and the last voxel (the interleaved
               tail), in a channel of the cascade's second block, and next to exact zeros"""
import numpy as np

SHAPES = [(12, (9, 12, 14), 3), (4, (6, 8, 37), 2), (16, (7, 9, 11), 3), (33, (6, 5, 8), 2)]
KINDS = ("textured", "periodic", "blocks", "zero_background", "plateau")
SCALES = (-74, -72, -70, -68, -66, -64, -62, -58, -40, -20, 20, 40, 55)      # + 57 where 729 C 2^(2e) <= 2^127
SCALES_SHORT = (-70, -66, -64, 20, 55)
ODD_SCALES = (1000.0, 3e-19)
PAIR_SHAPE = (12, (24, 32, 28))
PAIR_KW = dict(lambda_weight=0, grid_sp=2, disp_hw=3, selected_niter=1, grid_sp_adam=2, ic=True)
PAIR_SCALES = (-66, -20, -8, -4, 0, 4, 8, 20, 55)
CONTRACT_LOG2 = 127

# certify.hip's constants, restated (test_certified_cases_reference.py holds them against the file's text): the exact entry lies in
# [max(ssdu CLO - TINY, 0), ssdu CHI + min(ssdu, TINY)] with CLO / CHI = (1 -/+ EPS) / BOXES; a column with an entry 0 < ssdu < FLAG is
# resolved exactly
EPS, BOXES, TINY, FLAG = 2.0 ** -16, 729.0, np.float32(1.0e-40), 1.0e-36
CLO, CHI = np.float32((1.0 - EPS) / BOXES), np.float32((1.0 + EPS) / BOXES)


def cert_lower(s):
    """cert_lower of certify.hip on a float32 array, one float32 step further out: the product of two float32 is exact in float64, the sum
    is rounded to float64 and then to float32 where the kernel's fmaf rounds once -- the step covers that double rounding"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (s.astype(np.float64) * np.float64(CLO) - np.float64(TINY)).astype(np.float32)
        return np.maximum(np.nextafter(v, np.float32(-np.inf)), np.float32(0))


def cert_upper(s):
    with np.errstate(invalid="ignore", over="ignore"):
        v = (s.astype(np.float64) * np.float64(CHI) + np.minimum(s, TINY).astype(np.float64)).astype(np.float32)
        return np.nextafter(v, np.float32(np.inf))


def scale_allowed(C, e):
    """729 C 2^(2e) <= 2^127: the bound of the contract for features in [-1, 1)"""
    return 729 * C * 4.0 ** e <= 2.0 ** CONTRACT_LOG2


def base(kind, C, shape, seed=0):
    """(f, m) float32 in [0, 1) ([-1, 1) for `signed`)"""
    h, w, d = shape
    rng = np.random.default_rng(1000 * seed + 7 * C + h * w * d)
    f = rng.random((C,) + shape, dtype=np.float32)
    if kind == "textured":             # a shifted copy + 5 % noise: one clear minimum per column, near ties around it
        m = (np.roll(f, (1, -2, 1), (1, 2, 3)) + np.float32(0.05) * rng.random((C,) + shape, dtype=np.float32)).astype(np.float32)
    elif kind == "signed":
        f = (2 * f - 1).astype(np.float32)
        m = (np.roll(f, (1, -2, 1), (1, 2, 3)) + np.float32(0.05) * (2 * rng.random((C,) + shape, dtype=np.float32) - 1)).astype(np.float32)
    elif kind == "periodic":           # period 2 along every axis: displacements that differ by the period cost the same up to rounding
        b = rng.random((C, 2, 2, 2), dtype=np.float32)
        f = np.tile(b, (1, h // 2 + 1, w // 2 + 1, d // 2 + 1))[:, :h, :w, :d].copy()
        m = f.copy()
    elif kind == "blocks":             # piecewise constant features: whole plateaus of equal cost
        b = rng.random((C, 3, 3, 3), dtype=np.float32)
        f = np.repeat(np.repeat(np.repeat(b, h // 3 + 1, 1), w // 3 + 1, 2), d // 3 + 1, 3)[:, :h, :w, :d].copy()
        m = np.roll(f, 1, 2).copy()
    elif kind == "zero_background":    # columns that hold exact zeros next to positive sums
        m = np.roll(f, (0, 1, 1), (1, 2, 3)).copy()
        f[:, :, : w // 2] = 0
        m[:, :, : w // 2 + 1] = 0
    elif kind == "plateau":            # a flat moving image and a fixed image one ulp away from it in places: many identical tiny sums
        m = np.ones((C,) + shape, np.float32)
        f = np.ones((C,) + shape, np.float32)
        f[:, 2:5, 3:7, 2:9] = np.nextafter(np.float32(1), np.float32(0))
        f[0, min(4, h - 1), min(5, w - 1), min(6, d - 1)] = np.float32(0.999)
    elif kind in ("mirror", "mirror_perm"):
        # f constant along z, m mirrored in z: on the central plane the displacements +dz and -dz sum the same values in another order
        # -- costs that differ by their roundings only, and not by the same roundings in the fast kernels as in ATen.  mirror_perm: f the
        # same in every channel and the mirrored half with its channels reversed, so that the channel sums round differently too
        f = np.repeat(f[:, :1], h, 1).copy()
        m = rng.random((C,) + shape, dtype=np.float32)
        if kind == "mirror":
            m = np.concatenate([m[:, : (h + 1) // 2], m[:, : h // 2][:, ::-1]], 1).copy()
        else:
            f[:] = f[:1]
            m[:, h // 2 + 1:] = m[::-1, : h // 2][:, ::-1]
    else:
        raise ValueError(kind)
    return f, m


def scaled(fm, s):
    return tuple((a * np.float32(s)).astype(np.float32) for a in fm)


def _outlier_places(shape):
    h, w, d = shape
    return (("corner", (0, 0, 0)), ("face", (0, w // 2, d // 2)), ("edge", (h - 1, w - 1, d // 2)),
            ("inside_face", (1, w // 2, d // 2)), ("interior", (h // 2, w // 2, d // 2)))


def _nan_layouts(C, shape):
    """name -> (tensor 'f' / 'm', index tuples)"""
    h, w, d = shape
    lay = {
        "one_in_m": [("m", (3 % C, 2, 3, 4))],                              # some displacements of the neighbouring voxels see the NaN
        "voxel_in_f": [("f", (slice(None), 2, 2, 2))],                      # every displacement of the neighbourhood is NaN
        "scattered": [("m", (0, 0, 0, 0)), ("m", (5 % C, h - 1, w - 1, d - 1)), ("f", (2, 1, 4, 3))],
        "first_voxel": [("f", (0, 0, 0, 0))],
        "last_voxel": [("m", (C - 1, h - 1, w - 1, d - 1))],                # the reference tensor's last elements: the interleaved tail
    }
    if C > 16:
        lay["cascade"] = [("f", (C - 1, h // 2, w // 2, d // 2))]           # channel 16+: the cascade's second block
    elif C == 16:
        lay["cascade"] = [("f", (15, h // 2, w // 2, d // 2))]              # the last channel of the one full block
    return lay


def _put_nans(f, m, layout):
    f, m = f.copy(), m.copy()
    for which, idx in layout:
        (f if which == "f" else m)[idx] = np.nan
    return f, m


def _build():
    cases = []

    def add(name, C, shape, hw, fm):
        cases.append(("%s/C%d" % (name, C), C, shape, hw, fm[0], fm[1]))

    for si, (C, shape, hw) in enumerate(SHAPES):
        tex = base("textured", C, shape)
        add("textured", C, shape, hw, tex)
        for e in SCALES + (57,):
            if scale_allowed(C, e):
                add("textured@e%d" % e, C, shape, hw, scaled(tex, 2.0 ** e))
    # every other kind on two of the four shapes (rotating), unscaled and at the short list
    for ki, kind in enumerate(KINDS[1:]):
        for C, shape, hw in (SHAPES[ki % 4], SHAPES[(ki + 2) % 4]):
            b = base(kind, C, shape)
            add(kind, C, shape, hw, b)
        C, shape, hw = SHAPES[ki % 4]
        for e in SCALES_SHORT:
            add("%s@e%d" % (kind, e), C, shape, hw, scaled(base(kind, C, shape), 2.0 ** e))
    # rounding-level near ties between different sums (odd h: shapes 0 and 2).  The two seeds of mirror_perm are those, of twelve tried, on
    # which an interval of 2^-24 instead of 2^-16 certifies a wrong winner: seed 10 on the staged kernel's volume, seed 11 on the role kernel's
    for C, shape, hw in (SHAPES[0], SHAPES[2]):
        add("mirror", C, shape, hw, base("mirror", C, shape))
    for seed in (10, 11):
        C, shape, hw = SHAPES[0]
        add("mirror_perm_s%d" % seed, C, shape, hw, base("mirror_perm", C, shape, seed=seed))
    for C, shape, hw in (SHAPES[0], SHAPES[2]):
        for s in ODD_SCALES:
            add("textured@x%g" % s, C, shape, hw, scaled(base("textured", C, shape), s))
    for C, shape, hw in (SHAPES[0], SHAPES[3]):
        sg = base("signed", C, shape)
        add("signed", C, shape, hw, sg)
        for e in (-66, 55):
            add("signed@e%d" % e, C, shape, hw, scaled(sg, 2.0 ** e))
    for kind, (C, shape, hw) in (("textured", SHAPES[0]), ("textured", SHAPES[1]), ("signed", SHAPES[0])):
        ch = (2.0 ** (-30 + 5 * np.arange(C))).astype(np.float32).reshape(C, 1, 1, 1)
        add("mixed_channels_%s" % kind, C, shape, hw, tuple((a * ch).astype(np.float32) for a in base(kind, C, shape)))
    for C, shape, hw in (SHAPES[0], SHAPES[2]):
        for which in ("f", "m"):
            for pi, (place, pos) in enumerate(_outlier_places(shape)):
                f, m = (a.copy() for a in base("textured", C, shape))
                t = f if which == "f" else m
                c = (5 * pi + 3) % C
                t[(c,) + pos] = np.float32(2.0 ** 20) * max(t[(c,) + pos], np.float32(0.5))
                add("outlier_%s_%s" % (which, place), C, shape, hw, (f, m))
    for C, shape, hw in SHAPES:
        tex = base("textured", C, shape)
        for lname, layout in _nan_layouts(C, shape).items():
            if C in (16, 33) and lname in ("one_in_m", "voxel_in_f", "scattered"):
                continue
            add("nan_%s" % lname, C, shape, hw, _put_nans(tex[0], tex[1], layout))
    for C, shape, hw in (SHAPES[0], SHAPES[2]):                            # columns that hold NaNs and exact zeros together
        zb = base("zero_background", C, shape)
        h, w, d = shape
        add("nan_zero_background", C, shape, hw, _put_nans(zb[0], zb[1], [("m", (1, h // 2, w // 2 + 2, d // 2)), ("f", (0, 1, 1, 1))]))
    return cases


def _build_pairs():
    C, shape = PAIR_SHAPE
    pairs = []
    tex = base("textured", C, shape, seed=5)
    tex = (tex[0], (np.roll(tex[0], (1, -1, 2), (1, 2, 3)) + np.float32(0.1) * np.random.default_rng(6).random((C,) + shape, dtype=np.float32)).astype(np.float32))
    for e in PAIR_SCALES:
        pairs.append(("pair_textured@e%d" % e, ) + scaled(tex, 2.0 ** e))
    pairs.append(("pair_signed@e0",) + base("signed", C, shape, seed=5))
    zb = base("zero_background", C, shape, seed=5)
    for e in (-8, 8):
        pairs.append(("pair_zero_background@e%d" % e,) + scaled(zb, 2.0 ** e))
    pairs.append(("pair_nan_one_in_m",) + _put_nans(tex[0], tex[1], [("m", (3, 10, 13, 14))]))
    pairs.append(("pair_nan_scattered",) + _put_nans(tex[0], tex[1], [("m", (0, 0, 0, 0)), ("m", (5, 23, 31, 27)), ("f", (slice(None), 8, 9, 10)), ("f", (2, 17, 4, 21))]))
    return pairs


CASES = _build()
PAIRS = _build_pairs()
NAMES = [c[0] for c in CASES]
PAIR_NAMES = [p[0] for p in PAIRS]
assert len(set(NAMES)) == len(NAMES) and len(set(PAIR_NAMES)) == len(PAIR_NAMES)


def case(name):
    return CASES[NAMES.index(name)]


def pair(name):
    return PAIRS[PAIR_NAMES.index(name)]


def scale_exponent(name):
    """k of a '@e<k>' case (0 for an unscaled base case), None for every other case"""
    head = name.split("/")[0]
    if "@e" in head:
        return int(head.split("@e")[1])
    return 0 if head in KINDS + ("signed", "mirror") else None


def unscaled_name(name):
    head, tail = name.split("/")
    return head.split("@")[0] + "/" + tail


def inside_contract(C, f, m):
    """finite or NaN, and 729 C max|f - m|^2 <= 2^127 over every difference the kernels can form: any fixed value against any moving value
    or against the 0 that stands for a moving voxel outside the volume"""
    if np.isinf(f).any() or np.isinf(m).any():
        return False
    f_lo, f_hi = float(np.nanmin(f)), float(np.nanmax(f))
    m_lo, m_hi = min(float(np.nanmin(m)), 0.0), max(float(np.nanmax(m)), 0.0)
    big = max(f_hi - m_lo, m_hi - f_lo)
    return 729.0 * C * big * big <= 2.0 ** CONTRACT_LOG2
