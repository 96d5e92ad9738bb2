"""Cost volumes that take the coupled-convex stage (convex_adam_utils.py:93-109; csrc/convex.hip) across float32's range, to costs of
either sign, to -Inf and to bounds that overflow: numpy only, seeded, shared by tests/test_coupled_range_reference.py (CPU: the cases do
what they claim, the oracle equals upstream on them), tests/test_gpu_coupled_range.py (the kernels) and
tests/golden/make_golden_coupled_range.py (upstream's captures).

A case is a Case: name = '<kind>/<h>x<w>x<d>-hw<hw>', shape, hw, cls, and -- built on first use, then kept read-only --
  ssd()         [K, h, w, d] float32, the volume handed to the operator
  mask          None, or the [h, w, d] uint8 cell mask of a `masked` case (the columns of dropped cells hold NaN, -Inf and 3e38 in turn)
  seen()        the values the passes see: ssd(), or ssd() with clean +0.0 columns where the mask drops the cell
  seed(which)   'true': torch.argmin(seen, 0) -- the first NaN of a column, otherwise its first minimum under `<`; 'foreign': random indices

Geometries: the smallest that select each kernel (GEOMETRIES; k_slices restates cvx_common.h and the module asserts what it gives).
At the shapes of 27 and 125 displacements every displacement is its own slice of the plain and the streamed argmin pass; LARGE = 16x20x16,
hw 2 has kslice = 2 -- the in-register scan of a slice AND the atomicMin merge across slices decide -- and carries the five kinds of
LARGE_KINDS only.  (4x5x6, hw 4 has slices of two as well: 729 displacements against a target of 512 slices.)

Classes and kinds (r = rng.random, float32; every kind at every small geometry):
  scaled_noise    noise@2^e = 2^e r for e in -140 (all entries denormal), -126, -100, -30, 10, 17, 24, 60, 100, 127 (the maximum stays finite)
  real_minimum    realmin@2^e, e in -100, 14, 40, 120: the volume of test_coupled_convex_vs_oracle (features rolled by (1, -2, 3) through the
                  oracle's correlate) times 2^e -- pruning closes boxes here, on noise it does not
  offset_spread   2^14+r, 2^17+64r, -2^17+8r, 2^24+r: ulp(cost) is comparable to the penalty steps, rounding creates ties (2^24+r holds two
                  values only)
  absorbed        2^30+r, -2^30+r: every entry rounds to +-2^30, a penalty below half an ulp (64, 32) vanishes, index 0 wins every pass
  signed          signed@2^e = 2^e (r - 0.5) and negative@2^e = -2^e r for e in 0, 20, 100
  wide_spread     +-1e30^uniform(-1, 1): sixty orders of magnitude inside one column
  overflow_bound  half of the columns hold 3e38 and -3e38: B - smin = +Inf for any previous winner at the large entry
  neg_inf         -Inf scattered at 10 % and 40 %; whole -Inf columns (interior, faces, corners); columns with -Inf and +Inf; columns with
                  -Inf and one NaN, before and after the first -Inf; a plane of -Inf columns
  signed_zeros    columns of +0.0 with -0.0 only at later indices (-0.0 orders below +0.0 in the keys, equal under `<`) and one column that
                  is all -0.0; once among noise, once as the whole volume
  masked          2^14+r, signed@2^20 and -Inf at 10 % under a cell mask that keeps about 60 % of the cells
The kinds of neg_inf and signed_zeros and signed@2^0 are built from half values (half_ok): cvx_coupled_convex_f16 takes them unchanged."""
import zlib

import numpy as np

CLASSES = ("scaled_noise", "real_minimum", "offset_spread", "absorbed", "signed", "wide_spread", "overflow_bound", "neg_inf", "signed_zeros",
           "masked")
# (shape, hw, what it selects)
GEOMETRIES = (((5, 6, 7), 2, "v % 4 != 0: scalar k_argmin, scalar stream"),
              ((4, 6, 8), 2, "the 16-byte kernels"),
              ((5, 6, 7), 1, "27 displacements"),
              ((4, 5, 6), 4, "729 displacements: a listed box of more than 256 takes several chunks of k_argmin_wave"))
LARGE = ((16, 20, 16), 2, "kslice = 2: a slice's scan and the merge across slices")
LARGE_KINDS = ("noise@2^17", "noise@2^127", "realmin@2^14", "2^14+r", "signed@2^20")
COEFFS = (0.003, 0.01, 0.03, 0.1, 0.3, 1.0)
NOISE_EXPONENTS = (-140, -126, -100, -30, 10, 17, 24, 60, 100, 127)
REALMIN_EXPONENTS = (-100, 14, 40, 120)
SIGNED_EXPONENTS = (0, 20, 100)
MASKED_KINDS = ("2^14+r", "signed@2^20", "neginf_scattered10")
MASK_POISON = (np.nan, -np.inf, 3e38)
INF = np.float32(np.inf)


def k_slices(v, K, aligned=True):
    """(kslice, nslices) of the plain and the streamed argmin pass (k_slices and argmin_pass, csrc/cvx_common.h and convex.hip)"""
    vec4 = v % 4 == 0 and aligned
    xb = -(-(v // 4 if vec4 else v) // 256)
    want = -(-(512 if vec4 else 1024) // xb)
    kslice = -(-K // min(max(want, 1), K))
    return kslice, -(-K // kslice)


def tag(shape, hw):
    return "%dx%dx%d-hw%d" % (shape + (hw,))


def widen(x):
    """float32 -> half -> float32"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def f32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.ascontiguousarray(x, dtype=np.float32)


def first_minimum(vol):
    """torch.argmin(vol, 0): the first NaN of a column, otherwise the first index of its minimum under `<` (-0.0 == +0.0)"""
    col = vol.reshape(vol.shape[0], -1)
    nan = np.isnan(col)
    first = np.where(nan.any(0), nan.argmax(0), np.where(nan, np.inf, col).argmin(0))
    return first.reshape(vol.shape[1:]).astype(np.int64)


_realmin = {}


def realmin_base(shape, hw):
    """the volume of test_coupled_convex_vs_oracle (tests/test_gpu_parity.py) at this geometry"""
    if (shape, hw) not in _realmin:
        from oracle import oracle
        rng = np.random.default_rng(hw)
        f = rng.random((12,) + shape, dtype=np.float32)
        m = np.roll(f, (1, -2, 3), (1, 2, 3)) + 0.05 * rng.random((12,) + shape, dtype=np.float32)
        _realmin[shape, hw] = oracle.correlate(f, m.astype(np.float32), hw)[0]
    return _realmin[shape, hw]


def marked_columns(shape):
    """interior, faces, corners"""
    h, w, d = shape
    return ((h // 2, w // 2, d // 2), (1, 2, 3), (0, w // 2, d // 2), (h // 2, 0, 2), (h // 2, w // 2, d - 1), (0, 0, 0), (h - 1, w - 1, d - 1))


def _noise(e):
    return lambda rng, K, shape, hw: f32(rng.random((K,) + shape, dtype=np.float32).astype(np.float64) * 2.0 ** e)


def _realmin_at(e):
    return lambda rng, K, shape, hw: f32(realmin_base(shape, hw).astype(np.float64) * 2.0 ** e)


def _offset(off, spread):
    return lambda rng, K, shape, hw: f32(off + spread * rng.random((K,) + shape, dtype=np.float32).astype(np.float64))


def _signed(e, negative):
    def make(rng, K, shape, hw):
        r = rng.random((K,) + shape, dtype=np.float32)
        x = -r if negative else r - np.float32(0.5)
        return widen(x) if e == 0 else f32(x.astype(np.float64) * 2.0 ** e)     # (e = 0: half values)
    return make


def _wide(rng, K, shape, hw):
    sign = np.where(rng.random((K,) + shape) < 0.5, -1.0, 1.0)
    return f32(sign * 1e30 ** rng.uniform(-1.0, 1.0, (K,) + shape))


def _overflow(rng, K, shape, hw):
    ssd = f32((rng.random((K,) + shape, dtype=np.float32) - np.float32(0.5)).astype(np.float64) * 2.0 ** 100)
    col = ssd.reshape(K, -1)
    for x in np.nonzero(rng.random(col.shape[1]) < 0.5)[0]:
        k1, k2 = rng.choice(K, 2, replace=False)
        col[k1, x], col[k2, x] = np.float32(3e38), np.float32(-3e38)
    return ssd


def half_noise(rng, K, shape):
    return widen(rng.random((K,) + shape, dtype=np.float32))


def _neginf_scattered(share):
    def make(rng, K, shape, hw):
        ssd = half_noise(rng, K, shape)
        ssd[rng.random(ssd.shape) < share] = -INF
        return ssd
    return make


def _neginf_columns(rng, K, shape, hw):
    ssd = half_noise(rng, K, shape)
    for z, y, x in marked_columns(shape):
        ssd[:, z, y, x] = -INF
    return ssd


def _neginf_with_posinf(rng, K, shape, hw):
    ssd = half_noise(rng, K, shape)
    for i, (z, y, x) in enumerate(marked_columns(shape)):
        pick = rng.random(K)
        ssd[:, z, y, x] = np.where(pick < 0.3, -INF, np.where(pick < 0.6, INF, ssd[:, z, y, x]))
        ssd[0, z, y, x] = INF if i % 2 == 0 else -INF               # the first -Inf behind a +Inf / in front of every +Inf
        ssd[K - 1, z, y, x] = -INF
    return ssd


def _neginf_with_nan(rng, K, shape, hw):
    ssd = half_noise(rng, K, shape)
    p = K // 3
    for i, (z, y, x) in enumerate(marked_columns(shape)):
        ssd[p, z, y, x] = -INF
        ssd[K - 2, z, y, x] = -INF
        ssd[p - 2 if i % 2 == 0 else p + 3, z, y, x] = np.nan     # before / after the first -Inf
    return ssd


def _neginf_plane(rng, K, shape, hw):
    ssd = half_noise(rng, K, shape)
    ssd[:, :, shape[1] // 2, :] = -INF
    return ssd


def _zeros(everywhere):
    def make(rng, K, shape, hw):
        ssd = half_noise(rng, K, shape)
        col = ssd.reshape(K, -1)
        zero = np.ones(col.shape[1], bool) if everywhere else rng.random(col.shape[1]) < 0.3
        col[:, zero] = 0.0
        late = (rng.random(col.shape) < 0.2) & zero[None]
        late[0] = False                                             # -0.0 only behind the first +0.0
        late[K - 1] |= zero
        col[late] = -0.0
        z, y, x = marked_columns(shape)[0]
        ssd[:, z, y, x] = -0.0                                      # the column that is all -0.0
        return ssd
    return make


def _kinds():
    out = []
    out += [("noise@2^%d" % e, "scaled_noise", _noise(e)) for e in NOISE_EXPONENTS]
    out += [("realmin@2^%d" % e, "real_minimum", _realmin_at(e)) for e in REALMIN_EXPONENTS]
    out += [("2^14+r", "offset_spread", _offset(2.0 ** 14, 1.0)), ("2^17+64r", "offset_spread", _offset(2.0 ** 17, 64.0)),
            ("-2^17+8r", "offset_spread", _offset(-2.0 ** 17, 8.0)), ("2^24+r", "offset_spread", _offset(2.0 ** 24, 1.0))]
    out += [("2^30+r", "absorbed", _offset(2.0 ** 30, 1.0)), ("-2^30+r", "absorbed", _offset(-2.0 ** 30, 1.0))]
    out += [("signed@2^%d" % e, "signed", _signed(e, False)) for e in SIGNED_EXPONENTS]
    out += [("negative@2^%d" % e, "signed", _signed(e, True)) for e in SIGNED_EXPONENTS]
    out += [("wide@1e30", "wide_spread", _wide), ("3e38_and_-3e38", "overflow_bound", _overflow)]
    out += [("neginf_scattered10", "neg_inf", _neginf_scattered(0.1)), ("neginf_scattered40", "neg_inf", _neginf_scattered(0.4)),
            ("neginf_columns", "neg_inf", _neginf_columns), ("neginf_with_posinf", "neg_inf", _neginf_with_posinf),
            ("neginf_with_nan", "neg_inf", _neginf_with_nan), ("neginf_plane", "neg_inf", _neginf_plane)]
    out += [("zeros_late_negative", "signed_zeros", _zeros(False)), ("zeros_everywhere", "signed_zeros", _zeros(True))]
    return out


KINDS = _kinds()
WHOLE_NEGINF_COLUMNS = ("neginf_columns", "neginf_plane")          # kinds with columns that are -Inf throughout
TIE_KINDS = ("2^14+r", "-2^17+8r")


class Case:
    def __init__(self, kind, cls, make, shape, hw, masked=False):
        self.kind, self.cls, self.shape, self.hw, self.masked = ("masked:" + kind if masked else kind), cls, shape, hw, masked
        self.K = (2 * hw + 1) ** 3
        self.name = "%s/%s" % (self.kind, tag(shape, hw))
        self.large = (shape, hw) == LARGE[:2]
        self._make, self._ssd, self._seen, self._seeds, self.mask = make, None, None, {}, None
        if masked:
            self.mask = (self._rng(1).random(shape) < 0.6).astype(np.uint8)
            self.mask.setflags(write=False)

    def _rng(self, salt=0):
        return np.random.default_rng([zlib.crc32(self.name.encode()), salt])

    def ssd(self):
        if self._ssd is None:
            ssd = self._make(self._rng(), self.K, self.shape, self.hw)
            assert ssd.shape == (self.K,) + self.shape and ssd.dtype == np.float32 and ssd.flags.c_contiguous, self.name
            if self.masked:
                ssd = ssd.copy()
                col = ssd.reshape(self.K, -1)
                for i, x in enumerate(np.nonzero(self.mask.reshape(-1) == 0)[0]):
                    col[:, x] = np.float32(MASK_POISON[i % 3])
            ssd.setflags(write=False)
            self._ssd = ssd
        return self._ssd

    def seen(self):
        if self._seen is None:
            self._seen = self.ssd()
            if self.masked:
                self._seen = np.where(self.mask[None] != 0, self.ssd(), np.float32(0.0))
                self._seen.setflags(write=False)
        return self._seen

    def seed(self, which):
        if which not in self._seeds:
            s = first_minimum(self.seen()) if which == "true" else self._rng(2).integers(0, self.K, self.shape).astype(np.int64)
            s.setflags(write=False)
            self._seeds[which] = s
        return self._seeds[which]

    def half_ok(self):
        """the operator on half storage takes the volume unchanged"""
        return not self.masked and (self.cls in ("neg_inf", "signed_zeros") or self.kind in ("signed@2^0", "negative@2^0"))

    def __repr__(self):
        return "Case(%s)" % self.name


SEEDS = ("true", "foreign")


def _build():
    cases = []
    for shape, hw, _ in GEOMETRIES:
        cases += [Case(kind, cls, make, shape, hw) for kind, cls, make in KINDS]
        cases += [Case(kind, "masked", make, shape, hw, masked=True) for kind, _, make in KINDS if kind in MASKED_KINDS]
    cases += [Case(kind, cls, make, LARGE[0], LARGE[1]) for kind, cls, make in KINDS if kind in LARGE_KINDS]
    return cases


CASES = _build()
NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)
# every displacement is its own slice at the three shapes of 27 and 125 displacements; 729 displacements over one block of 16-byte columns
# already give slices of two (target 512 slices < K), v = 5120 gives slices of two at 125 displacements
assert [k_slices(s[0] * s[1] * s[2], (2 * hw + 1) ** 3) for s, hw, _ in GEOMETRIES] == [(1, 125), (1, 125), (1, 27), (2, 365)]
assert k_slices(16 * 20 * 16, 125) == (2, 63)


def case(name):
    return CASES[NAMES.index(name)]
