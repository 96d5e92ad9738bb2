"""Pins the restatements that tests/test_gpu_metrics.py grades the evaluation kernels against (csrc/metrics.hip, the histogram kernels of
csrc/edt.hip) to torch, numpy and scipy on the CPU -- no GPU, no capture of the reference: ties, borders, extremes and long rows.

The case builders below (WARP_CASES, JAC_CASES, CONVEX_CASES, percentile_neighbours_f32) are shared with the GPU file, so the oracle is pinned
on exactly the inputs the kernels are graded on.  Inputs come from fixed seeds; no case is skipped or filtered.  Where a reference is
undefined for an input, the input is named here with the reason and graded against the oracle instead (UNDEFINED_IN_ATEN, UNDEFINED_IN_SCIPY)."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

f32 = np.float32


@pytest.fixture(scope="module")
def morc():
    from oracle import metrics_oracle
    return metrics_oracle


# ---- numpy's float32 percentile indices -------------------------------------------------------------------------------------------
def percentile_neighbours_f32(n, q):
    """(k0, k1, virt) of numpy.percentile(method="linear") on n float32 samples at the float32 quantile q (numpy/lib/_function_base_impl.py:
    _quantile, _get_indexes): virt = float32(n-1) * float32(q); both indices are n-1 when virt >= float32(n-1), else floor(virt) and
    floor(virt) + 1.  The one definition of the rule k_hist_order_stats restates (k0 == -2), used by both test files."""
    last = f32(n - 1)
    virt = f32(last * f32(q))
    if virt >= last:
        return n - 1, n - 1, virt
    k0 = int(np.floor(virt))
    return k0, k0 + 1, virt


Q95 = float(np.true_divide(95, f32(100)))                    # what cupy_hd95 passes: numpy's q / float32(100) for float32 data
PERCENTILE_LARGE_M = [3001, 4097, 65537, 1000001, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 24) + 4, (1 << 24) + 5,
                      (1 << 25) + 3]


def check_percentile_rule(m, qs, rng):
    """np.percentile on m random float32 values against the rule: the linear value (what cupy_hd95 restates), and the methods lower and
    higher, which name the two samples one by one.  'higher' is the sample at ceil(virt): the upper neighbour k1 when virt has a fraction,
    and the lower one when virt is a whole number (gamma = 0: the linear value is the lower neighbour then, and k1 carries weight 0).
    Above 2^24 samples lower and higher are not asked: numpy evaluates them from another float32 expression, n q + (1 - q) - 1, which
    rounds differently from float32(n-1) q there (n = 2^24 + 2, q = 1: 'lower' returns the second largest sample) and leaves the data
    at n = 2^24 + 4, q = 1 (ValueError: kth out of bounds).  The linear method has no such case: every float32 >= 2^24 is a whole
    number, so gamma = 0 and the value is the sample k0 alone -- which this check pins."""
    from convexadam_amd.convexAdam_hyper_util import percentile_linear_from_sorted_pair, percentile_neighbours
    x = rng.standard_normal(m).astype(f32)
    s = np.sort(x)
    for q100 in qs:
        q = np.true_divide(q100, f32(100))
        k0, k1, virt = percentile_neighbours_f32(m, q)
        assert 0 <= k0 <= k1 <= m - 1, (m, q100, k0, k1)             # float32(n-1) rounding never sends an index outside the data
        whole = float(virt) == np.floor(float(virt))
        if m <= 1 << 24:
            assert np.percentile(x, q100, method="lower") == s[k0], (m, q100)
            assert np.percentile(x, q100, method="higher") == s[k0 if whole else k1], (m, q100)
        a, b, gamma = percentile_neighbours(m, q100)
        assert (a, b) == (k0, k1), (m, q100)
        got = np.percentile(x, q100)
        assert got.dtype == np.float32 and got == percentile_linear_from_sorted_pair(s[k0], s[k1], gamma), (m, q100)
        if whole:
            assert got == s[k0], (m, q100)
        assert whole or m <= 1 << 24


def test_float32_percentile_rule_equals_numpy_for_every_small_count():
    rng = np.random.default_rng(2024)
    for m in range(1, 3001):
        check_percentile_rule(m, (95,), rng)
    for m in range(1, 200):
        check_percentile_rule(m, (0, 50, 100, 2.5, 99.9), rng)


@pytest.mark.parametrize("m", PERCENTILE_LARGE_M)
def test_float32_percentile_rule_equals_numpy_for_large_counts(m):
    """Counts around 2^24 and 2^25, where float32(n-1) is not n-1: numpy evaluates virt and the bound in float32 there as well, and both
    indices stay inside the data (k1 <= n-1: virt < float32(n-1) implies virt <= float32(n-1) - ulp, and ulp >= 2 there)."""
    check_percentile_rule(m, (95, 0, 50, 100), np.random.default_rng(m))


def test_numpy_lower_and_higher_leave_the_rule_above_2_24():
    """The behaviour of numpy that check_percentile_rule steps around, asserted so that a change of numpy is noticed: at n = 2^24 + 2,
    q = 1, method="lower" returns the second largest sample while the linear value is the largest; at n = 2^24 + 4 it raises."""
    n = (1 << 24) + 4
    x = np.random.default_rng(3).standard_normal(n).astype(f32)
    with pytest.raises(ValueError, match="kth"):
        np.percentile(x, 100, method="lower")
    assert np.percentile(x, 100) == x.max()
    x = x[:n - 2]
    s = np.sort(x)
    assert s[-2] < s[-1]
    assert np.percentile(x, 100, method="lower") == s[-2] and np.percentile(x, 100) == s[-1]


# ---- nearest-neighbour label warp -------------------------------------------------------------------------------------------------
def torch_warp_nearest(seg, disp):
    """F.grid_sample(mode="nearest") on the CPU over the sweep script's sampling grid (convex_run_withconfig.py:96,134,141), float32: the
    identity grid of affine_grid plus the displacement, channels reversed to (x, y, z), divided by half of (extent - 1) per axis."""
    H, W, D = seg.shape
    identity = F.affine_grid(torch.eye(3, 4)[None], (1, 1, H, W, D), align_corners=False)
    half_extent = torch.tensor([D - 1, W - 1, H - 1]) / 2
    offset = torch.from_numpy(np.ascontiguousarray(disp)).flip(0).permute(1, 2, 3, 0) / half_extent
    out = F.grid_sample(torch.from_numpy(np.ascontiguousarray(seg))[None, None], identity + offset[None], mode="nearest", padding_mode="zeros",
                        align_corners=False)
    return out[0, 0].numpy()


def half_voxel_steps(S):
    """The multiples k of half a voxel that the tie cases use along an axis of extent S: +-1 and +-3 (half to even in both parities),
    +-(2S-1) (from voxel 0 exactly onto S - 0.5, from voxel S-1 exactly onto -0.5), and 0."""
    return np.array([0, 1, -1, 3, -3, 2 * S - 1, -(2 * S - 1)])


def tie_displacement(shape, seed):
    """(disp, k): per voxel and axis a random k of half_voxel_steps; disp = k * 0.5 * (S-1)/S voxels, which moves the sample by k/2
    voxels -- exactly, when S is a power of two (every step below is then exact in float32: (S-1)/S, k/S, (2i+1)/S - 1 + k/S, i + k/2)."""
    rng = np.random.default_rng(seed)
    disp = np.empty((3,) + tuple(shape), f32)
    ks = np.empty((3,) + tuple(shape), np.int64)
    for a, S in enumerate(shape):
        ks[a] = rng.choice(half_voxel_steps(S), size=shape)
        disp[a] = ks[a].astype(f32) * f32(0.5) * (f32(S - 1) / f32(S))
    return disp, ks


def label_map(shape, seed, n_labels=9):
    """Random labels 1 .. n_labels-1, never 0: a sample that wrongly lands inside the volume reads a non-zero value."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, n_labels, shape).astype(f32)


def _warp_ties(shape, seed):
    return label_map(shape, seed), tie_displacement(shape, seed + 1)[0]


def _warp_gauss_and_ties(shape, seed):
    seg, disp = _warp_ties(shape, seed)
    rng = np.random.default_rng(seed + 2)
    mix = rng.random((1,) + tuple(shape)) < 0.5
    return seg, np.where(mix, (rng.standard_normal(disp.shape) * 2.5).astype(f32), disp).astype(f32)


def _warp_extreme(shape, seed, values):
    seg, disp = _warp_gauss_and_ties(shape, seed)
    rng = np.random.default_rng(seed + 3)
    where = rng.integers(0, len(values) + 3, disp.shape)            # about len/(len+3) of all components carry one of the values
    for i, v in enumerate(values):
        disp[where == i] = v
    return seg, disp


def _warp_odd_values(shape, seed):
    seg, disp = _warp_gauss_and_ties(shape, seed)
    rng = np.random.default_rng(seed + 4)
    pick = rng.integers(0, 6, shape)
    for i, v in enumerate((1e6, 0.5, -7.0)):                        # no small integers: a gather passes them through unchanged
        seg[pick == i] = v
    return seg, disp


POW2_SHAPES = [(4, 4, 4), (8, 8, 8), (16, 16, 16), (64, 64, 64), (4, 16, 8), (8, 4, 64)]
WARP_CASES = {}
for _s in POW2_SHAPES:
    WARP_CASES["ties-%dx%dx%d" % _s] = (_warp_ties, _s, 11 + sum(_s))
for _s in [(8, 5, 16), (5, 16, 8), (2, 2, 2), (3, 3, 3), (2, 3, 8), (3, 2, 5), (4, 4, 257), (2, 3, 300)]:
    WARP_CASES["mixed-%dx%dx%d" % _s] = (_warp_gauss_and_ties, _s, 23 + sum(_s))
WARP_CASES["huge-8x8x16"] = (lambda s, seed: _warp_extreme(s, seed, (1e30, -1e30)), (8, 8, 16), 31)
WARP_CASES["inf-8x8x16"] = (lambda s, seed: _warp_extreme(s, seed, (np.inf, -np.inf)), (8, 8, 16), 37)
WARP_CASES["inf-huge-4x5x300"] = (lambda s, seed: _warp_extreme(s, seed, (np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9)), (4, 5, 300), 41)
WARP_CASES["values-8x8x8"] = (_warp_odd_values, (8, 8, 8), 43)
WARP_CASES["values-3x5x257"] = (_warp_odd_values, (3, 5, 257), 47)
# ATen's nearest sampler casts std::nearbyint(x) to int64 before its bounds test; for NaN that cast is undefined in C++ (x86 gives
# INT64_MIN: outside, 0; other targets may give 0: voxel 0).  The kernel and the oracle test bounds in float, where NaN is outside: 0.
UNDEFINED_IN_ATEN = {"nan-8x8x16": (lambda s, seed: _warp_extreme(s, seed, (np.nan,)), (8, 8, 16), 53),
                     "nan-inf-2x3x300": (lambda s, seed: _warp_extreme(s, seed, (np.nan, np.inf, -np.inf)), (2, 3, 300), 59)}


def warp_case(name):
    fn, shape, seed = (WARP_CASES.get(name) or UNDEFINED_IN_ATEN[name])
    return fn(shape, seed)


def nan_free_expectation(seg, disp):
    """For the NaN cases: the voxels whose displacement holds a NaN must come out 0 (float bounds test); every other voxel is graded
    against torch, which is defined there.  Returns (torch's result, mask of NaN voxels)."""
    nan = np.isnan(disp).any(0)
    return torch_warp_nearest(seg, np.where(np.isnan(disp), f32(0), disp)), nan


def test_tie_cases_sit_exactly_on_ties_and_on_both_borders():
    """The tie displacements do what their name says (in float64, from k): samples at .5 with an even and with an odd lower neighbour,
    exactly on -0.5 and exactly on S - 0.5, for every power-of-two shape -- and numpy's float32 arithmetic lands on them exactly."""
    for shape in POW2_SHAPES:
        disp, ks = tie_displacement(shape, 12 + sum(shape))
        for a, S in enumerate(shape):
            idx = np.arange(S).reshape([S if b == a else 1 for b in range(3)])
            pos = idx + ks[a] / 2.0
            g = ((2 * idx + 1).astype(f32) / f32(S) - f32(1)) + disp[a] / (f32(S - 1) / f32(2))
            assert g.dtype == np.float32 and np.array_equal((((g + f32(1)) * f32(S)) - f32(1)) / f32(2), pos.astype(f32))
            half = pos[pos != np.floor(pos)]
            lower = np.floor(half)
            inside = (lower >= 0) & (lower < S - 1)
            assert (lower[inside] % 2 == 0).any() and (lower[inside] % 2 == 1).any()
            assert (pos == -0.5).any() and (pos == S - 0.5).any()
            assert (pos == S - 1.5).any() and (pos == 0.5).any()


@pytest.mark.parametrize("name", list(WARP_CASES))
def test_oracle_warp_nearest_equals_torch(morc, name):
    seg, disp = warp_case(name)
    want = torch_warp_nearest(seg, disp)
    got = morc.warp_labels_nearest(seg, disp)
    assert np.array_equal(got, want)
    assert (want != 0).any() and (want == 0).any(), "the case must sample inside and outside the volume"
    if name.startswith(("huge", "inf")):
        far = (np.abs(disp) >= 1e30).any(0)
        assert far.any() and not want[far].any()
    if name.startswith("values"):
        assert {1e6, 0.5, -7.0} <= set(np.unique(want).tolist())


@pytest.mark.parametrize("name", list(UNDEFINED_IN_ATEN))
def test_oracle_warp_nearest_gives_zero_for_nan(morc, name):
    """NaN displacements (undefined in ATen, see UNDEFINED_IN_ATEN): 0 from the oracle at those voxels, torch's value everywhere else."""
    seg, disp = warp_case(name)
    want, nan = nan_free_expectation(seg, disp)
    got = morc.warp_labels_nearest(seg, disp)
    assert nan.any() and not got[nan].any()
    assert np.array_equal(got[~nan], want[~nan]) and got[~nan].any()


# ---- Jacobian statistics ----------------------------------------------------------------------------------------------------------
def jac_reference(j):
    """(std, folding fraction): two-pass float64 std(ddof=1) of log(float64(clip(float32(j + 3), 1e-9f, 1e9f))) and count(j < 0) / n."""
    j = np.asarray(j, f32)
    l = np.log(np.clip((j + f32(3)).astype(f32), f32(1e-9), f32(1e9)).astype(np.float64))
    n = l.size
    with np.errstate(invalid="ignore", divide="ignore"):
        if n > 1:
            mean = l.sum() / n
            std = float(np.sqrt(((l - mean) ** 2).sum() / (n - 1)))
        else:
            std = float("nan")                                       # 0 / 0: torch and numpy both answer nan for one sample
    return std, float(np.count_nonzero(j < 0)) / n


def jac_torch(j):
    """The reference's own expression (convex_run_withconfig.py:148-150), float32 on the CPU."""
    t = torch.from_numpy(np.array(j, f32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                              # torch warns about the degrees of freedom of one sample
        return float(t.add(3).clamp_(1e-9, 1e9).log().std()), float((t < 0).float().mean())


def _near_identity(n, seed):
    return (1 + 1e-3 * np.random.default_rng(seed).standard_normal(n)).astype(f32)


def _jac_plain(n, seed):
    return (1 + 0.3 * np.random.default_rng(seed).standard_normal(n)).astype(f32)     # a registration's spread; a few per mille fold


def _jac_first(n, seed, first):
    j = _near_identity(n, seed)
    j[0] = first
    return j


def jac_clamped(n, seed):
    rng = np.random.default_rng(seed)
    j = _jac_plain(n, seed)
    u = rng.random(n)
    j[u < 0.01] = (-3 - 10 * rng.random(np.count_nonzero(u < 0.01))).astype(f32)      # about 1 % below -3: the lower clamp
    j[u > 0.999] = f32(3e9)                                                           # some above 1e9: the upper clamp
    return j


def _jac_with(n, seed, at, values):
    j = _jac_plain(n, seed)
    for i, v in zip(at, values):
        j[i] = v
    return j


STRIDE = 1024 * 256                                         # threads of k_jacobian_stats' capped grid
JAC_CASES = {}
for _n in (1, 2, 63, 64, 255, 256, 257, STRIDE * 8 - 1, STRIDE * 8, STRIDE * 8 + 1):
    JAC_CASES["n=%d" % _n] = (lambda n=_n: _jac_plain(n, 100 + n % 977))
JAC_CASES["cropped-156x188x220"] = lambda: _jac_plain(156 * 188 * 220, 7)               # 6.45 M: 24.6 strides of the capped grid
JAC_CASES["first=-5"] = lambda: _jac_first(100003, 8, -5.0)                             # l0 = log(1e-9): the lower clamp binds in l0
JAC_CASES["first=2e9"] = lambda: _jac_first(100003, 9, 2e9)                             # l0 = log(1e9): the upper clamp binds in l0
JAC_CASES["first=-5,n=2M"] = lambda: _jac_first(STRIDE * 8 + 1, 10, -5.0)
JAC_CASES["clamped-1%"] = lambda: jac_clamped(300007, 11)
JAC_CASES["constant"] = lambda: np.full(70001, 1.25, f32)
JAC_CASES["constant-folded"] = lambda: np.full(513, -0.5, f32)
JAC_CASES["one-nan"] = lambda: _jac_with(50021, 12, (777,), (np.nan,))
JAC_CASES["first-nan"] = lambda: _jac_with(50021, 13, (0,), (np.nan,))
JAC_CASES["+inf"] = lambda: _jac_with(50021, 14, (5, 40000), (np.inf, np.inf))
JAC_CASES["-inf"] = lambda: _jac_with(50021, 15, (6, 40001), (-np.inf, -np.inf))
JAC_CASES["first=+inf,-inf"] = lambda: _jac_with(50021, 16, (0, 255, 256), (np.inf, -np.inf, -np.inf))
JAC_NAN = {"n=1", "one-nan", "first-nan"}                   # the cases whose standard deviation is nan (in every implementation)


def std_floor(n, ref):
    """Forward bound of a float64 sum of n terms, relative to the result: n * 2^-52 * ref."""
    return n * 2.0 ** -52 * abs(ref)


def torch_std_bound(j):
    """How far torch's float32 evaluation may sit from the two-pass float64 value, from float32 arithmetic alone (u = 2^-24, M = max |l|,
    L = ceil(log2 n) + 2 levels of a blocked float32 sum):
      each logarithm is a float32 within one ulp of log:            |e_i| <= 2 u M
      the float32 mean of n such values:                            |delta| <= L u M
      a standard deviation moves by at most sqrt(n/(n-1)) times the largest change of a term or of the mean,
      and the float32 sum of squares, division and root add         (L + 2) u std.
    The measured distances are 5 to 1000 times inside it; a reference with another offset or another clamp is far outside."""
    j = np.asarray(j, f32)
    l = np.log(np.clip((j + f32(3)).astype(f32), f32(1e-9), f32(1e9)).astype(np.float64))
    n, u = l.size, 2.0 ** -24
    if n < 2 or np.isnan(l).any():
        return float("nan")
    L = int(np.ceil(np.log2(n))) + 2
    return float(np.sqrt(n / (n - 1.0)) * u * np.abs(l).max() * (2 + L) + (L + 2) * u * jac_reference(j)[0])


def std_no_farther_than_torch(got, j):
    """The grading rule for the standard deviation: |got - float64| <= max(|torch float32 - float64|, floor); nan where float64 says nan.
    Returns (ok, distance of got, distance of torch)."""
    ref, _ = jac_reference(j)
    tor, _ = jac_torch(j)
    if np.isnan(ref):
        return bool(np.isnan(got) and np.isnan(tor)), float("nan"), float("nan")
    d_got, d_tor = abs(got - ref), abs(tor - ref)
    return bool(d_got <= max(d_tor, std_floor(np.asarray(j).size, ref))), d_got, d_tor


@pytest.mark.parametrize("name", list(JAC_CASES))
def test_oracle_jacobian_stats_equals_two_pass_float64(morc, name):
    """morc.jacobian_stats == the two-pass float64 expression, and torch's float32 evaluation of the script's expression is within
    torch_std_bound of both (the distances measured per case are in DESIGN 18: they depend on the host's vector log, so the assertion uses
    the bound); the folding fractions are equal, torch's to the one rounding of its float32 mean."""
    j = JAC_CASES[name]()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                              # numpy warns about ddof = n for one sample, and about nan / inf inputs
        std, neg = morc.jacobian_stats(j)
    ref, ref_neg = jac_reference(j)
    assert neg == ref_neg
    assert np.isnan(ref) == (name in JAC_NAN)
    ok, d_orc, d_tor = std_no_farther_than_torch(std, j)
    assert ok, (name, std, ref, d_orc, d_tor)
    if not np.isnan(ref):
        assert std == ref, (name, std, ref)
        tor = jac_torch(j)[0]
        assert d_tor == abs(tor - ref) <= torch_std_bound(j), (name, tor, ref, torch_std_bound(j))     # the float64 value is torch's, to float32 accuracy
        assert abs(std - tor) <= torch_std_bound(j)
        assert abs(jac_torch(j)[1] - ref_neg) <= 2.0 ** -24          # torch's float32 mean of 0/1 values: one rounding of count / n
    if name.startswith("constant"):
        assert ref <= 1e-15                                          # the rounding of the mean: the two-pass value of a constant is not 0


# ---- Dice ---------------------------------------------------------------------------------------------------------------------------
def torch_dice(a, b, max_label):
    """Dice per label 1 .. max_label-1 with torch on the CPU in float32: twice the mean of the joint indicator over 1e-8 plus the two
    indicator means, summed left to right."""
    ta, tb = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1), torch.from_numpy(np.ascontiguousarray(b)).reshape(-1)
    out = []
    for k in range(1, max_label):
        in_a, in_b = ta == k, tb == k
        both = (in_a & in_b).float().mean()
        out.append(2 * both / (1e-8 + in_a.float().mean() + in_b.float().mean()))
    return torch.stack(out).numpy() if out else np.zeros(0, f32)


def dice_pair(n, nl, seed):
    """Two label maps that differ: a random one, and a roll of it with 5 % of its voxels relabelled."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, nl, n).astype(f32)
    b = np.roll(a, 3)
    ch = rng.random(n) < 0.05
    b[ch] = rng.integers(0, nl, np.count_nonzero(ch)).astype(f32)
    return a, b


@pytest.mark.parametrize("n,nl", [(1, 2), (2, 3), (255, 7), (4097, 9), (17160, 14), (300000, 36), (1 << 21, 3)])
def test_oracle_dice_equals_torch(morc, n, nl):
    """Counts below 2^24, where torch's float32 mean of 0/1 values is count / n rounded once (its sum of ones is exact)."""
    a, b = dice_pair(n, nl, n + nl)
    want = torch_dice(a, b, nl)
    assert np.array_equal(morc.dice_coeff(a, b, nl), want)
    if n > 1000:
        assert (want > 0).all() and (want < 1).all()
    assert np.array_equal(morc.dice_coeff(a, a, nl), torch_dice(a, a, nl))
    empty = np.zeros(n, f32)
    assert np.array_equal(morc.dice_coeff(a, empty, nl), torch_dice(a, empty, nl))     # no voxel of any label: 0 / 1e-8-guarded sum


# ---- apply_convex -------------------------------------------------------------------------------------------------------------------
def convex_boundary_field(shape, seed, extras=()):
    """(H,W,D,3) float64 displacements whose sample coordinates (disp + voxel index) sit, per axis, exactly on 0, exactly on n-1, exactly
    on other integers, one ulp outside each border and one ulp inside, plus random ones; `extras` are values written into single
    components (NaN, +-inf).  Also returns the coordinates, for the coverage assertions."""
    rng = np.random.default_rng(seed)
    idn = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), -1)
    coord = np.empty(tuple(shape) + (3,), np.float64)
    for a, S in enumerate(shape):
        last = float(S - 1)
        special = np.array([0.0, last, np.nextafter(0.0, -1.0), np.nextafter(last, np.inf), np.nextafter(0.0, 1.0), np.nextafter(last, -np.inf),
                            float(rng.integers(0, S)), float(S // 2), -1.0, float(S)])
        pick = rng.integers(0, len(special) + 4, shape)
        c = rng.uniform(-1.0, S, shape)
        for i, v in enumerate(special):
            c[pick == i] = v
        coord[..., a] = c
    disp = coord - idn
    # a coordinate the subtraction cannot reproduce (index + disp rounds away from it) is written where it can: index 0 reproduces all
    flat = disp.reshape(-1, 3)
    for i, v in enumerate(extras):
        flat[(7 * i + 3) % len(flat), i % 3] = v
    return disp, disp + idn


CONVEX_CASES = {"13x9x17": ((13, 9, 17), 5), "1x2x5": ((1, 2, 5), 6), "2x1x1": ((2, 1, 1), 7), "2x2x2": ((2, 2, 2), 8), "1x1x1": ((1, 1, 1), 9),
                "1x9x2": ((1, 9, 2), 10)}
# scipy maps a NaN coordinate through comparisons and then an integer cast of floor(NaN): what comes out depends on the build.  The
# kernel and the oracle treat NaN as outside (every comparison with NaN is false): 0.
UNDEFINED_IN_SCIPY = {"13x9x17-nan": ((13, 9, 17), 11), "2x1x3-nan": ((2, 1, 3), 12)}


def convex_trials(name):
    """[(disp, coord, moving)]: one field for the 13x9x17 volume (with +-inf and +-1e300, and NaN in the UNDEFINED_IN_SCIPY cases); 200
    fields for each tiny volume, whose few voxels cannot hold every border at once (the first three carry the extreme values)."""
    shape, seed = (CONVEX_CASES.get(name) or UNDEFINED_IN_SCIPY[name])
    extras = (np.inf, -np.inf, 1e300, -1e300) + ((np.nan, np.nan, np.nan) if name in UNDEFINED_IN_SCIPY else ())
    out = []
    for trial in range(1 if shape == (13, 9, 17) else 200):
        ex = extras if shape == (13, 9, 17) else extras[trial::3][:1] if trial < 3 else ()
        if name in UNDEFINED_IN_SCIPY and shape != (13, 9, 17) and trial % 2:
            ex = (np.nan,)
        disp, coord = convex_boundary_field(shape, 1000 * seed + trial, ex)
        mov = np.random.default_rng(seed + 100 + trial).standard_normal(shape) * 100 + 7
        out.append((disp, coord, mov))
    return out


def scipy_map(disp, mov):
    from scipy.ndimage import map_coordinates
    idn = np.stack(np.meshgrid(*[np.arange(s) for s in mov.shape], indexing="ij"))
    return map_coordinates(mov, disp.transpose(3, 0, 1, 2) + idn, order=1)


def whole_voxel_samples(coord, mov):
    """Mask of the samples that sit exactly on a voxel along every axis, and the values of those voxels."""
    whole = np.all((coord == np.floor(coord)) & (coord >= 0) & (coord <= np.array(mov.shape) - 1.0), -1)
    ii = coord[whole].astype(np.int64)
    return whole, mov[ii[:, 0], ii[:, 1], ii[:, 2]]


def test_convex_cases_reach_every_border():
    (disp, coord, _), = convex_trials("13x9x17")
    for a, S in enumerate((13, 9, 17)):
        c = coord[..., a]
        for v in (0.0, S - 1.0, np.nextafter(0.0, -1.0), np.nextafter(S - 1.0, np.inf), np.nextafter(0.0, 1.0), np.nextafter(S - 1.0, -np.inf)):
            assert (c == v).any(), (a, v)
        assert ((c == np.floor(c)) & (c > 0) & (c < S - 1)).any()
    inside = np.all((coord >= 0) & (coord <= np.array([12.0, 8.0, 16.0])), -1)
    assert inside.any() and (~inside).any()
    assert np.isposinf(disp).any() and np.isneginf(disp).any()
    for name in CONVEX_CASES:
        trials = convex_trials(name)
        assert any(whole_voxel_samples(c, m)[0].any() for d, c, m in trials), name       # an extent of 1 is inside only at exactly 0
        assert any(np.isinf(d).any() for d, c, m in trials), name
    for name in UNDEFINED_IN_SCIPY:
        assert any(np.isnan(d).any() for d, c, m in convex_trials(name)), name


@pytest.mark.parametrize("name", list(CONVEX_CASES))
def test_oracle_apply_convex_equals_scipy_on_borders(morc, name):
    nonzero = False
    for disp, coord, mov in convex_trials(name):
        want = scipy_map(disp, mov)
        assert np.array_equal(morc.apply_convex(disp, mov), want)
        nonzero |= bool((want != 0).any())
        whole, vox = whole_voxel_samples(coord, mov)                 # exactly on a voxel along every axis: the voxel itself, unrounded
        assert np.array_equal(want[whole], vox)
    assert nonzero


@pytest.mark.parametrize("name", list(UNDEFINED_IN_SCIPY))
def test_oracle_apply_convex_gives_zero_for_nan(morc, name):
    """NaN coordinates (see UNDEFINED_IN_SCIPY): 0 from the oracle; every other sample equals scipy on the field with the NaNs replaced."""
    seen = False
    for disp, coord, mov in convex_trials(name):
        nan = np.isnan(disp).any(-1)
        got = morc.apply_convex(disp, mov)
        assert not got[nan].any()
        want = scipy_map(np.where(np.isnan(disp), 0.0, disp), mov)
        assert np.array_equal(got[~nan], want[~nan])
        seen |= bool(nan.any())
    assert seen
