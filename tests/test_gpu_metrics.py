"""GPU tests of the evaluation kernels the sweep ranks settings by (csrc/metrics.hip; k_edt_sqdist, k_surface_hist and k_hist_order_stats
of csrc/edt.hip) against float64 / numpy / scipy / torch-CPU references, at the sizes and values where such kernels go wrong: one element,
one wavefront +- 1, one sweep of the capped grid +- 1, the full volume; both clamps, NaN, +-inf; exact rounding ties and samples exactly on
a border; order statistics on chunk edges; both load widths.  Every comparison is exact unless its test says otherwise.

The inputs and the CPU references come from tests/test_oracle_metrics.py, which pins the oracle's restatements on the same inputs."""
import numpy as np
import pytest
import torch

import test_oracle_metrics as cases  # shared case builders and CPU references (tests/ is on the path: rootdir-style imports); its own tests need no GPU

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def HU():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import convexAdam_hyper_util
    return convexAdam_hyper_util


@pytest.fixture(scope="module")
def morc():
    from oracle import metrics_oracle
    return metrics_oracle


def api():
    from convexadam_amd._lib import CvxError, check, lib, ptr, stream_ptr
    return lib(), check, ptr, stream_ptr(torch.device(DEV)), CvxError


# ---- Jacobian statistics ------------------------------------------------------------------------------------------------------------
JAC_GRID = 1024 * 256                                       # threads of the capped grid of k_jacobian_stats (one sweep = 8 x this many values)


@pytest.mark.parametrize("name", list(cases.JAC_CASES))
def test_jacobian_stats_vs_float64(HU, name):
    """The folding fraction equals count(j < 0) / n (an integer count in a double; NaN counts as not folded, like j < 0).  The standard
    deviation is graded against the two-pass float64 value with torch's own float32 evaluation of the reference's expression as the
    yardstick: the kernel must be at least as close as torch is (floor: n 2^-52 of the value, the forward bound of a float64 sum of n
    terms).  Where float64 says nan (one sample, a NaN among the values) the kernel says nan.  The distances are printed."""
    j = cases.JAC_CASES[name]()
    n = j.size
    ref, ref_neg = cases.jac_reference(j)
    std, neg = HU.jacobian_log_std_and_folding(dev(j))
    assert neg == ref_neg
    L, check, ptr, sp, _ = api()
    jd, acc = dev(j), torch.full((3,), 7.0, dtype=torch.float64, device=DEV)
    check(L.cvx_jacobian_stats_f64(ptr(jd), n, ptr(acc), sp))
    s, s2, cnt = [float(v) for v in host(acc)]
    assert cnt == float(np.count_nonzero(j < 0))
    ok, d_kernel, d_torch = cases.std_no_farther_than_torch(std, j)
    print("JACSTD %-22s n=%8d ref=%.17g kernel-ref=%.3e torch-ref=%.3e floor=%.3e" % (name, n, ref, d_kernel, d_torch, cases.std_floor(n, ref)))
    assert ok, (name, std, ref, d_kernel, d_torch)
    assert np.isnan(std) == (name in cases.JAC_NAN)
    if not np.isnan(ref):
        assert d_torch <= cases.torch_std_bound(j)                   # the yardstick itself is bounded: float32 accuracy, not more
    if name.startswith("constant"):
        assert std == 0.0 and s == 0.0 and s2 == 0.0                 # every term is l - l0 = 0 exactly
    if n == 1:
        assert np.isnan(cases.jac_torch(j)[0]) and s == 0.0 and s2 == 0.0   # torch: nan for one sample; the sums themselves are fine


def test_jacobian_stats_accepts_a_cropped_volume_tensor(HU):
    """The wrapper flattens a (H-4, W-4, D-4) tensor as the sweep passes it, and a non-contiguous view of the same values: the same
    folding fraction, and a standard deviation graded like every other (the order of the workgroups' atomics is free, so two runs need
    not agree bit for bit)."""
    j = cases.jac_clamped(20 * 24 * 28, 3).reshape(20, 24, 28)
    for t in (dev(j), dev(j.transpose(2, 0, 1).copy()).permute(1, 2, 0)):
        std, neg = HU.jacobian_log_std_and_folding(t)
        assert neg == cases.jac_reference(j)[1]
        ok, d_kernel, d_torch = cases.std_no_farther_than_torch(std, j)
        assert ok and d_torch <= cases.torch_std_bound(j), (std, d_kernel, d_torch)
    assert not t.is_contiguous()


# ---- label overlap ------------------------------------------------------------------------------------------------------------------
def overlap_reference(a, b, nl):
    """np.bincount over the values that are exact integers in [0, nl): rows |a == l|, |b == l|, |a == l and b == l|."""
    def labels(x):
        with np.errstate(invalid="ignore"):
            ok = (x >= 0) & (x < nl) & (x == np.floor(x))
        return np.where(ok, x, -1).astype(np.int64)
    la, lb = labels(np.asarray(a, f32).reshape(-1)), labels(np.asarray(b, f32).reshape(-1))
    return np.stack([np.bincount(la[la >= 0], minlength=nl), np.bincount(lb[lb >= 0], minlength=nl),
                     np.bincount(la[(la >= 0) & (la == lb)], minlength=nl)]).astype(np.int64)


OVERLAP_SWEEP = 1024 * 256 * 16                             # voxels one sweep of k_label_overlap's capped grid covers


def _odd_values(n, nl, seed):
    a, b = cases.dice_pair(n, nl, seed)
    rng = np.random.default_rng(seed + 1)
    odd = np.array([2.5, -1.0, -0.0, np.nan, np.inf, -np.inf, nl, nl + 0.5], f32)
    for m in (a, b):
        at = rng.random(n) < 0.3
        m[at] = rng.choice(odd, np.count_nonzero(at))
    return a, b


OVERLAP_CASES = {}
for _n in (1, 255, 4097, OVERLAP_SWEEP - 1, OVERLAP_SWEEP, OVERLAP_SWEEP + 1):
    OVERLAP_CASES["n=%d" % _n] = (_n, 9, cases.dice_pair)
for _nl in (14, 36):
    OVERLAP_CASES["160x192x224-%d" % _nl] = (160 * 192 * 224, _nl, cases.dice_pair)     # 1.64 sweeps: the stride loop wraps
for _nl in (1, 2, 255, 4096):
    OVERLAP_CASES["labels=%d" % _nl] = (100003, _nl, cases.dice_pair)
OVERLAP_CASES["odd-values"] = (50021, 6, _odd_values)
OVERLAP_CASES["odd-values-1-label"] = (4097, 1, _odd_values)
OVERLAP_CASES["one-label-holds-all"] = (OVERLAP_SWEEP + 1, 9, lambda n, nl, seed: (np.full(n, 3, f32), np.full(n, 3, f32)))
OVERLAP_CASES["last-label-holds-all"] = (300007, 4096, lambda n, nl, seed: (np.full(n, 4095, f32), np.full(n, 4095, f32)))


@pytest.mark.parametrize("name", list(OVERLAP_CASES))
def test_label_overlap_counts_vs_bincount(HU, morc, name):
    """All three rows of label_overlap_counts == np.bincount (two maps that differ), and dice_coeff == the oracle's restatement of
    hyper_util.py:53-60 from them.  Values that are no label in 0 .. num_labels-1 (2.5, -1, NaN, +-inf, num_labels, num_labels + 0.5)
    are counted nowhere; -0.0 is label 0."""
    n, nl, make = OVERLAP_CASES[name]
    a, b = make(n, nl, 17 + nl)
    want = overlap_reference(a, b, nl)
    got = HU.label_overlap_counts(dev(a), dev(b), nl)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if name.startswith("odd"):
        assert want[0].sum() < n and want[1].sum() < n and want[0, 0] > np.count_nonzero((a == 0) & ~np.signbit(a))   # -0.0 counted as 0
    elif not name.endswith("holds-all"):
        assert want[0].sum() == n and want[1].sum() == n and (n < 1000 or nl == 1 or 0 < want[2].sum() < n)
    if nl > 1 and n <= 1 << 24:
        with np.errstate(invalid="ignore"):
            d = HU.dice_coeff(dev(a), dev(b), nl).numpy()
            assert np.array_equal(d, morc.dice_coeff(a, b, nl))
            assert np.array_equal(HU.dice_coeff(dev(a), dev(b), nl, counts=got).numpy(), d)


def test_label_overlap_refuses_label_counts_outside_1_to_4096(HU):
    L, check, ptr, sp, CvxError = api()
    a = dev(np.zeros(100, f32))
    counts = torch.zeros(3 * 4097, dtype=torch.int64, device=DEV)
    for nl in (4097, 0, -1):
        with pytest.raises(CvxError, match="not in 1..4096"):
            check(L.cvx_label_overlap_i64(ptr(a), ptr(a), 100, nl, ptr(counts), sp))
    with pytest.raises(CvxError, match="not in 1..4096"):
        HU.label_overlap_counts(a, a, 4097)
    with pytest.raises(CvxError, match="cvx_label_overlap_i64"):      # no labels, no counts array: refused one check earlier
        HU.label_overlap_counts(a, a, 0)
    assert np.array_equal(HU.label_overlap_counts(a, a, 4096)[:, :2], [[100, 0]] * 3)     # the library is usable after a refusal


@pytest.mark.parametrize("bad", [2.5, -1.0, np.nan, np.inf, -np.inf, 4.0, 4.5])
def test_hd95_raises_on_values_that_are_no_class(HU, bad):
    """cupy_hd95's range check rests on the overlap counts: a value F.one_hot would refuse (or could not be cast for) raises the
    RuntimeError of hyper_util.py:33 on both methods, in the fixed and in the moving map; -0.0 is class 0 and passes."""
    nl = 3
    rng = np.random.default_rng(5)
    a = rng.integers(0, nl + 1, (12, 10, 14)).astype(f32)
    b = np.roll(a, 1, 2)
    bad_map = a.copy()
    bad_map[3, 4, 5] = bad
    for method in ("surface", "edt"):
        for fx, mv in ((bad_map, b), (b, bad_map)):
            with pytest.raises(RuntimeError, match="class values must be in 0"):
                HU.cupy_hd95(dev(fx), dev(mv), nl, method=method)
    zero = a.copy()
    zero[a == 0] = -0.0
    assert np.signbit(zero).any()
    assert np.array_equal(host(HU.cupy_hd95(dev(zero), dev(b), nl)), host(HU.cupy_hd95(dev(a), dev(b), nl)))


# ---- nearest-neighbour label warp ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.WARP_CASES))
def test_warp_labels_nearest_vs_torch_cpu(HU, morc, name):
    """k_warp_nearest == F.grid_sample(mode="nearest") on the CPU, on the grid the sweep script builds, and == the oracle: exact ties in both
    parities, samples exactly on -0.5 (rounds into the volume) and on S - 0.5 (rounds out of it), extents 2 and 3, rows longer than a
    workgroup, displacements of +-1e30 and +-inf (0), label values that are no small integers (unchanged)."""
    seg, disp = cases.warp_case(name)
    got = host(HU.warp_labels_nearest(dev(seg), dev(disp)[None]))
    assert np.array_equal(got, cases.torch_warp_nearest(seg, disp))
    assert np.array_equal(got, morc.warp_labels_nearest(seg, disp))
    assert got.any() and not got.all()
    if name.startswith(("huge", "inf")):
        assert not got[(np.abs(disp) >= 1e30).any(0)].any()


@pytest.mark.parametrize("name", list(cases.UNDEFINED_IN_ATEN))
def test_warp_labels_nearest_gives_zero_for_nan(HU, morc, name):
    """A NaN displacement gives 0 (the kernel tests bounds in float before the integer cast).  Graded against the oracle: ATen casts
    nearbyint(NaN) to int64 first, which C++ leaves undefined (tests/test_oracle_metrics.py::UNDEFINED_IN_ATEN).  The voxels without a
    NaN are graded against torch as well."""
    seg, disp = cases.warp_case(name)
    got = host(HU.warp_labels_nearest(dev(seg), dev(disp)[None]))
    assert np.array_equal(got, morc.warp_labels_nearest(seg, disp))
    want, nan = cases.nan_free_expectation(seg, disp)
    assert nan.any() and not got[nan].any() and np.array_equal(got[~nan], want[~nan])


def test_warp_labels_nearest_refuses_an_extent_of_one(HU):
    _, _, _, _, CvxError = api()
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):
        with pytest.raises(CvxError, match="bad extent"):
            HU.warp_labels_nearest(dev(np.ones(shape, f32)), dev(np.zeros((1, 3) + shape, f32)))


# ---- order statistics and percentile of a histogram -----------------------------------------------------------------------------------
def order_stat_reference(sparse, k):
    """Bin of the k-th smallest entry (0-based) of the histogram {bin: count}, by a cumulative sum in Python integers; -1 outside."""
    run = 0
    if k >= 0:
        for b in sorted(sparse):
            c = int(sparse[b])
            if c and k < run + c:
                return b
            run += c
    return -1


def total(sparse):
    return sum(int(c) for c in sparse.values())


def dense(nbins, sparse):
    h = np.zeros(nbins, np.int64)
    for b, c in sparse.items():
        h[b] = c
    return h


def split_at_neighbours(m, lo_bin, hi_bin, q=cases.Q95):
    """m entries: those up to the lower neighbour k0 of the quantile in lo_bin, the rest (from k1 on) in hi_bin."""
    k0, _, _ = cases.percentile_neighbours_f32(m, q)
    return {lo_bin: k0 + 1, hi_bin: m - k0 - 1} if m - k0 - 1 else {lo_bin: m}


def _order_cases():
    out = {}
    for nb in (1, 2, 1023, 1024, 1025, 16 * 1024 - 1, 16 * 1024, 16 * 1024 + 1, 111000, 4096 * 1024):
        out["%d-first" % nb] = (nb, {0: 21})
        out["%d-last" % nb] = (nb, {nb - 1: 21})
        if nb > 1:
            out["%d-ends" % nb] = (nb, {0: 20, nb - 1: 1})                        # k0 in bin 0, k1 in the last bin: every chunk between is empty
            rng = np.random.default_rng(nb)
            out["%d-random" % nb] = (nb, {int(b): int(rng.integers(0, 40)) for b in rng.integers(0, nb, 50)})
    nb = 111000                                                                     # cupy_hd95 at 160 x 192 x 224
    for m in (2, 20, 21, 1000):
        out["edge-adjacent-%d" % m] = (nb, split_at_neighbours(m, 1023, 1024))      # k0 = last entry of chunk 0 (lane 63, slot 15), k1 = first of chunk 1
        out["edge-gap-%d" % m] = (nb, split_at_neighbours(m, 2047, 5 * 1024))       # chunks 2 .. 4 hold nothing
        out["edge-same-lane-%d" % m] = (nb, split_at_neighbours(m, 16 * 1024 + 1008, 16 * 1024 + 1023))   # slots 0 and 15 of lane 63, second round of wave 0
        out["edge-last-slot-%d" % m] = (nb, {17 * 1024 + 1023: m})
    out["empty"] = (4097, {})
    for m in (1, 2, 20, 21, 1 << 24, (1 << 24) + 3, 3 * 10 ** 9):
        out["count-%d" % m] = (4097, {5: m // 3, 1023: m // 3, 3000: m - 2 * (m // 3)})
    out["count-2^24+3-two-bins"] = (4097, {7: (1 << 24) + 2, 4096: 1})             # only the very last entry in the upper bin
    return out


ORDER_CASES = _order_cases()
QUANTILES = (cases.Q95, 0.0, 0.5, 1.0)


def run_order_stats(hd, nbins, k0, k1):
    L, check, ptr, sp, _ = api()
    out = torch.full((3,), -9, dtype=torch.int64, device=DEV)
    check(L.cvx_hist_order_stats_i64(ptr(hd), nbins, k0, k1, ptr(out), sp))
    return [int(v) for v in host(out)]


def run_percentile(hd, nbins, q, n_hist=None):
    L, check, ptr, sp, _ = api()
    out = torch.full((3 * (n_hist or 1),), -9, dtype=torch.int64, device=DEV)
    if n_hist is None:
        check(L.cvx_hist_percentile_neighbours_i64(ptr(hd), nbins, q, ptr(out), sp))
        return [int(v) for v in host(out)]
    check(L.cvx_hist_percentile_neighbours_batch_i64(ptr(hd), nbins, n_hist, q, ptr(out), sp))
    return host(out).reshape(n_hist, 3).tolist()


def percentile_reference(sparse, q):
    m = total(sparse)
    if m == 0:
        return [-1, -1, 0]
    k0, k1, _ = cases.percentile_neighbours_f32(m, q)
    return [order_stat_reference(sparse, k0), order_stat_reference(sparse, k1), m]


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_hist_percentile_neighbours_vs_python_integers(HU, name):
    """out3 = (bin of the k0-th entry, bin of the k1-th entry, count) with k0, k1 by numpy's float32 rule (pinned to np.percentile in
    tests/test_oracle_metrics.py) and the bins by a Python-integer cumulative sum, for q = 0.95f as cupy_hd95 passes it, 0, 0.5 and 1.
    Up to 2 million entries the value cupy_hd95 composes from out3 equals np.percentile of the float32 sample sqrt(bins), bit for bit.
    The explicit order statistics (cvx_hist_order_stats_i64) are asked at the same neighbours, at both ends and outside the data (-1)."""
    nbins, sparse = ORDER_CASES[name]
    hd = dev(dense(nbins, sparse))
    m = total(sparse)
    for q in QUANTILES:
        want = percentile_reference(sparse, q)
        assert run_percentile(hd, nbins, q) == want, (name, q)
        assert run_percentile(hd, nbins, q, n_hist=1) == [want], (name, q)
    if 0 < m <= 2 * 10 ** 6:
        bins = np.array(sorted(sparse), np.int64)
        sample = np.sqrt(np.repeat(bins, [sparse[b] for b in bins]).astype(np.float64)).astype(f32)
        out3 = np.array([[run_percentile(hd, nbins, cases.Q95)] * 2], np.int64)
        got = float(HU._hd95_from_order_stats(out3, [1], 1, 1, torch.device(DEV))[0])
        want = np.percentile(sample, 95)
        assert want.dtype == np.float32 and got == float(want), (name, got, want)
    k0, k1, _ = cases.percentile_neighbours_f32(max(m, 1), cases.Q95)
    for a, b in ((k0, k1), (0, m - 1), (m - 1, m), (-1, 0), (m, m + 5), (-7, -3), (m // 2, m // 2)):   # (-2 is the ABI's "by quantile" mark)
        want = [order_stat_reference(sparse, a), order_stat_reference(sparse, b), m]
        assert run_order_stats(hd, nbins, a, b) == want, (name, a, b)
    if m == 0:
        assert run_percentile(hd, nbins, cases.Q95) == [-1, -1, 0]


@pytest.mark.parametrize("nbins", [1025, 111000])
@pytest.mark.parametrize("n_hist", [1, 2, 26])
def test_hist_percentile_batch_equals_single_calls(nbins, n_hist):
    """1, 2 and 26 histograms in one launch (26 = 13 labels x 2 directions) == the single calls == the reference."""
    pool = [s for nb, s in ORDER_CASES.values() if all(b < nbins for b in s) and total(s) < 10 ** 6]
    rng = np.random.default_rng(nbins + n_hist)
    pick = [pool[i] for i in rng.integers(0, len(pool), n_hist - 1)] + [{}]                  # the last one empty
    assert len(pool) >= 10
    rows = np.stack([dense(nbins, s) for s in pick])
    hd = dev(rows)
    for q in QUANTILES:
        got = run_percentile(hd, nbins, q, n_hist=n_hist)
        assert got == [percentile_reference(s, q) for s in pick]
        assert got == [run_percentile(hd[i], nbins, q) for i in range(n_hist)]
    assert got[-1] == [-1, -1, 0]


def test_hist_order_stats_bin_limit():
    """4 194 304 bins are accepted (in ORDER_CASES); one more is refused, by both entry points."""
    L, check, ptr, sp, CvxError = api()
    hd = torch.zeros(4096 * 1024 + 1, dtype=torch.int64, device=DEV)
    out = torch.zeros(3, dtype=torch.int64, device=DEV)
    with pytest.raises(CvxError, match="bad size"):
        check(L.cvx_hist_order_stats_i64(ptr(hd), 4096 * 1024 + 1, 0, 0, ptr(out), sp))
    with pytest.raises(CvxError, match="bad arguments"):
        check(L.cvx_hist_percentile_neighbours_i64(ptr(hd), 4096 * 1024 + 1, 0.5, ptr(out), sp))
    assert (4096 * 1024, {0: 21}) == ORDER_CASES["4194304-first"]


# ---- surface histogram and squared distance -------------------------------------------------------------------------------------------
SURF_LDS_BINS = 2048                                        # k_surface_hist keeps the bins below this in LDS
SURF_GRID = 2048 * 256                                      # threads of its capped grid
SURF_SIZES = (1, 3, 4, 5, 1027, 4 * SURF_GRID + 5)          # the last: the 16-byte loop wraps once, the 4-byte loop four times
SURF_BINS = (100, 2048, 2049, 5000)
SURF_OFFSETS = (0, 1, 2, 3)                                 # base address of every volume: 16-byte aligned + 4 x this


def surface_inputs(n, nbins, seed, overflow):
    """(a_in2, a_out2, b_in2) int32: b_in2 == 1 on about 40 % of the voxels (all, when n <= 5); the squared distance a_in2 + a_out2 (one
    of the two is 0) on both sides of 2047 / 2048 and at both ends of the histogram.  overflow: some surface voxels carry nbins or a
    negative value.  Voxels off the surface carry out-of-range values in either case (they must not raise the flag)."""
    rng = np.random.default_rng(seed)
    b = rng.choice(np.array([0, 1, 1, 2, 3], np.int32), n)
    if n <= 5:
        b[:] = 1
    marks = np.array([0, 1, min(2046, nbins - 1), min(2047, nbins - 1), min(2048, nbins - 1), min(2049, nbins - 1), nbins - 1, nbins // 2])
    d = np.where(rng.random(n) < 0.6, rng.choice(marks, n), rng.integers(0, nbins, n)).astype(np.int32)
    if overflow:
        u = rng.random(n)
        d[u < 0.1] = nbins
        d[u > 0.9] = -1
        d[0] = nbins if seed % 2 else -1
    off = b != 1
    d[off] = np.where(rng.random(n) < 0.5, nbins + 3, -5)[off]
    inner = rng.random(n) < 0.5
    return np.where(inner, d, 0).astype(np.int32), np.where(inner, 0, d).astype(np.int32), b


def surface_reference(a_in, a_out, b, nbins):
    sel = b == 1
    bins = a_in.astype(np.int64) + a_out
    valid = (bins >= 0) & (bins < nbins)
    hist = np.zeros(nbins, np.int64)
    np.add.at(hist, bins[sel & valid], 1)
    return hist, int((sel & ~valid).any())


def place(vols, off):
    """The volumes as slices of ONE allocation, each starting 4 * off bytes after a 16-byte boundary."""
    n = len(vols[0])
    slot = (n + 3) // 4 * 4 + 4
    buf = torch.zeros(len(vols) * slot + 4, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = []
    for i, v in enumerate(vols):
        t = buf[i * slot + off: i * slot + off + n]
        t.copy_(torch.from_numpy(v))
        assert t.data_ptr() % 16 == 4 * off
        out.append(t)
    return buf, out


def surface_case_ids():
    return [(n, nbins, off, ov) for n in SURF_SIZES for nbins in SURF_BINS for off in SURF_OFFSETS for ov in (False, True)
            if n < 10 ** 6 or (nbins == 5000 and off in (0, 3))]


@pytest.mark.parametrize("n,nbins,off,overflow", surface_case_ids())
def test_surface_hist_vs_numpy(n, nbins, off, overflow):
    """k_surface_hist == np.add.at over the voxels with b_in2 == 1, for every alignment of the three volumes (16-byte loads with a 4-byte
    tail / 4-byte loads throughout), bins in LDS and in global memory; a bin equal to nbins or negative on the surface sets the flag
    and is not counted; a run without one leaves the flag 0."""
    L, check, ptr, sp, _ = api()
    a_in, a_out, b = surface_inputs(n, nbins, n + nbins + off, overflow)
    want, want_flag = surface_reference(a_in, a_out, b, nbins)
    assert want_flag == int(overflow)
    buf, (ta, to, tb) = place((a_in, a_out, b), off)
    hist = torch.full((nbins,), 3, dtype=torch.int64, device=DEV)
    flag = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    check(L.cvx_surface_hist_i64(ptr(ta), ptr(to), ptr(tb), n, nbins, ptr(hist), ptr(flag), sp))
    assert np.array_equal(host(hist), want)
    assert int(host(flag)[0]) == want_flag
    assert want.sum() > 0 or overflow


@pytest.mark.parametrize("n_hist", [1, 7])
@pytest.mark.parametrize("n,nbins", [(5, 100), (1027, 2049), (40003, 5000)])
def test_surface_hist_batch_equals_single_calls(n_hist, n, nbins):
    """One launch over a device table of 1 and of 7 (a_in2, a_out2, b_in2) triples == the single calls == numpy; triple h sits 4 * (h % 4)
    bytes after a 16-byte boundary, and every second one overflows (flags are per histogram)."""
    L, check, ptr, sp, _ = api()
    keep, tab, want, want_flags = [], [], [], []
    for h in range(n_hist):
        vols = surface_inputs(n, nbins, 50 + h, overflow=bool(h % 2))
        buf, ts = place(vols, h % 4)
        keep.append(buf)
        tab += [t.data_ptr() for t in ts]
        hist, fl = surface_reference(*vols, nbins)
        want.append(hist)
        want_flags.append(fl)
        single, sflag = torch.empty(nbins, dtype=torch.int64, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
        check(L.cvx_surface_hist_i64(ptr(ts[0]), ptr(ts[1]), ptr(ts[2]), n, nbins, ptr(single), ptr(sflag), sp))
        assert np.array_equal(host(single), hist) and int(host(sflag)[0]) == fl
    tab_d = torch.tensor(tab, dtype=torch.int64).to(DEV)
    hists = torch.full((n_hist, nbins), 3, dtype=torch.int64, device=DEV)
    flags = torch.full((n_hist,), 5, dtype=torch.int32, device=DEV)
    check(L.cvx_surface_hist_batch_i64(ptr(tab_d), n_hist, n, nbins, ptr(hists), ptr(flags), sp))
    assert np.array_equal(host(hists), np.stack(want))
    assert host(flags).tolist() == want_flags == [h % 2 for h in range(n_hist)]


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 4, 5), (2, 3, 300), (5, 1, 257), (16, 16, 16)])
def test_edt_sqdist_vs_numpy(shape):
    """cvx_edt_sqdist_i32 == sum((feat - idx)**2) where obj != 0 and 0 elsewhere; obj holds 0, -0.0 (both "zero"), NaN and values that
    are not 1 (all "not zero"); feat is any in-range coordinate table, not a transform's."""
    L, check, ptr, sp, _ = api()
    H, W, D = shape
    rng = np.random.default_rng(sum(shape))
    obj = rng.choice(np.array([0.0, -0.0, 1.0, 2.5, -3.0, np.nan], f32), shape)
    feat = np.stack([rng.integers(0, s, shape) for s in shape]).astype(np.int32)
    idx = np.stack(np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing="ij"))
    want = np.where(obj != 0, ((feat.astype(np.int64) - idx) ** 2).sum(0), 0).astype(np.int32)
    out = torch.full(shape, -1, dtype=torch.int32, device=DEV)
    od, fd = dev(obj), dev(feat)
    check(L.cvx_edt_sqdist_i32(ptr(od), ptr(fd), H, W, D, ptr(out), sp))
    assert np.array_equal(host(out), want)
    assert H * W * D == 1 or ((want > 0).any() and (want == 0).any())


# ---- apply_convex ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CONVEX_CASES))
def test_apply_convex_vs_scipy_on_borders(name):
    """k_map_linear_f64 == scipy.ndimage.map_coordinates(order=1) where a coordinate is exactly 0, exactly n-1 (the upper tap clamps),
    exactly another integer, one ulp outside and inside each border, +-inf and +-1e300; volumes with extents of 1 and 2."""
    from convexadam_amd.apply_convex import apply_convex
    for disp, coord, mov in cases.convex_trials(name):
        got = apply_convex(disp, mov)
        assert got.dtype == np.float64 and np.array_equal(got, cases.scipy_map(disp, mov))
        whole, vox = cases.whole_voxel_samples(coord, mov)
        assert np.array_equal(got[whole], vox)


@pytest.mark.parametrize("name", list(cases.UNDEFINED_IN_SCIPY))
def test_apply_convex_gives_zero_for_nan(morc, name):
    """NaN coordinates give 0.  Graded against the oracle: scipy's own answer for NaN rests on an integer cast of NaN and is
    platform-defined (tests/test_oracle_metrics.py::UNDEFINED_IN_SCIPY); the samples without NaN are graded against scipy too."""
    from convexadam_amd.apply_convex import apply_convex
    for disp, coord, mov in cases.convex_trials(name):
        got = apply_convex(disp, mov)
        assert np.array_equal(got, morc.apply_convex(disp, mov))
        nan = np.isnan(disp).any(-1)
        assert not got[nan].any()
        assert np.array_equal(got[~nan], cases.scipy_map(np.where(np.isnan(disp), 0.0, disp), mov)[~nan])


# ---- Jacobian determinant -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("convert1", [False, True])
@pytest.mark.parametrize("shape,special", [((5, 5, 5), False), ((5, 5, 300), False), ((5, 6, 5), False), ((6, 5, 5), False), ((5, 5, 5), True),
                                           ((9, 8, 70), True), ((5, 5, 300), True)])
def test_jacobian_determinant_small_extents_and_non_finite(HU, morc, shape, special, convert1):
    """Extents of exactly 5 (one output voxel per axis), a row beyond a workgroup, and fields holding +-inf and NaN: equal to the oracle
    including where the NaNs are."""
    rng = np.random.default_rng(sum(shape) + special)
    flow = (rng.standard_normal((3,) + shape) * (0.1 if convert1 else 2.0)).astype(f32)
    if special:
        at = rng.integers(0, 12, flow.shape)
        for i, v in enumerate((np.inf, -np.inf, np.nan)):
            flow[at == i] = v
    with np.errstate(invalid="ignore"):
        want = morc.jacobian_determinant_3d(flow, convert1)
    got = host(HU.jacobian_determinant_3d(dev(flow)[None], convert1))
    assert got.shape == tuple(s - 4 for s in shape)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isfinite(want).all() != special


# ---- what the parametrisation reaches ---------------------------------------------------------------------------------------------------
def test_cases_reach_every_kernel_branch():
    """From the parametrisation alone: a stride loop that wraps (k_jacobian_stats, k_label_overlap, both loops of k_surface_hist) and one
    that does not; both load widths of k_surface_hist and its tail; bins in LDS and in global memory, on the surface; order statistics in
    the same chunk and in different chunks, with empty chunks between, and a target at lane 63, slot 15; both clamps of jac_log, in the
    shift l0 and in the body."""
    sizes = {name: cases.JAC_CASES[name]().size for name in cases.JAC_CASES if not name.startswith("cropped")}
    assert max(sizes.values()) > 8 * JAC_GRID and 156 * 188 * 220 > 3 * 8 * JAC_GRID
    assert {1, 2, 63, 64, 255, 256, 257, 8 * JAC_GRID - 1, 8 * JAC_GRID, 8 * JAC_GRID + 1} <= set(sizes.values())
    lo, hi = cases.JAC_CASES["first=-5"](), cases.JAC_CASES["first=2e9"]()
    assert lo[0] + f32(3) < f32(1e-9) and hi[0] + f32(3) > f32(1e9)
    assert not ((lo[1:] + f32(3) < f32(1e-9)) | (hi[1:] + f32(3) > f32(1e9))).any()          # ... and only there: l0 is the outlier
    body = cases.JAC_CASES["clamped-1%"]()
    assert 0.005 < np.mean(body + f32(3) < f32(1e-9)) < 0.02 and (body + f32(3) > f32(1e9)).any()
    ns = {n for n, _, _ in OVERLAP_CASES.values()}
    assert {1, 255, 4097, OVERLAP_SWEEP - 1, OVERLAP_SWEEP, OVERLAP_SWEEP + 1, 160 * 192 * 224} <= ns
    assert {1, 2, 255, 4096, 14, 36} <= {nl for _, nl, _ in OVERLAP_CASES.values()}
    ids = surface_case_ids()
    assert {off for n, nb, off, ov in ids if n >= 4} == {0, 1, 2, 3}
    assert any(n > 4 * SURF_GRID and off == 0 for n, nb, off, ov in ids) and any(n > SURF_GRID and off for n, nb, off, ov in ids)
    assert any(n % 4 and n > 4 and off == 0 for n, nb, off, ov in ids) and any(n < 4 and off == 0 for n, nb, off, ov in ids)
    for n, nb, off, ov in ids:
        if n >= 1027 and nb > SURF_LDS_BINS:
            a_in, a_out, b = surface_inputs(n, nb, n + nb + off, ov)
            d = (a_in + a_out)[b == 1]
            assert (d == SURF_LDS_BINS - 1).any() and (d == SURF_LDS_BINS).any() and (nb < 5000 or ((d > SURF_LDS_BINS) & (d < nb)).any())
    assert any(nb < SURF_LDS_BINS for n, nb, off, ov in ids)
    same = different = gap = last_slot = 0
    for name, (nbins, sparse) in ORDER_CASES.items():
        for q in QUANTILES:
            b0, b1, m = percentile_reference(sparse, q)
            if m:
                same += b0 >> 10 == b1 >> 10
                different += (b1 >> 10) - (b0 >> 10) == 1
                gap += (b1 >> 10) - (b0 >> 10) > 1
                last_slot += b0 % 1024 == 1023 or b1 % 1024 == 1023
                edge = b0 % 1024 == 1023 and b1 % 1024 == 0 and b1 == b0 + 1
                if name.startswith("edge-adjacent") and q == cases.Q95:
                    assert edge, name
    assert same and different and gap and last_slot
    assert {nb for nb, _ in ORDER_CASES.values()} >= {1, 2, 1023, 1024, 1025, 16383, 16384, 16385, 111000, 4194304}
    assert {total(s) for _, s in ORDER_CASES.values()} >= {0, 1, 2, 20, 21, 1 << 24, (1 << 24) + 3, 3 * 10 ** 9}
