"""Cross-check of the CPU oracle against the upstream reference itself, on inputs that are NOT in the other golden files.
The reference's outputs on these inputs are stored in tests/golden/live.npz (captured by tests/golden/make_golden_live.py, which
also regenerates the inputs from seeds here): small outputs as arrays, large ones as a digest of their bits (make_golden_live.digest:
equal digests <=> np.array_equal(..., equal_nan=True) with the same shape and dtype).  Never part of the `-m gpu` selection."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_live as L  # noqa: E402  (the inputs, regenerated from seeds, and the digest)


@pytest.fixture(scope="module")
def ref(golden):
    return golden("live")


def same(ref, key, a):
    return L.digest(a) == str(ref[key])


def test_operators_on_fresh_inputs(ref, orc):
    # correlate -> coupled_convex -> inverse_consistency on random features (hw 3, ragged extents)
    f, m, a, b = L.ops_inputs()
    os_, oa = orc.correlate(f[0].numpy(), m[0].numpy(), L.OPS_HW)
    assert same(ref, "ops_ssd_digest", os_) and np.array_equal(ref["ops_argmin"], oa)
    assert np.array_equal(ref["ops_soft"], orc.coupled_convex(os_, oa, orc.disp_mesh(L.OPS_HW), L.OPS_HW))
    o1, o2 = orc.inverse_consistency(a[0].numpy(), b[0].numpy(), 7)
    assert np.array_equal(ref["ops_ic1"], o1) and np.array_equal(ref["ops_ic2"], o2)


@contextlib.contextmanager
def reference_exp(orc, mkl, threads=8):
    """The oracle in reference-bits mode: the capture host's MKL exp / sqrt (the golden host's tables) and torch's `threads`-thread mean."""
    t = mkl.golden_tables()
    orc.set_exp_table(t["exp"], t["exp_first"], t["exp_count"])
    orc.set_sqrt_table(t["sqrt"])
    orc.set_mean_threads(threads)
    try:
        yield
    finally:
        orc.set_exp_table(None)
        orc.set_sqrt_table(None)
        orc.set_mean_threads(0)


def test_mindssc_on_fresh_input(ref, orc, mkl):
    img = L.mind_input()[0, 0].numpy()
    with reference_exp(orc, mkl):
        out = orc.mindssc(img, 1, 2)                 # with MKL's exp as a table: the reference's output bit for bit ...
    assert same(ref, "mind_digest", out)
    mine = orc.mindssc(img, 1, 2)                    # ... and the oracle's own expf within one ulp of it
    assert np.abs(out - mine).max() <= 6e-8          # MKL vsExp vs the expf restatement: <= 1 ulp


def test_whole_pipeline_convex_stage_on_fresh_pair(ref, orc, mkl):
    fix, mov = L.convex_pair()
    with reference_exp(orc, mkl):
        out = orc.convex_adam_pipeline(fix.numpy(), mov.numpy(), **L.CONVEX_KW)     # the reference's field bit for bit ...
    assert same(ref, "convex_field_digest", out)
    mine = orc.convex_adam_pipeline(fix.numpy(), mov.numpy(), **L.CONVEX_KW)
    epe = float(np.sqrt(((out - mine) ** 2).sum(-1)).mean())
    assert epe <= 1e-5, epe                          # exp differs by <= 1 ulp; everything downstream is restated exactly


@pytest.mark.parametrize("threads", L.BITS_THREADS)
def test_whole_pipeline_bit_identical_in_reference_bits_mode_on_fresh_pairs(ref, orc, mkl, threads):
    """The reference ran on pairs that are in no other golden file (a textured pair with a zero background -- flat regions whose
    variance is clamped, so the thread-count dependent mean matters -- 25 Adam iterations, final smoothing) with `threads` torch threads;
    the oracle, given the capture host's MKL tables (the golden host's, mkl.golden_tables) and the run's thread count, returns the same
    bits."""
    with reference_exp(orc, mkl, threads):
        for i, (shape, seed, kw) in enumerate(L.BITS_CASES):
            fix, mov = L.bits_pair(shape, seed)
            mine = orc.convex_adam_pipeline(fix.numpy(), mov.numpy(), **kw)
            assert same(ref, "bits%d_t%d_digest" % (i, threads), mine), shape


def test_nan_and_inf_in_the_cost_volume(ref, orc):
    """Nulls: torch.argmin returns the FIRST NaN of a column (a NaN counts as smaller than everything) and otherwise the first minimum;
    the oracle follows that in the plain argmin and in the six coupled passes (round 3; before, NaN entries were skipped)."""
    mesh = orc.disp_mesh(L.NAN_HW)
    for case, (f, m) in enumerate(L.nan_inputs()):
        rs, ra = orc.correlate(f, m, L.NAN_HW)
        assert same(ref, "nan%d_ssd_digest" % case, rs) and np.array_equal(ref["nan%d_argmin" % case], ra), case
        assert np.array_equal(ref["nan%d_soft" % case], orc.coupled_convex(rs, ra, mesh, L.NAN_HW), equal_nan=True), case
