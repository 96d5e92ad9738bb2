"""The soft cost-volume statistics on the device (run on the MI355X box with `-m gpu`): cvx_soft_stats_f32 against the numpy
restatement of csrc/softstats_core.h (tests/softstats_restatement.py) bit for bit -- all twelve channels and the counter -- over
hw in {0, 1, 2, 3, 5} x the grids (1, 1, 1), (3, 5, 7), (2, 3, 67), (4, 9, 33) x float32 / float16 volumes x with / without a field: the
smallest shapes with a partial 64-cell slab (every one), more cells than one workgroup (201 and 1188 cells: 4 and 19 slabs), more chunks
than wavefronts per workgroup (hw 5: 11 chunks on 6 wavefronts, a full round and one of five; hw <= 3 take one round), K = 1 (hw 0), and
planes shorter than, equal to and not a multiple of the eight entries of look-ahead (1, 9, 25, 49, 121).  Then the known answers,
non-finite columns, repeatability, the Python helpers and convex_confidence."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softstats_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def U():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import convex_adam_utils
    return convex_adam_utils


def device_stats(U, ssd, hw, beta, field=None, coupling=0.0):
    out, info = U.soft_stats(torch.from_numpy(ssd).to(DEV), hw, beta, None if field is None else torch.from_numpy(field).to(DEV), coupling,
                             return_info=True)
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == (12,) + tuple(ssd.shape[1:])
    return out.cpu().numpy(), info["non_finite"]


CASES = R.bit_cases()


def test_the_cases_cover_every_axis():
    assert len(CASES) == 5 * 4 * 2 * 2 and len({c[0] for c in CASES}) == 80


@pytest.mark.parametrize("hw", R.HWS)
def test_device_equals_the_restatement_bit_for_bit(U, hw):
    for name, ssd, chw, beta, field, coupling in CASES:
        if chw != hw:
            continue
        want, bad = R.soft_stats(ssd, hw, beta, field, coupling)
        got, n = device_stats(U, ssd, hw, beta, field, coupling)
        assert n == bad == 0, name
        diff = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
        assert diff.size == 0, "%s: %d of %d values differ, the first at channel %d" % (name, diff.size, got.size, diff[0] // (got.size // 12))


def test_known_answers(U):
    for hw in (0, 1, 3, 5):
        out, bad = device_stats(U, R.flat_column(hw), hw, 2.0)
        o = out.reshape(12)
        assert bad == 0 and (o[0:3] == 0).all() and o[3] == o[6] == o[8] == F(np.float64(hw * (hw + 1)) / 3.0) and o[4] == o[5] == o[7] == 0
        assert o[9] == (2 * hw + 1) ** 3 and o[10] == 0 and o[11] == F(3.25)
        assert same_bits(out, R.soft_stats(R.flat_column(hw), hw, 2.0)[0])
    for hw, beta, k in ((1, 2.0, 0), (2, 2.0, 7), (2, 0.125, 124), (3, 40.0, 171), (5, 1.0, 1330)):
        out, bad = device_stats(U, R.spike_column(hw, beta, k), hw, beta)
        o = out.reshape(12)
        assert bad == 0 and (o[0:3] == R.deltas(hw)[k]).all() and (o[3:9] == 0).all() and o[9] == 1 and o[10] == 0 and o[11] == 0


def test_half_volume_with_infinite_entries(U):
    ssd = R.half_with_inf()
    for field, coupling in ((None, 0.0), (R.random_field(2, (3, 5, 7), 4), 1.0)):
        want, bad = R.soft_stats(ssd, 2, 0.001, field, coupling)
        got, n = device_stats(U, ssd, 2, 0.001, field, coupling)
        assert n == bad == 0 and np.isfinite(got).all() and same_bits(got, want)


def test_non_finite_columns_are_nan_counted_and_alone(U):
    for half in (False, True):
        ssd, cells = R.poisoned(half=half)
        clean = R.random_volume(2, (3, 5, 7), 321, half)
        for field, coupling in ((None, 0.0), (R.random_field(2, (3, 5, 7), 5), 1.0)):
            got, n = device_stats(U, ssd, 2, 3.0, field, coupling)
            want, bad = R.soft_stats(ssd, 2, 3.0, field, coupling)
            assert n == bad == 3 and same_bits(got, want)
            g = got.reshape(12, -1)
            nan_cells = np.flatnonzero(np.isnan(g).any(0))
            assert nan_cells.tolist() == sorted(cells) and np.isnan(g[:, nan_cells]).all()
            ref = device_stats(U, clean, 2, 3.0, field, coupling)[0].reshape(12, -1)
            keep = np.setdiff1d(np.arange(g.shape[1]), cells)
            assert same_bits(g[:, keep], ref[:, keep]), "a non-finite column changed its neighbours"


def test_two_runs_give_identical_bytes(U):
    name, ssd, hw, beta, field, coupling = next(c for c in CASES if c[0] == "hw5-4x9x33-f32-field")
    s, u = torch.from_numpy(ssd).to(DEV), torch.from_numpy(field).to(DEV)
    a = U.soft_stats(s, hw, beta, u, coupling)
    b = U.soft_stats(s, hw, beta, u, coupling)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_python_helpers(U):
    name, ssd, hw, beta, field, coupling = next(c for c in CASES if c[0] == "hw2-3x5x7-f32-data")
    want, _ = R.soft_stats(ssd, hw, beta)
    st = U.soft_stats(torch.from_numpy(ssd).to(DEV), hw, beta)
    disp = U.soft_displacement(st)
    assert tuple(disp.shape) == (1, 3, 3, 5, 7) and same_bits(disp[0].cpu().numpy(), want[0:3])
    cov = U.soft_covariance(st)
    assert tuple(cov.shape) == (3, 5, 7, 3, 3) and torch.equal(cov, cov.transpose(-1, -2))
    c = cov.cpu().numpy()
    for (a, b), ch in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(3, 9)):
        assert same_bits(c[..., a, b], want[ch]) and same_bits(c[..., b, a], want[ch])
    ent = U.soft_entropy(st, beta)
    assert ent.dtype == torch.float64 and tuple(ent.shape) == (3, 5, 7)
    # torch's and numpy's float64 log may differ in the last place: 2 ulp of ln Z <= ln 125
    assert float(np.abs(ent.cpu().numpy() - R.entropy(want, beta)).max()) <= 2 * np.spacing(np.log(125.0))
    assert float(ent.min()) >= 0.0 and float(ent.max()) <= np.log(125.0) + 1e-6
    sig = U.soft_sigma(st, 4)
    assert tuple(sig.shape) == (3, 5, 7)
    assert np.allclose(sig.cpu().numpy(), np.sqrt(want[3] + want[6] + want[8]) * 4, rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        U.soft_stats(torch.from_numpy(ssd).to(DEV), 3, beta)
    with pytest.raises(ValueError, match="needs a field"):
        U.soft_stats(torch.from_numpy(ssd).to(DEV), hw, beta, coupling=1.0)
    from convexadam_amd._lib import CvxError
    with pytest.raises(CvxError, match="beta"):
        U.soft_stats(torch.from_numpy(ssd).to(DEV), hw, 0.0)


def test_convex_confidence_on_a_phantom_pair(U):
    from convexadam_amd.phantom import phantom
    fix = phantom((48, 48, 48), 1, 10)
    mov = torch.roll(fix, (4, 0, 0), (0, 1, 2))
    a, b = fix.to(DEV), mov.to(DEV)
    grid_sp, hw, beta = 4, 2, 50.0
    res = U.convex_confidence(a, b, beta, grid_sp=grid_sp, disp_hw=hw)
    # by hand: the same operators, one after the other
    from convexadam_amd.convex_adam_MIND import extract_features
    ff, fm = extract_features(a, b, 1, 2, False, None, None, device=torch.device(DEV), dtype=torch.float32)
    ff, fm = U.avg_pool(ff, grid_sp), U.avg_pool(fm, grid_sp)
    ssd, am = U.correlate(ff, fm, hw, grid_sp, (48, 48, 48), 12)
    field = U.coupled_convex(ssd, am, U.disp_mesh_t(hw, DEV), grid_sp, (48, 48, 48))
    assert tuple(res.field.shape) == (1, 3, 12, 12, 12) and torch.equal(res.field, field)
    stats, info = U.soft_stats(ssd, hw, beta, field=field, coupling=1.0, return_info=True)
    assert info["non_finite"] == 0 and torch.equal(res.stats.view(torch.int32), stats.view(torch.int32))
    assert tuple(res.sigma.shape) == (48, 48, 48) == tuple(res.entropy.shape) and res.sigma.is_cuda
    assert bool(torch.isfinite(res.sigma).all()) and float(res.entropy.min()) >= -1e-5 and float(res.entropy.max()) <= np.log(125.0) + 1e-4
    assert same_bits(stats.cpu().numpy(), R.soft_stats(ssd.cpu().numpy(), hw, beta, field[0].cpu().numpy(), 1.0)[0])
    # in the interior the soft mean of the coupled energy stays near the field it was taken around
    inner = (slice(None), slice(3, 9), slice(3, 9), slice(3, 9))
    assert float((U.soft_displacement(stats)[0] - field[0])[inner].abs().max()) < 1.0
    coarse = U.convex_confidence(a, b, beta, grid_sp=grid_sp, disp_hw=hw, full_res=False)
    assert coarse.sigma is None and coarse.entropy is None and torch.equal(coarse.stats.view(torch.int32), stats.view(torch.int32))
