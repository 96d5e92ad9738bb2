"""The SSIM kernel (csrc/ssim.hip) on the device.

Bounds.  Against the reference's float64 result, the allowance is the reference's OWN float32 distance from it (E_map, E_mean, E_slice:
captured in tests/golden/ssim.npz for the golden cases, taken from a dense float32 torch-CPU evaluation for the edge cases) plus
2^-20 for the map (eight float32 ulps at 1) and 2^-22 for the means (two): no multiplicative margin.  The separable float32
evaluation sits 2 to 9 times inside the reference's distance (golden/make_golden_ssim.py asserts that before it writes the
fixture); the additive terms cover the cases where that distance is itself only a few ulps.
Exact properties are asserted bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_golden  # noqa: E402
from test_ssim_reference import ssim_dense, ssim_f64  # noqa: E402

pytestmark = pytest.mark.gpu

MAP_ADD, MEAN_ADD = 2.0 ** -20, 2.0 ** -22


@pytest.fixture(scope="module")
def S():
    from convexadam_amd import ssim
    return ssim


def dev(t):
    return t.to("cuda")


def run_all(S, x, y, ws):
    """map, mean, slice means of device tensors -> numpy float64 / float / numpy float64"""
    m = S.ssim3D_map(x, y, ws)
    r = S.ssim3D(x, y, ws)
    s = S.ssim3D(x, y, ws, size_average=False)
    assert m.shape == x.shape and m.dtype == torch.float32 and m.is_cuda
    assert r.shape == () and r.dtype == torch.float32 and r.is_cuda
    assert s.shape == (x.shape[0], x.shape[-1]) and s.dtype == torch.float32 and s.is_cuda
    return m.cpu().numpy().astype(np.float64), float(r.cpu().double()), s.cpu().numpy().astype(np.float64)


def grade(got, want, allow, what=""):
    (m, r, s), (m64, r64, s64), (e_map, e_mean, e_slice) = got, want, allow
    d_map, d_mean, d_slice = np.abs(m - m64).max(), abs(r - r64), np.abs(s - s64).max()
    print("%s map %.3g (E %.3g)  mean %.3g (E %.3g)  slices %.3g (E %.3g)" % (what, d_map, e_map, d_mean, e_mean, d_slice, e_slice))
    assert np.isfinite(m).all()
    assert d_map <= e_map + MAP_ADD, what
    assert d_mean <= e_mean + MEAN_ADD, what
    assert d_slice <= e_slice + MEAN_ADD, what


def check_against_f64(S, x, y, ws, what=""):
    """x, y CPU float32 (N, C, H, W, D): the device against the float64 yardstick, allowance = a dense float32 CPU evaluation's distance."""
    want = ssim_f64(x, y, ws)
    m32, r32, s32 = ssim_dense(x, y, ws)
    allow = (np.abs(m32.double().numpy() - want[0]).max(), abs(float(r32.double()) - want[1]), np.abs(s32.double().numpy() - want[2]).max())
    grade(run_all(S, dev(x), dev(y), ws), want, allow, what)


def pair(shape, seed=0, nc=(1, 1)):
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand(*nc, *shape, generator=g)
    return x, (x + 0.2 * torch.randn(*nc, *shape, generator=g)).clamp_(0, 1)


# ---- 1. golden cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ws", [(n, w) for n, wss in ssim_golden.CASES for w in wss])
def test_golden_cases(S, golden, name, ws):
    g = golden("ssim")
    k = lambda f: ssim_golden.key(name, ws, f)                                  # noqa: E731
    x, y = ssim_golden.inputs(name)
    grade(run_all(S, dev(x), dev(y), ws), (g[k("m64")], float(g[k("r64")]), g[k("s64")]),
          (float(g[k("E_map")]), float(g[k("E_mean")]), float(g[k("E_slice")])), "%s ws %d:" % (name, ws))


# ---- 2. exact properties ------------------------------------------------------------------------------------------------------
def test_identical_and_zero_inputs_give_exactly_one(S):
    x = dev(pair((19, 18, 35), 1, (2, 2))[0])
    for a in (x, torch.zeros_like(x)):
        for ws in (11, 3):
            m = S.ssim3D_map(a, a.clone(), ws)
            assert torch.equal(m, torch.ones_like(m))
            assert float(S.ssim3D(a, a.clone(), ws)) == 1.0
            assert torch.equal(S.ssim3D(a, a.clone(), ws, size_average=False), torch.ones(2, 35, device="cuda"))


def test_symmetric_in_its_arguments(S):
    x, y = [dev(t) for t in pair((21, 19, 37), 2, (1, 2))]
    for ws in (11, 5):
        assert torch.equal(S.ssim3D_map(x, y, ws), S.ssim3D_map(y, x, ws))
        assert torch.equal(S.ssim3D(x, y, ws), S.ssim3D(y, x, ws))
        assert torch.equal(S.ssim3D(x, y, ws, False), S.ssim3D(y, x, ws, False))


def test_a_volume_has_the_same_bits_alone_and_anywhere_in_a_batch(S):
    """(the H chunking follows the number of volumes: 35 planes are walked as two chunks alone and as ONE chunk among 600 volumes)"""
    x, y = [dev(t) for t in pair((35, 18, 33), 3, (7, 1))]
    whole = S.ssim3D_map(x, y)
    as_channels = S.ssim3D_map(x.view(1, 7, 35, 18, 33), y.view(1, 7, 35, 18, 33))
    assert torch.equal(whole.view(-1), as_channels.view(-1))
    for i in (0, 3, 6):
        assert torch.equal(S.ssim3D_map(x[i:i + 1], y[i:i + 1]), whole[i:i + 1]), i
    many_x, many_y = x[:1].repeat(600, 1, 1, 1, 1), y[:1].repeat(600, 1, 1, 1, 1)
    many = S.ssim3D_map(many_x, many_y)
    assert torch.equal(many[0], whole[0]) and torch.equal(many[599], whole[0])


def test_two_runs_give_the_same_bits(S):
    x, y = [dev(t) for t in pair((40, 37, 70), 4, (2, 3))]
    first = (S.ssim3D_map(x, y), S.ssim3D(x, y), S.ssim3D(x, y, size_average=False))
    for _ in range(3):
        again = (S.ssim3D_map(x, y), S.ssim3D(x, y), S.ssim3D(x, y, size_average=False))
        assert all(torch.equal(a, b) for a, b in zip(first, again))


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def test_the_means_are_the_float64_means_of_the_map(S):
    for shape, nc, ws in (((40, 37, 70), (2, 3), 11), ((5, 4, 3), (1, 1), 11), ((33, 16, 32), (3, 1), 7)):
        x, y = [dev(t) for t in pair(shape, 5, nc)]
        m = S.ssim3D_map(x, y, ws).cpu().numpy().astype(np.float64)
        r, s = float(S.ssim3D(x, y, ws)), S.ssim3D(x, y, ws, size_average=False).cpu().numpy()
        assert ulps(r, np.float32(m.mean())) <= 1
        want = m.mean(axis=(1, 2, 3)).astype(np.float32)
        assert s.shape == want.shape and max(ulps(a, b) for a, b in zip(s.ravel(), want.ravel())) <= 1


# ---- 3. edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 7, 9), (9, 1, 7), (7, 9, 1), (5, 4, 3), (6, 7, 63), (6, 7, 64), (6, 7, 65)])
def test_extent_edges(S, shape):
    x, y = pair(shape, 6)
    check_against_f64(S, x, y, 11, "%s:" % (shape,))


@pytest.mark.parametrize("ws", [1, 3, 7, 11])
def test_window_sizes(S, ws):
    x, y = pair((12, 13, 14), 7, (1, 2))
    check_against_f64(S, x, y, ws, "ws %d:" % ws)


def _tile_extents():
    from convexadam_amd.ssim import TILE
    out = []
    for axis, t in enumerate(TILE):                      # H chunk, W tile, D tile: one below, at, one above, two tiles plus one
        for e in (t - 1, t, t + 1, 2 * t + 1):
            shape = [7, 6, 9]
            shape[axis] = e
            out.append(tuple(shape))
    return out


@pytest.mark.parametrize("shape", _tile_extents())
def test_tile_edges(S, shape):
    x, y = pair(shape, 8)
    check_against_f64(S, x, y, 11, "%s:" % (shape,))


def test_every_tiled_axis_cut_at_once(S):
    from convexadam_amd.ssim import TILE
    x, y = pair(tuple(2 * t + 1 for t in TILE), 9)
    check_against_f64(S, x, y, 11, "all axes:")


@pytest.mark.parametrize("nc", [(1, 1), (2, 1), (1, 2), (7, 1)])
def test_batches(S, nc):
    x, y = pair((9, 17, 33), 10, nc)
    check_against_f64(S, x, y, 11, "N, C = %s:" % (nc,))


def test_non_contiguous_and_other_dtypes(S):
    x, y = pair((9, 17, 33), 11, (2, 2))
    ref = [t.clone() for t in (S.ssim3D_map(dev(x), dev(y)), S.ssim3D(dev(x), dev(y)))]
    xp = dev(x).permute(0, 1, 4, 3, 2).contiguous().permute(0, 1, 4, 3, 2)        # same values, strides of another layout
    assert not xp.is_contiguous()
    assert torch.equal(S.ssim3D_map(xp, dev(y)), ref[0]) and torch.equal(S.ssim3D(xp, dev(y)), ref[1])
    assert torch.equal(S.ssim3D_map(dev(x).double(), dev(y).double()), ref[0])    # float64 in: converted to float32
    xh = dev(x).half()
    assert torch.equal(S.ssim3D_map(xh, dev(y)), S.ssim3D_map(xh.float(), dev(y)))


def test_refused_windows_raise_on_the_device_too(S):
    from convexadam_amd._lib import CvxError
    x = torch.zeros(1, 1, 8, 8, 8, device="cuda")
    with pytest.raises(CvxError, match="odd"):
        S.ssim3D(x, x, window_size=8)
    with pytest.raises(CvxError, match="at most 11"):
        S.ssim3D_map(x, x, window_size=13)


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------
def test_registration_raises_the_ssim(S):
    from convexadam_amd.convex_adam_MIND import register_pair_device
    from convexadam_amd.phantom import deformed_pair
    fixed, moving = [dev(t) for t in deformed_pair((48, 56, 64))]
    disp = register_pair_device(fixed, moving, grid_sp=4, disp_hw=3, selected_niter=10)
    after = S.registration_ssim(fixed, moving, disp)
    before = S.ssim3D(fixed[None, None], moving[None, None])
    assert after.is_cuda and after.shape == ()
    print("ssim before %.4f after %.4f" % (float(before), float(after)))
    assert float(after) > float(before)
    warped = S.warp_device(moving, disp)
    assert torch.equal(after, S.ssim3D(fixed[None, None], warped[None, None]))
    # the field in the layout convex_adam_pt returns
    assert torch.equal(S.registration_ssim(fixed, moving, disp.permute(1, 2, 3, 0).contiguous()), after)
