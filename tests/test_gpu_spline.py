"""Cubic B-spline interpolation on the device (run on the MI355X box with `-m gpu`): the three entry points of include/convexadam_spline.h
and the Python functions built on them against the numpy restatement of csrc/spline_core.h, EXACTLY, and against scipy.ndimage (order=3,
mode='constant') inside the bound that tests/spline_restatement.py states (64 times the measured restatement-to-scipy figure).

Every shape of spline_restatement.SHAPES: lengths 1, 2 and 3, extents that fill no tile, a contiguous line of 131 samples (four staged
chunks of 32 and a rest of 3), strided lines of 67.  The coordinate list of a case (about 280 points: inside, around the edges, on them,
a hair outside, NaN, +-Inf, 1e300) is visited by fields that aim each voxel at a point of the list, as many launches as the volume needs
to see them all."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spline_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CASES = {}


def case(shape):
    """volume, coefficients (restatement), coordinate list -- computed once per shape and never changed"""
    if shape not in _CASES:
        k = R.SHAPES.index(shape)
        vol = R.volume(shape, k)
        c = R.coordinates(shape, k)
        _CASES[shape] = dict(vol=vol, vol32=vol.astype(np.float32), coef=R.prefilter(vol), coef32=R.prefilter(vol.astype(np.float32)), c=c)
        for v in _CASES[shape].values():
            v.setflags(write=False)
    return _CASES[shape]


@pytest.fixture(scope="module")
def S():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import spline
    return spline


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a copy: the shared cases are read-only)


def host(t):
    return t.cpu().numpy()


def test_coefficients_equal_the_restatement_and_scipy(S):
    for shape in R.SHAPES:
        _coefficients(S, shape)


def _coefficients(S, shape):
    k = case(shape)
    for vol, want in ((k["vol"], k["coef"]), (k["vol32"], k["coef32"])):
        got = S.spline_coefficients(dev(vol))
        assert got.dtype == torch.float64 and got.is_cuda
        assert np.array_equal(host(got), want), (shape, vol.dtype, float(np.abs(host(got) - want).max()))
        ref = ndimage.spline_filter(vol.astype(np.float64), order=3, mode="constant", output=np.float64)
        assert np.abs(host(got) - ref).max() <= R.SCIPY_BOUND_COEF * np.abs(vol).max()
    # integer volumes are read as float64
    ints = np.rint(k["vol"]).astype(np.int16)
    assert np.array_equal(host(S.spline_coefficients(dev(ints))), R.prefilter(ints.astype(np.float64)))


def test_in_place_prefilter_equals_out_of_place(S):
    from convexadam_amd import _lib
    _lib.spline_lib()
    for shape in R.SHAPES:
        k = case(shape)
        buf = dev(k["vol"])
        _lib.call(torch.device(DEV), "cvx_spline_prefilter_f64", _lib.ptr(buf), 1, *shape, _lib.ptr(buf))
        assert np.array_equal(host(buf), k["coef"]) and np.array_equal(host(buf), host(S.spline_coefficients(dev(k["vol"])))), shape


def raw_warp(coef, disp, planar):
    """cvx_map_coordinates_cubic_f64 with the strides of the layout said outright"""
    from convexadam_amd import _lib
    shape = tuple(coef.shape)
    V = int(np.prod(shape))
    out = torch.empty(shape, dtype=torch.float64, device=DEV)
    _lib.spline_lib()
    _lib.call(torch.device(DEV), "cvx_map_coordinates_cubic_f64", _lib.ptr(coef), _lib.ptr(disp), int(disp.dtype == torch.float64),
              V if planar else 1, 1 if planar else 3, *shape, _lib.ptr(out))
    return out


def test_values_equal_the_restatement_and_scipy(S):
    for shape in R.SHAPES:
        _values(S, shape)


def _values(S, shape):
    k = case(shape)
    V, n = int(np.prod(shape)), len(k["c"])
    coef_d = dev(k["coef"])
    seen_inside = seen_outside = 0
    all_got, all_c = [], []
    combos = [("interleaved", np.float64), ("planar", np.float64), ("interleaved", np.float32), ("planar", np.float32)]
    starts = list(range(0, n, V))                            # a volume smaller than the list sees it in several launches, one combination each
    for b, start in enumerate(starts):
        for layout, dt in (combos if len(starts) <= 4 else [combos[b % 4]]):
            field = R.field_through(shape, k["c"], start, dt)
            c = R.warp_coordinates(shape, field)
            want = R.map_cubic(k["coef"], c).reshape(shape)
            disp = dev(field if layout == "interleaved" else np.moveaxis(field, -1, 0))
            got = host(raw_warp(coef_d, disp, layout == "planar"))
            if shape != (3, 3, 3) or layout == "interleaved":            # (3, 3, 3, 3) is read as (H, W, D, 3) by the Python layer: _lib.field_operand
                assert np.array_equal(host(S.warp_cubic(coef_d, disp, prefiltered=True)), got)
            assert np.array_equal(got, want), (shape, layout, dt, start)
            all_got.append(got.reshape(-1))
            all_c.append(c)
            inside = R.is_inside(shape, c).reshape(shape)
            assert (got[~inside] == 0.0).all() and (got[inside] != 0.0).all()
            seen_inside += int(inside.sum())
            seen_outside += int((~inside).sum())
    ref = ndimage.map_coordinates(k["vol"], np.concatenate(all_c).T, order=3, mode="constant", cval=0.0)      # scipy once, on every point sampled
    assert np.abs(np.concatenate(all_got) - ref).max() <= R.SCIPY_BOUND_VALUE * np.abs(k["vol"]).max()
    assert seen_inside >= n // 2 and seen_outside >= 19, "the launches visit the whole list: inside points, outside and non-finite ones"
    # the unprefiltered call is the two steps in one
    field = R.field_through(shape, k["c"], 0, np.float32)
    assert torch.equal(S.warp_cubic(dev(k["vol"]), dev(field)), S.warp_cubic(coef_d, dev(field), prefiltered=True))
    assert np.array_equal(host(S.warp_cubic(dev(k["vol32"]), dev(field))),
                          R.map_cubic(k["coef32"], R.warp_coordinates(shape, field)).reshape(shape))


def test_non_finite_and_outside_coordinates_give_zero(S):
    shape = (5, 6, 7)
    k = case(shape)
    for bad in (np.nan, np.inf, -np.inf, 1e300, -1e300, -1e-9 - 6.0, 7.0):
        for axis in range(3):
            field = np.zeros(shape + (3,))
            field[..., axis] = bad
            assert (host(S.warp_cubic(dev(k["vol"]), dev(field))) == 0.0).all(), (bad, axis)
    for dt in (np.float32, np.float64):                      # a float32 field cannot hold 1e300: it is +Inf there, still outside
        with np.errstate(over="ignore"):
            field = np.full(shape + (3,), 1e300).astype(dt)
        assert (host(S.warp_cubic(dev(k["vol"]), dev(field))) == 0.0).all()


def test_constant_volume_and_integer_coordinates(S):
    for shape in ((5, 6, 7), (1, 4, 5), (3, 5, 131)):
        k = case(shape)
        const = np.full(shape, 7.25)
        field = R.field_through(shape, k["c"][:R.N_RANDOM * 3 // 4], 0)
        got = host(S.warp_cubic(dev(const), dev(field)))
        assert np.abs(got - 7.25).max() <= R.SCIPY_BOUND_VALUE * 7.25
        zero = np.zeros(shape + (3,), np.float32)
        got = host(S.warp_cubic(dev(k["vol"]), dev(zero)))
        assert np.abs(got - k["vol"]).max() <= R.SCIPY_BOUND_VALUE * np.abs(k["vol"]).max()
        whole = np.zeros(shape + (3,))                       # one voxel further along the last axis: the neighbour's sample, 0 behind the end
        whole[..., 2] = 1.0
        got = host(S.warp_cubic(dev(k["vol"]), dev(whole)))
        assert np.abs(got[..., :-1] - k["vol"][..., 1:]).max() <= R.SCIPY_BOUND_VALUE * np.abs(k["vol"]).max() and (got[..., -1] == 0.0).all()


def test_apply_convex_order_3_equals_scipy_and_order_1_is_untouched():
    from convexadam_amd.apply_convex import apply_convex
    import convexAdam.apply_convex as shim
    shape = (9, 8, 12)
    k = case(shape)
    rng = np.random.default_rng(5)
    disp = rng.uniform(-2.5, 2.5, shape + (3,))
    c = R.warp_coordinates(shape, disp)
    want = ndimage.map_coordinates(k["vol"], c.T, order=3, mode="constant", cval=0.0).reshape(shape)
    vol = k["vol"].copy()
    got = apply_convex(disp, vol, order=3)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert np.abs(got - want).max() <= R.SCIPY_BOUND_VALUE * np.abs(k["vol"]).max()
    assert np.array_equal(got, R.map_cubic(k["coef"], c).reshape(shape))
    inside = R.is_inside(shape, c).reshape(shape)
    assert inside.any() and (~inside).any() and (got[~inside] == 0.0).all() and (got[inside] != 0.0).all()
    assert np.array_equal(shim.apply_convex(disp, vol, order=3), got)
    # device tensors keep their dtype; integer tensors are rounded like scipy's integer outputs
    got32 = apply_convex(torch.from_numpy(disp).to(DEV), dev(k["vol32"]), order=3)
    assert got32.dtype == np.float32 and np.array_equal(got32, R.map_cubic(k["coef32"], c).reshape(shape).astype(np.float32))
    ints = np.rint(k["vol"]).astype(np.int16)
    goti = apply_convex(disp, torch.from_numpy(ints), order=3)
    wanti = ndimage.map_coordinates(ints, c.T, order=3, mode="constant", cval=0.0).reshape(shape)
    # (both round a float64 value to nearest; the two values differ by at most the bound, so only a value that close to a tie may round apart)
    assert goti.dtype == np.int16 and np.abs(goti.astype(np.int64) - wanti).max() <= 1 and (goti == wanti).mean() > 0.99
    # order=1 is the call without the keyword, byte for byte, and scipy's order=1
    a, b = apply_convex(disp, vol), apply_convex(disp, vol, order=1)
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert np.abs(a - ndimage.map_coordinates(k["vol"], c.T, order=1, mode="constant", cval=0.0).reshape(shape)).max() <= 1e-12 * R.MAGNITUDE
    assert np.abs(a - got).max() > 1.0, "the two orders differ on a random volume"
    with pytest.raises(ValueError, match="order must be 1"):
        apply_convex(disp, vol, order=2)


def _grid(shape, origin=(0.0, 0.0, 0.0)):
    from convexadam_amd.geometry import Grid
    return Grid(tuple(int(s) for s in shape[::-1]), (1.0, 1.0, 1.0), tuple(origin), tuple(np.eye(3).reshape(-1)))


def test_resample_device_order_3_equals_the_restatement():
    for shape in ((5, 6, 7), (3, 5, 131), (1, 4, 5)):
        _resample_device(shape)


def _resample_device(shape):
    from convexadam_amd import geometry
    k = case(shape)
    sg = _grid(shape)
    # the identity map returns the samples (within the bound: the taps at integer coordinates are 1/6, 4/6, 1/6 of the coefficients)
    got = geometry.resample_device(dev(k["vol"]), sg, sg, default=-1.0, order=3)
    M, t = geometry.index_map(sg, sg)
    want = R.itk_cubic(k["coef"], R.index_grid(shape, M, t), -1.0).reshape(shape)
    assert got.dtype == torch.float64 and np.array_equal(host(got), want)
    assert np.abs(host(got) - k["vol"]).max() <= R.SCIPY_BOUND_VALUE * np.abs(k["vol"]).max()
    # half a voxel along x onto a grid one voxel longer on every axis: interpolated values, the clamped half voxel behind the last sample,
    # and the default beyond it
    out_shape = tuple(s + 1 for s in shape)
    og = _grid(out_shape, origin=(0.5, 0.0, 0.0))
    M, t = geometry.index_map(sg, og)
    c = R.index_grid(out_shape, M, t)
    for vol, coef, dt in ((k["vol"], k["coef"], np.float64), (k["vol32"], k["coef32"], np.float32)):
        want = R.itk_cubic(coef, c, -7.5).reshape(out_shape).astype(dt)
        got = geometry.resample_device(dev(vol), sg, og, default=-7.5, order=3)
        assert got.dtype == (torch.float64 if dt == np.float64 else torch.float32) and np.array_equal(host(got), want), (shape, dt)
        assert (want == -7.5).any() and (want != -7.5).any()
        assert (host(got)[-1] == -7.5).all() and (host(got)[:, -1] == -7.5).all()
    # without the keyword, and with order=1, the linear path answers as before
    a, b = geometry.resample_device(dev(k["vol"]), sg, og, default=-7.5), geometry.resample_device(dev(k["vol"]), sg, og, default=-7.5, order=1)
    assert torch.equal(a, b) and not torch.equal(a, geometry.resample_device(dev(k["vol"]), sg, og, default=-7.5, order=3))
    # non-finite index maps and defaults are refused by the library, by name
    from convexadam_amd._lib import CvxError
    with pytest.raises(CvxError, match="cvx_resample_cubic_f64: non-finite"):
        geometry.resample_device(dev(k["vol"]), sg, og, default=float("nan"), order=3)


def test_resample_entry_point_with_a_general_index_map(S):
    """a sheared, scaled map through the raw entry point, float32 and float64 outputs"""
    from convexadam_amd import _lib
    shape, out_shape = (5, 6, 7), (4, 9, 10)
    k = case(shape)
    M = np.array([[0.8, 0.1, 0.0], [-0.05, 0.7, 0.2], [0.0, 0.15, 1.1]])
    t = np.array([-0.4, 0.3, -0.6])
    c = R.index_grid(out_shape, M, t)
    want = R.itk_cubic(k["coef"], c, 2.5).reshape(out_shape)
    assert (want == 2.5).any() and (want != 2.5).sum() > want.size // 4
    m12 = (C.c_double * 12)(*M.reshape(-1).tolist(), *t.tolist())
    coef = dev(k["coef"])
    _lib.spline_lib()
    for f64, dt in ((1, torch.float64), (0, torch.float32)):
        out = torch.empty(out_shape, dtype=dt, device=DEV)
        _lib.call(torch.device(DEV), "cvx_resample_cubic_f64", _lib.ptr(coef), *shape, _lib.ptr(out), f64, *out_shape, m12, 2.5)
        assert np.array_equal(host(out), want.astype(np.float64 if f64 else np.float32))


def test_two_runs_give_the_same_bytes(S):
    k = case((3, 5, 131))
    field = dev(R.field_through((3, 5, 131), k["c"], 0, np.float32))
    a = S.warp_cubic(dev(k["vol"]), field)
    b = S.warp_cubic(dev(k["vol"]), field)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
