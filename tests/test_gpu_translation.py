"""The field-mean kernels (csrc/fieldmean.hip) and the device path of convex_adam_translation on the device.

Sums and counts are compared BIT FOR BIT with the numpy restatement of the contract (tests/translation_restatement.py: the same
additions in the same order; the mask of the segmentation mode from the resampling restatement of tests/geometry_restatement.py).  The
end-to-end cases compare the device path with the host path (device=None) of the same call: same whole-voxel translation, same moved
origin; their inputs and what the CPU oracle says about them are in tests/translation_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_restatement as G  # noqa: E402
import translation_cases as TC  # noqa: E402
import translation_restatement as R  # noqa: E402

from convexadam_amd import geometry  # noqa: E402
from convexadam_amd.geometry import Grid, field_mean_device, grid_of, resample_device  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = np.float32, np.float64
IDENT = tuple(np.eye(3).reshape(-1))
S = R.S
SIZES = (1, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 256 * S, 256 * S + 1)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def line_grid(V):
    return Grid((V, 1, 1), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), IDENT)


def same_bits(a, b):
    """equal bit patterns, any NaN equal to any NaN (payloads are not part of the contract)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def run(values, layout, grid, **kw):
    """values (V, 3) -> the field in `layout` on `grid`, field_mean_device, the result on the host: (sums float64[3], count int)"""
    shape = tuple(grid.size)[::-1]
    field = values.reshape(shape + (3,)) if layout == "last" else np.ascontiguousarray(values.T).reshape((3,) + shape)
    sums, count = field_mean_device(dev(field), grid, **kw)
    assert sums.is_cuda and count.is_cuda and sums.dtype == torch.float64 and count.dtype == torch.int64 and sums.shape == (3,) and count.dim() == 0
    return sums.cpu().numpy(), int(count)


# ---- (a) the order of the additions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SIZES)
def test_voxel_counts_bits(V):
    rng = np.random.default_rng(V)
    v64 = rng.standard_normal((V, 3)) * np.array([3.0, 40.0, 0.01]) + np.array([2.5, -0.3, 0.0])
    mask = rng.random(V) < 0.4
    g = line_grid(V)
    for dt in (F32, F64):
        values = v64.astype(dt)
        want_all, want_masked = R.field_sums(values.astype(F64)), R.field_sums(values.astype(F64), mask)
        assert want_all[1] == V and want_masked[1] == int(mask.sum())
        for layout in ("last", "first"):
            got = run(values, layout, g)
            assert got[1] == V and same_bits(got[0], want_all[0]), (V, dt, layout, got[0] - want_all[0])
            got = run(values, layout, g, mask=dev(mask.reshape(1, 1, V)))
            assert got[1] == want_masked[1] and same_bits(got[0], want_masked[0]), (V, dt, layout, got[0] - want_masked[0])


def test_three_dimensional_grid_and_mask_dtypes():
    """a (H, W, D) grid whose extents are not 3 (no layout is guessed from them) and masks that are not bytes: nonzero counts"""
    rng = np.random.default_rng(5)
    shape = (7, 33, 29)                                                   # 6699 voxels: two blocks
    g = Grid(shape[::-1], (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), IDENT)
    values = rng.standard_normal((7 * 33 * 29, 3)).astype(F32)
    mask = rng.random(shape) < 0.5
    want = R.field_sums(values.astype(F64), mask.reshape(-1))
    for m in (mask, mask.astype(np.uint8) * 200, mask.astype(F32) * -0.5, mask.astype(np.int64) * (1 << 40)):
        for layout in ("last", "first"):
            got = run(values, layout, g, mask=dev(m))
            assert got[1] == want[1] and same_bits(got[0], want[0])
    field = dev(values.reshape(shape + (3,)))
    sums, count = field_mean_device(field, mask=dev(mask))                # the grid's shape taken from the mask
    assert int(count) == want[1] and same_bits(sums.cpu().numpy(), want[0])
    sums, count = field_mean_device(field)                                # ... and from the field, whose layout its shape tells
    assert int(count) == values.shape[0] and same_bits(sums.cpu().numpy(), R.field_sums(values.astype(F64))[0])


def test_uniform_masks():
    V = S + 77
    rng = np.random.default_rng(1)
    values = (rng.standard_normal((V, 3)) - 3.0).astype(F32)              # negative sums: a zero result is not a sum that cancelled
    g = line_grid(V)
    plain = run(values, "first", g)
    for layout in ("last", "first"):
        sums, count = run(values, layout, g, mask=dev(np.zeros((1, 1, V), np.uint8)))
        assert count == 0 and np.array_equal(sums, np.zeros(3)) and not np.signbit(sums).any()
        sums, count = run(values, layout, g, mask=dev(np.ones((1, 1, V), np.uint8)))
        assert count == V and same_bits(sums, plain[0])
    assert same_bits(plain[0], R.field_sums(values.astype(F64))[0])


def test_quantize_float16_round_trip():
    special = np.array([2049.0, 2051.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -15,
                        65504.0, 65519.9, -65519.9, 0.1, -0.3, 3.14159], F32)
    q = R.quantize_f16(special)
    assert q[0] == 2048.0 and q[2] == 1.0 and q[5] == 0.0 and q[6] == 2.0 ** -23 and q[9] == 2.0 ** -15 and q[11] == 65504.0     # ties, subnormals
    g1 = line_grid(1)
    for x, want in zip(special, q):                                       # one value at a time: the sum IS the rounded value
        sums, count = run(np.full((1, 3), x, F32), "first", g1, quantize=torch.float16)
        assert count == 1 and same_bits(sums, np.full(3, want)), (x, sums, want)
        sums, _ = run(np.full((1, 3), x, F32), "last", g1, quantize=torch.float32)
        assert same_bits(sums, np.full(3, np.float64(x)))
    for x, want in ((65520.0, np.inf), (70000.0, np.inf), (-65520.0, -np.inf), (3.0e38, np.inf)):         # beyond the largest half: infinity
        sums, _ = run(np.full((1, 3), x, F32), "first", g1, quantize=1)
        assert np.array_equal(sums, np.full(3, want)), (x, sums)
    rng = np.random.default_rng(2)
    V = 2 * S + 19
    values = np.concatenate([np.tile(special, 3).reshape(-1, 3), (rng.standard_normal((V, 3)) * 4).astype(F32)])
    mask = rng.random(values.shape[0]) < 0.7
    g = line_grid(values.shape[0])
    for layout in ("last", "first"):
        for m in (None, mask):
            want = R.field_sums(R.quantize_f16(values), m)
            kw = {} if m is None else {"mask": dev(m.reshape(1, 1, -1))}
            got = run(values, layout, g, quantize=torch.float16, **kw)
            assert got[1] == want[1] and same_bits(got[0], want[0]), (layout, m is None)
            assert not same_bits(got[0], run(values, layout, g, **kw)[0])                                # the round trip does act
    with pytest.raises(Exception, match="float32"):                        # a float64 field has no float16 round trip
        field_mean_device(dev(values.astype(F64).reshape(1, 1, -1, 3)), g, quantize=torch.float16)


def test_non_finite_values():
    V = S + 300
    rng = np.random.default_rng(3)
    values = rng.standard_normal((V, 3)).astype(F32)
    g = line_grid(V)
    mask = np.ones(V, bool)
    mask[[5, S + 7]] = False
    clean = run(values, "first", g, mask=dev(mask.reshape(1, 1, V)))
    for bad, where, comp in ((np.nan, 5, 1), (np.inf, S + 7, 2), (-np.inf, 5, 0), (np.nan, S + 7, 0)):
        v = values.copy()
        v[where, comp] = bad
        for layout in ("last", "first"):
            got = run(v, layout, g, mask=dev(mask.reshape(1, 1, V)))                   # outside the mask: nothing changes
            assert got[1] == clean[1] and same_bits(got[0], clean[0])
            got = run(v, layout, g)                                                    # counted: that component alone is taken over
            want = R.field_sums(v.astype(F64))
            assert got[1] == V and same_bits(got[0], want[0])
            assert (np.isnan(got[0][comp]) if np.isnan(bad) else got[0][comp] == bad) and np.isfinite(np.delete(got[0], comp)).all()
    v = values.copy()
    v[3, 1], v[S + 1, 1] = np.inf, -np.inf                                             # inf - inf across two blocks
    assert np.isnan(run(v, "last", g)[0][1])
    v = values.copy()
    v[5, 0] = np.nan
    assert np.isnan(run(v, "first", g, quantize=torch.float16)[0][0])                  # NaN survives the float16 round trip


def test_repeatable():
    V = 37 * S + 5
    values = np.random.default_rng(4).standard_normal((V, 3)).astype(F32) * 100
    field = dev(np.ascontiguousarray(values.T).reshape(3, 1, 1, V))
    mask = dev(np.random.default_rng(5).random((1, 1, V)) < 0.5)
    g = line_grid(V)
    a, b = field_mean_device(field, g, mask=mask), field_mean_device(field, g, mask=mask)
    assert a[0].data_ptr() != b[0].data_ptr()
    assert same_bits(a[0].cpu().numpy(), b[0].cpu().numpy()) and int(a[1]) == int(b[1])
    assert same_bits(a[0].cpu().numpy(), R.field_sums(values.astype(F64), mask.cpu().numpy().reshape(-1))[0])


# ---- (b) the segmentation sampled in its own grid ----------------------------------------------------------------------------------------
def blob(shape, seed, kind):
    """a blob on (z, y, x) = shape: kind 0 float64 / 1 float32 values that are negative outside it, kind 2 uint8 labels 0, 1, 2"""
    noise = G.smooth_noise(shape, seed) + 0.15
    if kind == 2:
        return np.where(noise > 0.45, 2, np.where(noise > 0.0, 1, 0)).astype(np.uint8)
    return noise.astype(F32 if kind == 1 else F64)


def check_seg(field, field_grid, seg, seg_grid, quantize=None):
    """seg mode against the restatement and against the two-step path (resample_device, > 0, mask mode) -> (count, mask)"""
    mask = R.seg_mask(seg, seg_grid, field_grid)
    values = R.field_values(field, "last")
    want = R.field_sums(R.quantize_f16(values) if quantize is not None else values.astype(F64), mask.reshape(-1))
    seg_d = dev(seg)
    two_step = resample_device(seg_d, seg_grid, field_grid) > 0
    assert np.array_equal(two_step.cpu().numpy(), mask)
    for f in (dev(field), dev(np.ascontiguousarray(np.moveaxis(field, 3, 0)))):
        sums, count = field_mean_device(f, field_grid, seg=seg_d, seg_grid=seg_grid, quantize=quantize)
        assert int(count) == want[1] and same_bits(sums.cpu().numpy(), want[0]), (int(count), want[1])
        sums2, count2 = field_mean_device(f, field_grid, mask=two_step, quantize=quantize)
        assert int(count2) == int(count) and same_bits(sums2.cpu().numpy(), sums.cpu().numpy())
    return want[1], mask


@pytest.mark.parametrize("n", [1, 2, 3])
def test_seg_mode_on_the_shared_geometries(n):
    """field on the fixed image's 1 mm grid, the segmentation on the moving image's grid (own spacing, origin and axes)"""
    _, moving, gr, field = G.make_case(n)
    sg = grid_of(moving)
    for kind in (0, 1, 2):
        seg = blob(sg.size[::-1], 40 + n, kind)
        count, mask = check_seg(field, gr, seg, sg)
        assert 0 < count < mask.size, (n, kind, count)
    seg = blob(sg.size[::-1], 40 + n, 2)
    check_seg(field.astype(F32), gr, seg, sg)                             # a float32 field, as register_pair_device leaves it
    check_seg(field.astype(F32), gr, seg, sg, quantize=torch.float16)


def test_seg_mode_float32_field_with_a_float32_segmentation():
    """the one pair of element types no case above combines (a float32 field has met only integer segmentations): a (5, 4, 7) field grid,
    three distinct extents, and a float32 segmentation on a coarser, shifted grid of its own"""
    fg = Grid((7, 4, 5), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), IDENT)
    sg = Grid((5, 4, 3), (1.5, 1.2, 1.8), (-0.4, -0.3, -0.2), IDENT)
    field = G.smooth_noise((5, 4, 7), 11, amp=2.0, channels=3).astype(F32)
    count, mask = check_seg(field, fg, blob((3, 4, 5), 47, 1), sg)
    assert 0 < count < mask.size
    check_seg(field, fg, blob((3, 4, 5), 47, 1), sg, quantize=torch.float16)


def test_seg_mode_values_exactly_one_half():
    """spacing ratio 2 and a half-voxel offset: every second field voxel lies midway between two segmentation voxels, so a 0 | 1 edge
    interpolates to exactly 0.5 -- which an integer segmentation rounds to 0 (half to even) and a float one keeps above zero"""
    fg = Grid((12, 10, 8), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), IDENT)
    sg = Grid((7, 6, 5), (2.0, 2.0, 2.0), (-1.0, -1.0, -1.0), IDENT)       # segmentation index = (field index + 1) / 2
    lab = np.zeros((5, 6, 7), np.uint8)
    lab[1:4, 2:5, 2:5] = 1
    field = G.smooth_noise((8, 10, 12), 9, amp=2.0, channels=3)
    values, _ = G.resample(lab.astype(F64), sg, fg)
    half = values == 0.5
    assert half.sum() >= 20 and (values > 0.5).any() and ((values > 0) & (values < 0.5)).any()
    n_int, mask_int = check_seg(field, fg, lab, sg)
    n_f64, mask_f64 = check_seg(field, fg, lab.astype(F64), sg)
    n_f32, mask_f32 = check_seg(field, fg, lab.astype(F32), sg)
    assert not mask_int[half].any() and mask_f64[half].all() and mask_f32[half].all()
    assert np.array_equal(mask_int, values > 0.5) and np.array_equal(mask_f64, values > 0) and n_int < n_f64 == n_f32


def test_seg_mode_mostly_outside():
    """the 45 degree case of the geometry tests: most field voxels fall outside the segmentation's buffer and take the default 0"""
    rng = np.random.default_rng(7)
    sg = Grid((8, 8, 6), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), IDENT)
    fg = Grid((14, 14, 10), (1.0, 1.0, 1.0), (3.5, -5.0, -2.0), tuple(G.rot_z(np.pi / 4).reshape(-1)))
    field = G.smooth_noise((10, 14, 14), 8, amp=2.0, channels=3)
    for seg in (rng.random((6, 8, 8)) + 0.01, (rng.random((6, 8, 8)) + 0.01).astype(F32), rng.integers(1, 4, (6, 8, 8)).astype(np.int16)):
        count, mask = check_seg(field, fg, seg, sg)
        _, ci = G.resample(seg, sg, fg)
        inside = np.all((ci >= -0.5) & (ci <= np.array([8.0, 8.0, 6.0]).reshape(3, 1, 1, 1) - 0.5), axis=0)
        assert inside.mean() < 0.5 and np.array_equal(mask, inside) and count == int(inside.sum())       # positive everywhere inside


# ---- (c) end to end ------------------------------------------------------------------------------------------------------------------
def host_value_before_rounding(fixed, moving, seg):
    """the host path of convex_adam_translation up to mean / spacing (z, y, x)"""
    from convexadam_amd.convex_adam_MIND import convex_adam_pt
    from convexadam_amd.convex_adam_utils import resample_img, resample_moving_to_fixed
    fixed_1mm = resample_img(fixed, spacing=(1.0, 1.0, 1.0))
    field = convex_adam_pt(img_fixed=fixed_1mm, img_moving=resample_moving_to_fixed(fixed_1mm, moving))
    mask = resample_moving_to_fixed(moving=seg, fixed=fixed_1mm).array > 0 if seg is not None else None
    mean = np.mean(field[mask], axis=0) if mask is not None else np.mean(field, axis=(0, 1, 2))
    return mean / np.array(moving.GetSpacing()[::-1])


@pytest.mark.parametrize("name", TC.NAMES)
def test_translation_device_path_matches_the_host_path(name):
    """Same whole-voxel translation and same moved origin as device=None.  The cases of TC.TIE_FREE first assert that the host path's
    value before rounding lies at least 0.25 from a half-integer (a condition on the inputs).  known_shift cannot meet that condition
    with the inputs it is defined by (2.616 along z, 0.116 from 2.5, for every phantom seed tried: tests/translation_cases.py); it
    asserts the known answer (-2, 0, 3) and the reference test's own criterion instead, and shift_2_1_-1 is the tie-free case without a
    segmentation."""
    from convexadam_amd.convex_adam_translation import convex_adam_translation, translation_mean_device
    fixed, moving, seg, shift = TC.make(name)
    pre = host_value_before_rounding(fixed, moving, seg)
    print(name, "host value before rounding (z, y, x):", pre, "distance from a half-integer:", np.abs(pre - np.floor(pre) - 0.5))
    if name in TC.TIE_FREE:
        assert np.all(np.abs(pre - np.floor(pre) - 0.5) >= 0.25), pre
    co = [moving.copy()]
    t_host, moved_host, _ = convex_adam_translation(fixed, moving, segmentation=seg)
    t_dev, moved_dev, co_dev = convex_adam_translation(fixed, moving, segmentation=seg, co_moving_images=co, device=DEV)
    assert tuple(t_dev) == tuple(t_host), (t_dev, t_host)
    assert moved_dev.GetOrigin() == moved_host.GetOrigin() == co_dev[0].GetOrigin() and np.array_equal(moved_dev.array, moving.array)
    assert moved_dev.GetSpacing() == moving.GetSpacing()
    mean_dev, _ = translation_mean_device(fixed, moving, seg, DEV)
    print(name, "device mean (z, y, x):", mean_dev, "host mean:", pre * np.array(moving.GetSpacing()[::-1]))
    if name in ("known_shift", "segmentation"):
        assert tuple(t_dev) == (-2.0, 0.0, 3.0)
    if name != "segmentation":                                            # the reference test's criterion: within one unit of the applied shift
        assert np.allclose(np.array(t_dev), np.array(shift, float)[::-1], atol=1.0)
        assert np.allclose(mean_dev, np.array(shift, float), atol=1.0)


@pytest.mark.parametrize("name", ["known_shift", "segmentation"])
def test_downloaded_mean_is_the_restatement_of_its_field_and_mask(name):
    from convexadam_amd.convex_adam_translation import register_on_1mm_device, translation_mean_device
    fixed, moving, seg, _ = TC.make(name)
    field, gr = register_on_1mm_device(fixed, moving, DEV)
    assert field.dtype == torch.float32 and tuple(field.shape) == (3,) + TC.SHAPE and gr.size == TC.SHAPE[::-1]
    mask = R.seg_mask(seg.array, grid_of(seg), gr).reshape(-1) if seg is not None else None
    sums, count = R.field_mean(field.cpu().numpy(), "first", mask, quantize=True)
    mean, n = translation_mean_device(fixed, moving, seg, DEV)
    assert n == count and same_bits(mean, sums / np.float64(count))
    if seg is not None:
        assert 0 < count < mask.size and n == 12232                       # the host path's mask has as many voxels (CPU oracle run)


def test_empty_segmentation_is_refused_on_the_device_path():
    from convexadam_amd.convex_adam_translation import convex_adam_translation
    from convexadam_amd.imageio import Image
    fixed, moving, seg, _ = TC.make("segmentation")
    empty = Image(np.zeros_like(seg.array), seg.GetSpacing(), seg.GetOrigin(), seg.GetDirection())
    with pytest.raises(ValueError, match="empty"):
        convex_adam_translation(fixed, moving, segmentation=empty, device=DEV)
