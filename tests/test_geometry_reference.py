"""CPU: the float64 restatement of csrc/geometry.hip's contract (tests/geometry_restatement.py) against the host functions the device
path stands beside -- imageio.resample, rescale_displacement_field and scipy's map_coordinates(order=1) as apply_convex restates it --
so that the bit-for-bit GPU tests (tests/test_gpu_geometry.py) rest on something.

The two sides differ only in how the source coordinate is evaluated (element-wise in the contract's order there, a BLAS product here).
Bounds, derived per case from the case's own numbers (geometry_restatement.bound_*):
    interpolation   B_i = 64 eps max(|ci|, 1) 3 range(source)
    carried field   B_c = (3 B_i + 8 eps max|field|) max(ratio)
    warped volume   B_w = 3 B_c range(moving) + 64 eps max|moving|
Voxels whose reference coordinate lies within 1e-9 of an inside/outside boundary without being on it are left out (the two sides may
disagree there by a whole value); at most 0.1 % of a case's voxels, and in these cases none.  Observed: differences 0 .. 9e-15 against
bounds 3.5e-11 .. 1.3e-9; smallest distance of a resampling coordinate to a boundary 9e-4."""
import os
import sys

import numpy as np
import pytest
from scipy.ndimage import map_coordinates

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_restatement as G  # noqa: E402
from convexadam_amd import imageio  # noqa: E402
from convexadam_amd.convex_adam_utils import rescale_displacement_field  # noqa: E402
from convexadam_amd.geometry import field_frame, grid_of, index_map, resampled_grid  # noqa: E402


def left_out(mask, what):
    frac = float(mask.mean())
    print("%s: %d of %d voxels left out" % (what, int(mask.sum()), mask.size))
    assert frac <= G.MAX_LEFT_OUT, what
    return ~mask


def resample_boundaries(ci, src_shape):
    n = src_shape[::-1]
    return G.near_boundary(ci, [-0.5] * 3, [n[a] - 0.5 for a in range(3)])


def warp_boundaries(c, shape):
    return G.near_boundary(c, [0.0] * 3, [shape[a] - 1.0 for a in range(3)])


@pytest.fixture(scope="module", params=[1, 2, 3])
def case(request):
    return (request.param,) + G.make_case(request.param)


def test_index_map_is_the_host_paths(case):
    """geometry.index_map and resampled_grid give imageio.resample's / resample_img's numbers (same operations)"""
    from convexadam_amd.convex_adam_utils import resample_img
    n, fixed, moving, gr, field = case
    host = resample_img(fixed, (1.0, 1.0, 1.0))
    assert grid_of(host) == gr
    Ao, oo = host.index_to_physical_matrix()
    As, os_ = moving.index_to_physical_matrix()
    M, t = index_map(moving, gr)
    assert np.array_equal(M, np.linalg.solve(As, Ao)) and np.array_equal(t, np.linalg.solve(As, oo - os_))


def test_resampling_restatement_vs_host(case):
    n, fixed, moving, gr, field = case
    for name, src in (("fixed", fixed), ("moving", moving)):
        for dt in (np.float64, np.float32):
            img = imageio.Image(src.array.astype(dt), src.GetSpacing(), src.GetOrigin(), src.GetDirection())
            host = imageio.resample(img, gr.spacing, gr.size, gr.direction, gr.origin).array
            mine, ci = G.resample(img.array, grid_of(img), gr)
            assert mine.dtype == host.dtype == dt and mine.shape == host.shape
            keep = left_out(resample_boundaries(ci, img.array.shape), "case %d %s" % (n, name))
            b = G.bound_interp(ci, img.array) + (2.0 ** -23 * float(np.abs(img.array).max()) if dt == np.float32 else 0.0)   # + one float32 ulp: each side rounds once
            d = float(np.abs(mine.astype(np.float64) - host.astype(np.float64))[keep].max())
            print("case %d %s %s: diff %.3g, bound %.3g" % (n, name, np.dtype(dt).name, d, b))
            assert d <= b
            assert 0.05 < float((mine != 0).mean()) < 1.0 or name == "fixed"          # the case has an inside and an outside


def test_integer_source_rounds_half_even_like_the_host():
    """integer sources: interpolated in float64, cast back with np.rint; a half-voxel shift puts every interior value on k + 0.5"""
    src = imageio.Image(np.arange(4 * 5 * 6, dtype=np.int16).reshape(4, 5, 6), (1.0, 1.0, 1.0))
    out_grid = grid_of(imageio.Image(np.zeros((4, 5, 6)), (1.0, 1.0, 1.0), (0.5, 0.0, 0.0)))
    host = imageio.resample(src, out_grid.spacing, out_grid.size, out_grid.direction, out_grid.origin).array
    mine, ci = G.resample(src.array, grid_of(src), out_grid)
    assert mine.dtype == np.int16 and np.array_equal(mine, host)
    vals = G.interpolate_itk(src.array, ci)
    halves = vals[..., :5]
    assert np.all(halves - np.floor(halves) == 0.5)
    below = np.floor(halves)
    assert np.array_equal(mine[..., :5], np.where(below % 2 == 0, below, below + 1).astype(np.int16))     # the even neighbour
    assert np.any(mine[..., :5] != np.floor(halves + 0.5))                                              # ... which half-up is not


def test_carried_field_and_warp_restatement_vs_host(case):
    n, fixed, moving, gr, field = case
    fixed_r = G.grid_image(gr)
    host = rescale_displacement_field(field, moving, fixed, fixed_r)
    mine, ci = G.carry_field(field, moving, fixed, gr)
    assert host.shape == mine.shape == moving.array.shape + (3,) and mine.dtype == np.float64
    edge = resample_boundaries(ci, field.shape[:3])
    keep = left_out(edge, "case %d carried" % n)
    _, ratio = field_frame(moving, fixed, gr)
    b_c = G.bound_carried(ci, field, ratio)
    d = float(np.abs(mine - host)[keep].max())
    print("case %d carried: diff %.3g, bound %.3g" % (n, d, b_c))
    assert d <= b_c
    assert np.any(mine != 0) and np.any(np.all(mine == 0, -1))           # part of the moving grid lies outside the fixed grid

    # the warp: scipy's map_coordinates(order=1) of the host's field (what apply_convex restates) against the restatement's
    ident = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in moving.array.shape], indexing="ij")
    host_w = map_coordinates(moving.array.astype(np.float64), [host[..., a] + ident[a] for a in range(3)], order=1)
    mine_w = G.warp(moving.array, mine)
    keep = left_out(edge | warp_boundaries(G.warp_coordinates(host), moving.array.shape), "case %d warped" % n)
    b_w = G.bound_warped(b_c, moving.array)
    d = float(np.abs(mine_w - host_w)[keep].max())
    print("case %d warped: diff %.3g, bound %.3g" % (n, d, b_w))
    assert d <= b_w
    assert np.any(mine_w == 0) and float((mine_w != 0).mean()) > 0.3


def test_restatement_edges():
    """the restatement itself: identity map returns the input; extent-1 and extent-2 axes; outside gives the default"""
    rng = np.random.default_rng(5)
    for shape in ((4, 5, 6), (1, 5, 6), (4, 1, 6), (4, 5, 1), (2, 5, 6), (4, 5, 2)):
        img = imageio.Image(rng.random(shape), (0.7, 1.3, 2.1), (1.0, -2.0, 3.0), G.rot_z(0.3).reshape(-1))
        out, _ = G.resample(img.array, grid_of(img), grid_of(img))
        assert np.array_equal(out, img.array), shape
        shifted = grid_of(imageio.Image(img.array, (0.7, 1.3, 2.1), (1.0 + 0.35, -2.0, 3.0), G.rot_z(0.3).reshape(-1)))
        host = imageio.resample(img, shifted.spacing, shifted.size, shifted.direction, shifted.origin).array
        mine, ci = G.resample(img.array, grid_of(img), shifted)
        assert float(np.abs(mine - host).max()) <= G.bound_interp(ci, img.array), shape
    far = grid_of(imageio.Image(np.zeros((3, 3, 3)), (1.0, 1.0, 1.0), (100.0, 0.0, 0.0)))
    out, _ = G.resample(img.array, grid_of(img), far, default=-7.5)
    assert np.all(out == -7.5)
    assert resampled_grid(grid_of(img), (1.0, 1.0, 1.0)).size == tuple(int(n * s + 0.5) for n, s in zip(grid_of(img).size, (0.7, 1.3, 2.1)))
