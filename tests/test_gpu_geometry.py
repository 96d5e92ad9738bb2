"""The geometry kernels (csrc/geometry.hip) on the device.

Bit for bit against the float64 restatement of their contract (tests/geometry_restatement.py: the coordinate evaluated element-wise in
the contract's order, scipy's map_coordinates(order=1) for the taps), and against apply_convex's own kernel for the warp.  Against the
parent's host functions (imageio.resample, rescale_displacement_field, apply_convex_original_moving with device=None), which evaluate
the coordinate through BLAS, within the bounds derived in tests/test_geometry_reference.py (B_i, B_c, B_w; a float32 result adds one
float32 ulp of the largest value: each side rounds once) and under its condition (voxels whose reference coordinate lies within 1e-9
of an inside/outside boundary without being on it are left out, at most 0.1 %)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_restatement as G  # noqa: E402
from test_geometry_reference import left_out, resample_boundaries, warp_boundaries  # noqa: E402

from convexadam_amd import geometry, imageio  # noqa: E402
from convexadam_amd.geometry import Grid, field_frame, grid_of, index_map  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = np.float32, np.float64
TORCH_OF = {np.dtype(F32): torch.float32, np.dtype(F64): torch.float64}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                     # (a copy: the shared arrays are read-only)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def raw_resample(src, src_grid, out_grid, out_dtype, default=0.0):
    """cvx_resample_linear_f64 with its own output dtype (the Python function keeps the source's) -> numpy"""
    from convexadam_amd._lib import check, lib, ptr, stream_ptr
    sg, og = grid_of(src_grid), grid_of(out_grid)
    M, t = index_map(sg, og)
    s = dev(src)
    out = torch.empty(og.size[::-1], dtype=TORCH_OF[np.dtype(out_dtype)], device=DEV)
    m = (C.c_double * 12)(*np.concatenate([M.reshape(-1), t]).tolist())
    check(lib().cvx_resample_linear_f64(ptr(s), int(s.dtype == torch.float64), *s.shape, ptr(out), int(out.dtype == torch.float64), *out.shape, m,
                                        float(default), stream_ptr(s.device)))
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    """the three shared geometries with everything the restatement says about them, computed once and read-only"""
    out = {}
    for n in (1, 2, 3):
        fixed, moving, gr, field = G.make_case(n)
        carried, ci = G.carry_field(field, moving, fixed, gr)
        c = dict(fixed=fixed, moving=moving, gr=gr, field=field, carried=carried, ci=ci, warped=G.warp(moving.array, carried))
        for v in (fixed.array, moving.array, field, carried, ci, c["warped"]):
            v.setflags(write=False)
        out[n] = c
    return out


def edge_cases():
    rng = np.random.default_rng(7)
    ident = tuple(np.eye(3).reshape(-1))
    mk = lambda shape, sp, org=(0.0, 0.0, 0.0), d=ident: Grid(tuple(shape[::-1]), sp, org, tuple(np.asarray(d).reshape(-1)))   # noqa: E731
    return {
        # name: (source (z, y, x), source grid, output grid, default)
        "source_z_extent_1": (rng.random((1, 5, 6)), mk((1, 5, 6), (1.0, 1.0, 2.0)), mk((3, 7, 8), (0.7, 0.6, 0.9), (-0.4, -0.3, -1.2), G.rot_z(0.1)), 0.0),
        "source_x_extent_1": (rng.random((5, 6, 1)), mk((5, 6, 1), (2.0, 1.0, 1.0)), mk((6, 7, 4), (0.9, 0.8, 0.9), (-1.3, -0.3, -0.2), G.rot_y(0.05)), 0.0),
        "source_y_extent_2": (rng.random((5, 2, 6)), mk((5, 2, 6), (1.0, 1.5, 1.0)), mk((6, 8, 7), (0.8, 0.5, 0.9), (-0.2, -1.0, -0.3), G.rot_x(0.1)), 0.0),
        "output_x_extent_1": (rng.random((6, 7, 5)), mk((6, 7, 5), (1.0, 1.0, 1.0)), mk((9, 11, 1), (0.6, 0.7, 0.7), (1.7, -1.3, -0.9), G.rot_z(-0.2)), 0.0),
        "output_12x10x9": (rng.random((7, 6, 8)), mk((7, 6, 8), (0.9, 1.1, 1.2)), mk((12, 10, 9), (0.8, 0.7, 0.75), (-0.3, -0.2, -0.6), G.rot_x(0.07)), 1.25),
        "rotated_45_mostly_outside": (rng.random((6, 8, 8)), mk((6, 8, 8), (1.0, 1.0, 1.0)), mk((10, 14, 14), (1.0, 1.0, 1.0), (3.5, -5.0, -2.0), G.rot_z(np.pi / 4)), -7.5),
    }


# ---- (a) resampling, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_resample_cases_bits(cases, n):
    c = cases[n]
    for name in ("fixed", "moving"):
        img = c[name]
        for sd in (F32, F64):
            src = img.array.astype(sd)
            for od in (F32, F64):
                want, _ = G.resample(src, grid_of(img), c["gr"], out_dtype=od)
                got = raw_resample(src, img, c["gr"], od)
                assert same_bits(got, want), (n, name, sd, od, float(np.abs(got.astype(F64) - want.astype(F64)).max()))
            got = geometry.resample_device(dev(src), img, c["gr"])              # the Python function: source dtype out
            assert got.is_cuda and same_bits(got.cpu().numpy(), G.resample(src, grid_of(img), c["gr"])[0])


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_resample_edges_bits(name):
    src, sg, og, default = edge_cases()[name]
    for sd in (F32, F64):
        for od in (F32, F64):
            want, ci = G.resample(src.astype(sd), sg, og, default=default, out_dtype=od)
            got = raw_resample(src.astype(sd), sg, og, od, default)
            assert same_bits(got, want), (name, sd, od)
    want, ci = G.resample(src, sg, og, default=default)
    got = geometry.resample_device(dev(src), sg, og, default=default).cpu().numpy()
    assert same_bits(got, want)
    lim = np.array(src.shape[::-1], F64).reshape(3, 1, 1, 1)
    outside = ~np.all((ci >= -0.5) & (ci <= lim - 0.5), axis=0)
    assert outside.any() and not outside.all() and np.all(got[outside] == default)           # every case has both sides of the rule
    if name == "rotated_45_mostly_outside":
        assert outside.mean() > 0.5 and np.all(got[~outside] >= 0.0)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_identity_map_returns_the_input(dtype):
    rng = np.random.default_rng(3)
    src = (rng.standard_normal((5, 9, 31)) * 1e3).astype(dtype)                               # 1395 voxels: six blocks, the last one partial
    g = Grid((31, 9, 5), (0.7, 1.3, 2.1), (4.0, -2.0, 1.0), tuple(np.eye(3).reshape(-1)))
    M, t = index_map(g, g)
    assert np.array_equal(M, np.eye(3)) and np.array_equal(t, np.zeros(3))
    got = geometry.resample_device(dev(src), g, g, default=-1.0)
    assert same_bits(got.cpu().numpy(), src)
    # a turned grid onto itself: the solve leaves entries of 1e-19 beside the identity, which no coordinate of this size can see
    g = Grid((31, 9, 5), (0.7, 1.3, 2.1), (4.0, -2.0, 1.0), tuple(G.rot_z(0.3).reshape(-1)))
    M, t = index_map(g, g)
    assert float(np.abs(M - np.eye(3)).max()) < 1e-15 and float(np.abs(t).max()) < 1e-15
    got = geometry.resample_device(dev(src), g, g, default=-1.0)
    assert same_bits(got.cpu().numpy(), src)


def test_integer_source_rounds_half_even():
    src = np.arange(4 * 5 * 6, dtype=np.int16).reshape(4, 5, 6)
    sg = Grid((6, 5, 4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).reshape(-1)))
    og = Grid((6, 5, 4), (1.0, 1.0, 1.0), (0.5, 0.0, 0.0), tuple(np.eye(3).reshape(-1)))      # half a voxel along x: values k + 0.5
    want, _ = G.resample(src, sg, og)
    got = geometry.resample_device(dev(src), sg, og)
    assert got.dtype == torch.int16 and same_bits(got.cpu().numpy(), want)
    below = src[..., :5].astype(F64)
    assert np.array_equal(got.cpu().numpy()[..., :5], np.where(below % 2 == 0, below, below + 1))
    for dt in (np.uint8, np.int32, np.int64):
        got = geometry.resample_device(dev(src.astype(dt)), sg, og)
        assert same_bits(got.cpu().numpy(), want.astype(dt))


# ---- (b) carried field, bit for bit, from both layouts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_carried_field_bits(cases, n):
    c = cases[n]
    args = (c["moving"], c["fixed"], c["gr"])
    got = geometry.rescale_displacement_field_device(dev(c["field"]), *args)
    assert got.dtype == torch.float64 and got.is_cuda and same_bits(got.cpu().numpy(), c["carried"])
    planar64 = np.ascontiguousarray(np.moveaxis(c["field"], -1, 0))
    assert same_bits(geometry.rescale_displacement_field_device(dev(planar64), *args).cpu().numpy(), c["carried"])
    # the float32 planar field (register_pair_device's) gives the bits of its float64 copy
    planar32 = planar64.astype(F32)
    copy64 = np.ascontiguousarray(np.moveaxis(planar32.astype(F64), 0, -1))
    want, _ = G.carry_field(copy64, *args)
    a = geometry.rescale_displacement_field_device(dev(planar32), *args).cpu().numpy()
    b = geometry.rescale_displacement_field_device(dev(copy64), *args).cpu().numpy()
    assert same_bits(a, b) and same_bits(a, want)
    assert same_bits(geometry.rescale_displacement_field_device(dev(copy64.astype(F32)), *args).cpu().numpy(), want)       # float32 interleaved


# ---- (c) warped output: apply_convex's kernel on the restated field ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_warped_bits_of_apply_convex(cases, n):
    from convexadam_amd.apply_convex import apply_convex
    c = cases[n]
    args = (c["moving"], c["fixed"], c["gr"])
    field = dev(c["field"])
    for md in (F64, F32):
        mov = c["moving"].array.astype(md)
        want = apply_convex(disp=c["carried"], moving=mov.astype(F64))                       # the existing kernel on the existing path
        assert want.dtype == F64
        if md == F64:
            assert same_bits(want, c["warped"])                                              # ... which the restatement agrees with
        for wd, tdt in ((F64, torch.float64), (F32, torch.float32)):
            carried, warped = geometry.rescale_displacement_field_device(field, *args, moving=dev(mov), warped_dtype=tdt)
            assert same_bits(carried.cpu().numpy(), c["carried"])
            assert same_bits(warped.cpu().numpy(), want.astype(wd)), (n, md, wd)
    assert np.any(want == 0) and float((want != 0).mean()) > 0.3


def test_float32_field_with_a_float64_moving_volume_or_warped_output():
    """The element types of cvx_field_to_grid_f64 that no case above combines: a float32 field (both layouts) with a float64 moving volume
    or a float64 warped output.  A (z, y, x) = (5, 4, 7) field grid -- three distinct extents, one partial block -- and a turned moving
    grid of another spacing, against the restatement."""
    ident = tuple(np.eye(3).reshape(-1))
    gr = Grid((7, 4, 5), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), ident)
    fg = Grid((4, 4, 3), (2.0, 1.0, 1.5), (0.0, 0.0, 0.0), tuple(G.rot_z(0.1).reshape(-1)))
    mg = Grid((6, 5, 4), (1.1, 0.8, 1.3), (0.4, -0.3, 0.2), tuple(G.rot_x(0.15).reshape(-1)))
    field32 = G.smooth_noise((5, 4, 7), 51, amp=1.5, channels=3).astype(F32)
    mov64 = G.smooth_noise((4, 5, 6), 52) + 0.5
    carried, _ = G.carry_field(field32.astype(F64), mg, fg, gr)
    for md, wd in ((F64, F64), (F64, F32), (F32, F64)):
        mov = mov64.astype(md)
        want = G.warp(mov, carried)
        assert 0.3 < float((want != 0).mean()) < 1.0                                         # both sides of apply_convex's rule
        for f in (field32, np.ascontiguousarray(np.moveaxis(field32, -1, 0))):
            got_c, got_w = geometry.rescale_displacement_field_device(dev(f), mg, fg, gr, moving=dev(mov), warped_dtype=TORCH_OF[np.dtype(wd)])
            assert same_bits(got_c.cpu().numpy(), carried), (md, wd, f.shape)
            assert same_bits(got_w.cpu().numpy(), want.astype(wd)), (md, wd, f.shape)


# ---- (d) fused outputs and NaN ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_fused_equals_single_outputs_and_nan(cases, n):
    c = cases[n]
    args = (c["moving"], c["fixed"], c["gr"])
    mov = dev(c["moving"].array)
    carried, warped = geometry.rescale_displacement_field_device(dev(c["field"]), *args, moving=mov)
    only_c = geometry.rescale_displacement_field_device(dev(c["field"]), *args)
    only_w = geometry.rescale_displacement_field_device(dev(c["field"]), *args, moving=mov, want_field=False)
    assert warped.dtype == torch.float32 and torch.equal(carried, only_c) and torch.equal(warped, only_w)

    bad = c["field"].copy()
    q = tuple(s // 2 for s in bad.shape[:3])
    bad[q] = np.nan                                                                          # one NaN vector
    want, _ = G.carry_field(bad, *args)
    hit = np.isnan(want).any(-1)                                                             # the moving voxels that interpolate it
    assert 1 <= hit.sum() < hit.size // 4 and np.all(np.isnan(want[hit]))
    carried_n, warped_n = geometry.rescale_displacement_field_device(dev(bad), *args, moving=mov)
    carried_n, warped_n = carried_n.cpu().numpy(), warped_n.cpu().numpy()
    assert np.array_equal(np.isnan(carried_n), np.isnan(want)) and same_bits(carried_n[~hit], c["carried"][~hit])
    assert np.all(warped_n[hit] == 0.0) and same_bits(warped_n[~hit], warped.cpu().numpy()[~hit])


# ---- against the parent's host functions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_against_the_host_functions(cases, n):
    from convexadam_amd.apply_convex import apply_convex_original_moving
    from convexadam_amd.convex_adam_utils import rescale_displacement_field
    c = cases[n]
    fixed, moving, gr, field = c["fixed"], c["moving"], c["gr"], c["field"]
    for name, img in (("fixed", fixed), ("moving", moving)):
        host = imageio.resample(img, gr.spacing, gr.size, gr.direction, gr.origin).array
        _, ci = G.resample(img.array, grid_of(img), gr)
        got = geometry.resample_device(dev(img.array), img, gr).cpu().numpy()
        keep = left_out(resample_boundaries(ci, img.array.shape), "case %d %s" % (n, name))
        d, b = float(np.abs(got - host)[keep].max()), G.bound_interp(ci, img.array)
        print("case %d %s: diff %.3g, B_i %.3g" % (n, name, d, b))
        assert d <= b
    fixed_r = G.grid_image(gr)
    host_c = rescale_displacement_field(field, moving, fixed, fixed_r)
    carried, warped = geometry.rescale_displacement_field_device(dev(field), moving, fixed, gr, moving=dev(moving.array))
    edge = resample_boundaries(c["ci"], field.shape[:3])
    keep = left_out(edge, "case %d carried" % n)
    b_c = G.bound_carried(c["ci"], field, field_frame(moving, fixed, gr)[1])
    d = float(np.abs(carried.cpu().numpy() - host_c)[keep].max())
    print("case %d carried: diff %.3g, B_c %.3g" % (n, d, b_c))
    assert d <= b_c
    host_w = apply_convex_original_moving(field, moving, fixed, fixed_r)
    assert isinstance(host_w, imageio.Image) and host_w.array.dtype == F32
    keep = left_out(edge | warp_boundaries(G.warp_coordinates(host_c), moving.array.shape), "case %d warped" % n)
    b_w = G.bound_warped(b_c, moving.array) + 2.0 ** -23 * float(np.abs(moving.array).max())
    d = float(np.abs(warped.cpu().numpy().astype(F64) - host_w.array.astype(F64))[keep].max())
    print("case %d warped: diff %.3g, B_w (+ one float32 ulp) %.3g" % (n, d, b_w))
    assert d <= b_w


# ---- the device= keyword of the four public functions ---------------------------------------------------------------------------------------
def test_device_keyword_returns_the_host_paths_types(cases):
    from convexadam_amd.apply_convex import apply_convex_original_moving
    from convexadam_amd.convex_adam_utils import resample_img, resample_moving_to_fixed, rescale_displacement_field
    c = cases[2]
    gr, field = c["gr"], c["field"]
    for dt in (F32, F64, np.int16):
        scale = 1.0 if dt != np.int16 else 1000.0
        fixed = imageio.Image((c["fixed"].array * scale).astype(dt), *grid_of(c["fixed"])[1:])
        moving = imageio.Image((c["moving"].array * scale).astype(dt), *grid_of(c["moving"])[1:])
        a = resample_img(fixed, (1.0, 1.0, 1.0), device=DEV)
        assert isinstance(a, imageio.Image) and grid_of(a) == gr and a.array.dtype == dt
        assert same_bits(a.array, G.resample(fixed.array, grid_of(fixed), gr)[0])
        b = resample_moving_to_fixed(a, moving, device=DEV)
        assert isinstance(b, imageio.Image) and grid_of(b) == gr and b.array.dtype == dt
        assert same_bits(b.array, G.resample(moving.array, grid_of(moving), gr)[0])
        host = resample_moving_to_fixed(a, moving)
        assert type(host) is type(b) and grid_of(host) == grid_of(b) and host.array.dtype == b.array.dtype
    fixed, moving = c["fixed"], c["moving"]
    fixed_r = resample_img(fixed, (1.0, 1.0, 1.0), device=DEV)
    r = rescale_displacement_field(np.array(field), moving, fixed, fixed_r, device=DEV)
    host = rescale_displacement_field(field, moving, fixed, fixed_r)
    assert isinstance(r, np.ndarray) and r.dtype == host.dtype == F64 and r.shape == host.shape and same_bits(r, c["carried"])
    w = apply_convex_original_moving(field, moving, fixed, fixed_r, device=DEV)
    assert isinstance(w, imageio.Image) and w.array.dtype == F32 and grid_of(w) == grid_of(moving)
    assert same_bits(w.array, c["warped"].astype(F32))
    w_t = apply_convex_original_moving(torch.from_numpy(np.array(field)), moving, fixed, fixed_r, device=DEV)               # a tensor field, like the host path takes
    assert same_bits(w_t.array, w.array)


# ---- the whole flow -----------------------------------------------------------------------------------------------------------------------
def test_register_images_is_the_composition_of_its_pieces():
    from convexadam_amd.convex_adam_MIND import register_pair_device
    from convexadam_amd.phantom import phantom
    from convexadam_amd.ssim import registration_ssim, ssim3D
    shape = (48, 48, 40)
    fixed = imageio.Image(phantom(shape, 1, 10).numpy(), (1.0, 1.0, 1.0))
    shifted = imageio.Image(torch.roll(phantom(shape, 1, 11), 3, 1).numpy(), (1.0, 1.0, 1.0))      # the same phantom, 3 voxels along y
    # ... given 0.8 x 0.8 x 1.25 mm voxels and axes turned by 10 degrees about z, around the volume's centre
    sp, size, D = (0.8, 0.8, 1.25), (50, 60, 38), G.rot_z(np.deg2rad(10.0))
    centre = (np.array(shape[::-1], F64) - 1) / 2
    origin = centre - (D * np.array(sp)[None, :]) @ ((np.array(size, F64) - 1) / 2)
    moving = imageio.resample(shifted, sp, size, D.reshape(-1), origin)
    assert moving.array.dtype == F32 and float((moving.array != 0).mean()) > 0.8
    kw = dict(grid_sp=4, disp_hw=3, selected_niter=20, grid_sp_adam=2)
    res = geometry.register_images(fixed, moving, device=DEV, **kw)

    gf, gm = grid_of(fixed), grid_of(moving)
    gr = geometry.resampled_grid(gf, (1.0, 1.0, 1.0))
    assert gr == gf
    fx, mv = dev(fixed.array), dev(moving.array)
    fix_r, mov_r = geometry.resample_device(fx, gf, gr), geometry.resample_device(mv, gm, gr)
    assert torch.equal(fix_r, fx)                                                                 # 1 mm already: the identity map
    field = register_pair_device(fix_r, mov_r, **kw)
    carried, warped = geometry.rescale_displacement_field_device(field, gm, gf, gr, moving=mv)
    assert res.field.dtype == torch.float32 and res.field.is_cuda and torch.equal(res.field, field)
    assert res.carried_field.dtype == torch.float64 and res.carried_field.is_cuda and same_bits(res.carried_field.cpu().numpy(), carried.cpu().numpy())
    assert isinstance(res.warped, imageio.Image) and res.warped.array.dtype == F32 and grid_of(res.warped) == gm
    assert same_bits(res.warped.array, warped.cpu().numpy())
    before = float(ssim3D(fix_r[None, None], mov_r[None, None]))
    after = float(registration_ssim(fix_r, mov_r, field))
    print("ssim before %.4f after %.4f" % (before, after))
    assert res.ssim_before == before and res.ssim_after == after
    assert res.ssim_after > res.ssim_before                                                       # the reference test's own criterion
