"""The crop-field kernel (csrc/cropfield.hip) on the device, bit for bit against the numpy restatement of its contract
(tests/cropfield_restatement.py) and against CPU F.interpolate; on the golden inputs also against the reference's own output under the
criterion of tests/test_cropfield_reference.py.  All shapes are tiny."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cropfield_restatement as R  # noqa: E402
from test_cropfield_reference import TAGS, check_against_reference, golden_case  # noqa: E402

from convexadam_amd import cropfield  # noqa: E402
from convexadam_amd.cropfield import CROP_FIELD_VOXELS, CROP_IDENTITY, CROP_OUT_F32, CropCase  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, F32 = np.float16, np.float32
PRE_FIX, PRE_MOV = (2.0, 1.75, 2.5), (1.5, 2.25, 2.0)              # spacings of the two preprocessed images (voxel-field mode)
SENTINEL = 12345.0


def same(a, b):
    """same dtype, shape and bits; two NaNs count as the same whatever their payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = np.uint16 if a.dtype == F16 else np.uint32
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def launch(field, geom, full, flip=3, voxels=False, identity=False, out_dtype=F32, layout="planar", offset=0):
    """cvx_crop_field_half_f32 on a numpy field (H, W, D, 3) uploaded in `layout`; the output sits `offset` elements into a larger
    buffer whose other elements must come back untouched -> numpy (3, S0 // 2, S1 // 2, S2 // 2)"""
    from convexadam_amd._lib import check, lib, ptr, stream_ptr
    field = np.asarray(field, F32)
    n = field.shape[:3]
    if layout == "planar":
        f, cs, vs = torch.from_numpy(np.ascontiguousarray(np.moveaxis(field, 3, 0))).to(DEV), n[0] * n[1] * n[2], 1
    else:
        f, cs, vs = torch.from_numpy(np.array(field)).to(DEV), 1, 3
    oshape = (3,) + tuple(s // 2 for s in full)
    count = int(np.prod(oshape))
    buf = torch.full((count + 16,), SENTINEL, dtype=torch.float32 if out_dtype == F32 else torch.float16, device=DEV)
    out = buf[offset:offset + count]
    flags = (CROP_FIELD_VOXELS if voxels else 0) | (CROP_IDENTITY if identity else 0) | (CROP_OUT_F32 if out_dtype == F32 else 0)
    g = (C.c_double * 27)(*np.asarray(geom, np.float64).tolist()) if geom is not None else None
    check(lib().cvx_crop_field_half_f32(ptr(f), cs, vs, n[0], n[1], n[2], g, full[0], full[1], full[2], flip, flags, ptr(out), stream_ptr(f.device)))
    host = buf.cpu().numpy()
    assert np.all(host[:offset] == out_dtype(SENTINEL)) and np.all(host[offset + count:] == out_dtype(SENTINEL)), "wrote outside its output"
    return host[offset:offset + count].reshape(oshape).copy()


def make_cases():
    """name -> (CropCase, field shape); every crop resizes to the field's grid under the case's own spacing"""
    return {
        # the whole image, no resizing: original extents (2, 3, 5), one output voxel
        "full_2x3x5": (CropCase((2, 3, 5), (2.0, 2.0, 2.0), (0, 2, 0, 3, 0, 5), (4, 4, 6), (2.0, 2.0, 2.0), (1, 3, 0, 3, 1, 6)), (2, 3, 5)),
        # original voxels outside the registration grid on both sides of every axis; 5 * 1.5 = 7.5 -> 8 and 5 * 0.5 = 2.5 -> 2 (half to even)
        "inner_11x9x7": (CropCase((11, 9, 7), (3.0, 1.0, 2.0), (3, 8, 2, 7, 1, 5), (9, 12, 8), (2.0, 1.5, 2.5), (2, 9, 1, 10, 0, 6)), (8, 2, 4)),
        # a crop that reaches beyond the image on one side, a moving crop of another size
        "over_7x6x10": (CropCase((7, 6, 10), (1.0, 4.0, 1.5), (-2, 6, 1, 4, 2, 12), (8, 8, 8), (1.2, 1.0, 0.9), (0, 5, 2, 8, 1, 7)), (4, 6, 8)),
    }


@pytest.fixture(scope="module")
def fields():
    """one random field per case, shared and read-only"""
    rng = np.random.default_rng(27)
    out = {}
    for name, (case, n) in make_cases().items():
        assert tuple(int(v) for v in case.constants()["new_shape"]) == n, name
        f = (rng.standard_normal(n + (3,)) * 4.0).astype(F32)
        f.setflags(write=False)
        out[name] = f
    return out


def every_variant(field, case, flip):
    """the launches of one case: layouts x field kinds x output types against the restatement; the float16 output is the cast of the float32 one"""
    full = case.fix_shape
    for voxels in (False, True):
        geom = case.geometry(PRE_FIX, PRE_MOV) if voxels else case.geometry()
        want = R.crop_field_half(field, geom, full, flip, voxels=voxels)
        assert np.all(np.isfinite(want))
        for layout in ("planar", "interleaved"):
            got32 = launch(field, geom, full, flip, voxels=voxels, layout=layout)
            got16 = launch(field, geom, full, flip, voxels=voxels, layout=layout, out_dtype=F16)
            assert same(got32, want), (voxels, layout, float(np.abs(got32.astype(np.float64) - want).max()))
            assert same(got16, got32.astype(F16)) and same(got16, R.crop_field_half(field, geom, full, flip, voxels=voxels, out_dtype=F16))


@pytest.mark.parametrize("name", sorted(make_cases()))
def test_kernel_bits(fields, name):
    case, _ = make_cases()[name]
    every_variant(fields[name], case, case.flip_mask)


@pytest.mark.parametrize("tag", TAGS)
def test_kernel_bits_on_the_golden_cases(golden, tag, tmp_path):
    case, field, _ = golden_case(golden, tag, tmp_path)
    every_variant(field, case, case.flip_mask)


def test_voxels_outside_the_registration_grid_take_the_border(fields):
    case, n = make_cases()["inner_11x9x7"]
    geom = case.geometry()
    for a in range(3):
        _, g, _, _ = R.axis_taps(geom, a, case.fix_shape[a], n[a])
        assert (g < 0).any() and (g > n[a] - 1).any(), a                            # both sides of every axis
    # a field that is constant along an axis beyond its first / last plane is all the kernel can see there: moving the planes beside the
    # border ones changes nothing outside the crop
    field = np.array(fields["inner_11x9x7"])
    base = launch(field, geom, case.fix_shape, flip=0)
    assert same(base, R.crop_field_half(field, geom, case.fix_shape, 0))
    inner = np.array(field)
    inner[1:-1, :, 1:-1] += 1.0
    moved = launch(inner, geom, case.fix_shape, flip=0)
    assert same(moved, R.crop_field_half(inner, geom, case.fix_shape, 0))
    assert same(moved[:, 0, :, 0], base[:, 0, :, 0]) and not same(moved, base)  # output (0, ., 0): sources 0, 1 of axes 0 and 2, all below the crop


@pytest.mark.parametrize("o2", range(1, 10))
def test_every_width_of_the_fastest_axis(o2):
    """1 .. 9 outputs per row: below, at and beyond the four outputs a thread stores at once, odd and even original extents, and every
    alignment of a row's first output (the buffer offset shifts them all)"""
    s2 = 2 * o2 + (o2 % 2)
    case = CropCase((4, 6, s2), (2.0, 2.0, 2.0), (0, 3, 1, 5, 1, 7), (5, 5, 9), (1.5, 2.0, 2.5), (0, 4, 1, 4, 1, 8))
    rng = np.random.default_rng(o2)
    field = (rng.standard_normal((3, 4, 6, 3)) * 3.0).astype(F32)
    geom = case.geometry()
    want = R.crop_field_half(field, geom, case.fix_shape, 3)
    assert want.shape == (3, 2, 3, o2)
    for offset in (0, 1, 2, 3):
        got32 = launch(field, geom, case.fix_shape, offset=offset)
        got16 = launch(field, geom, case.fix_shape, out_dtype=F16, offset=offset, layout="interleaved")
        assert same(got32, want) and same(got16, want.astype(F16)), (o2, offset)
    ident = (rng.standard_normal((4, 6, s2, 3)) * 3.0).astype(F32)
    got = launch(ident, None, (4, 6, s2), flip=0, identity=True, offset=1)
    assert same(got, R.crop_field_half(ident, None, (4, 6, s2), 0, identity=True))


@pytest.mark.parametrize("flip", range(8))
def test_flip_masks(fields, flip):
    case, _ = make_cases()["over_7x6x10"]
    field = fields["over_7x6x10"]
    geom = case.geometry(PRE_FIX, PRE_MOV)
    assert same(launch(field, geom, case.fix_shape, flip), R.crop_field_half(field, geom, case.fix_shape, flip))
    assert same(launch(field, geom, case.fix_shape, flip, voxels=True, out_dtype=F16, layout="interleaved"),
                R.crop_field_half(field, geom, case.fix_shape, flip, voxels=True, out_dtype=F16))
    ident = np.ascontiguousarray(np.broadcast_to(field[:, :1, :, :], (4, 6, 8, 3)) + np.arange(6, dtype=F32).reshape(1, 6, 1, 1))[:, :5]
    want = torch.from_numpy(ident.copy())[None]
    for a in range(3):
        if (flip >> a) & 1:
            want = want.flip(1 + a)
            want[..., a] = -want[..., a]
    want = F.interpolate(want.permute(0, 4, 1, 2, 3), scale_factor=0.5, mode="trilinear", align_corners=False)[0].numpy()
    assert same(launch(ident, None, (4, 5, 8), flip, identity=True), want)


def test_known_answers():
    # the crop is the whole image, the spacings are equal, the field is zero: nothing moves, exactly
    case = CropCase((6, 5, 9), (2.0, 2.0, 2.0), (0, 6, 0, 5, 0, 9), (6, 5, 9), (2.0, 2.0, 2.0), (0, 6, 0, 5, 0, 9))
    zero = np.zeros((6, 5, 9, 3), F32)
    for voxels in (False, True):
        geom = case.geometry((2.0, 2.0, 2.0), (2.0, 2.0, 2.0))
        for out_dtype in (F32, F16):
            got = launch(zero, geom, case.fix_shape, flip=0, voxels=voxels, out_dtype=out_dtype)
            assert got.shape == (3, 3, 2, 4) and np.all(got == 0)
    # a dyadic scale: 4 mm voxels resized to 2 mm, a constant field of t = 1.5 voxels of the registration grid is 3 mm, 0.75 original voxels
    case = CropCase((4, 4, 6), (4.0, 4.0, 4.0), (0, 4, 0, 4, 0, 6), (4, 4, 6), (4.0, 4.0, 4.0), (0, 4, 0, 4, 0, 6))
    t = np.full((8, 8, 12, 3), 1.5, F32)
    geom = case.geometry((2.0, 2.0, 2.0), (2.0, 2.0, 2.0))
    for flip in (0, 3, 4, 7):
        sign = np.array([-1.0 if (flip >> a) & 1 else 1.0 for a in range(3)], F32).reshape(3, 1, 1, 1)
        for out_dtype in (F32, F16):
            got = launch(t, geom, case.fix_shape, flip=flip, voxels=True, out_dtype=out_dtype, layout="interleaved")
            assert same(got, np.broadcast_to(sign * out_dtype(0.75), (3, 2, 2, 3)).astype(out_dtype)), (flip, out_dtype)
            got = launch(t * 2.0, geom, case.fix_shape, flip=flip, out_dtype=out_dtype)      # the same 3 mm as a physical field
            assert same(got, np.broadcast_to(sign * out_dtype(0.75), (3, 2, 2, 3)).astype(out_dtype)), (flip, out_dtype)


def test_float16_overflows_to_infinity(fields):
    case, n = make_cases()["inner_11x9x7"]
    field = np.array(fields["inner_11x9x7"])
    field[..., 0] = 3.0e5                                          # millimetres: beyond 65504 original voxels after the chain, finite in float32
    field[..., 1] = -3.0e5
    geom = case.geometry()
    want = R.crop_field_half(field, geom, case.fix_shape, 0)
    got32 = launch(field, geom, case.fix_shape, flip=0)
    got16 = launch(field, geom, case.fix_shape, flip=0, out_dtype=F16)
    assert same(got32, want) and np.all(np.isfinite(got32)) and np.all(np.abs(got32[:2]) > 65504.0)
    assert np.all(got16[0] == np.inf) and np.all(got16[1] == -np.inf) and np.all(np.isfinite(got16[2]))
    with np.errstate(over="ignore"):
        assert same(got16, got32.astype(F16))


def test_one_nan_voxel_reaches_exactly_the_outputs_that_interpolate_it(fields):
    case, n = make_cases()["over_7x6x10"]
    clean = fields["over_7x6x10"]
    field = np.array(clean)
    bad = (2, 3, 5)
    field[bad + (1,)] = np.nan                                     # one component of one voxel
    geom = case.geometry()
    full = case.fix_shape
    got = launch(field, geom, full, flip=0)
    assert same(got, R.crop_field_half(field, geom, full, 0))
    # the outputs whose 2 x 2 x 2 sources have that voxel among their taps
    touched = []
    for a in range(3):
        _, _, (i0, i1), _ = R.axis_taps(geom, a, full[a], n[a])
        src = (i0 == bad[a]) | (i1 == bad[a])
        touched.append(np.array([src[2 * o] | src[min(2 * o + 1, full[a] - 1)] for o in range(full[a] // 2)]))
    expect = touched[0][:, None, None] & touched[1][None, :, None] & touched[2][None, None, :]
    assert expect.any() and not expect.all()
    assert np.array_equal(np.isnan(got[1]), expect) and not np.isnan(got[0]).any() and not np.isnan(got[2]).any()
    base = launch(clean, geom, full, flip=0)
    keep = ~np.isnan(got)
    assert same(got[keep], base[keep])                             # nothing else changes


@pytest.mark.parametrize("shape", [(5, 7, 9), (4, 6, 8)])
def test_half_resolution_field_is_aten_scale_factor_half(shape):
    rng = np.random.default_rng(9)
    x = torch.from_numpy((rng.standard_normal((1, 3) + shape) * 20).astype(F32))
    want = F.interpolate(x, scale_factor=0.5, mode="trilinear", align_corners=False)
    got = cropfield.half_resolution_field(x.to(DEV))
    assert got.is_cuda and got.dtype == torch.float32 and same(got.cpu().numpy(), want.numpy())
    got3 = cropfield.half_resolution_field(x[0].to(DEV), out_dtype=torch.float16)
    assert got3.dtype == torch.float16 and same(got3.cpu().numpy(), want[0].numpy().astype(F16))
    from convexadam_amd.convex_adam_utils import resize_trilinear
    by_size = resize_trilinear(x.to(DEV), tuple(s // 2 for s in shape)).cpu().numpy()
    if shape == (5, 7, 9):
        assert not np.array_equal(by_size, want.numpy())           # size= takes the scale in / out, scale_factor= takes exactly 2: why this rule is new
        assert same(by_size, F.interpolate(x, size=(2, 3, 4), mode="trilinear", align_corners=False).numpy())
    else:
        assert same(by_size, want.numpy())                         # even extents: the two rules agree


@pytest.mark.parametrize("tag", TAGS)
def test_python_layer_on_the_golden_inputs(golden, tag, tmp_path):
    """convert_crop_field under the reference criterion; submission_field = convert_crop_field(physical_displacement(.)), bit for bit"""
    case, field, want = golden_case(golden, tag, tmp_path)
    disp_p = torch.from_numpy(field.copy())[None].to(DEV)
    got16 = cropfield.convert_crop_field(case, disp_p)
    got32 = cropfield.convert_crop_field(case, disp_p, out_dtype=torch.float32)
    assert got16.is_cuda and got16.dtype == torch.float16 and tuple(got16.shape) == want.shape
    r = got32.cpu().numpy()
    assert same(r, R.crop_field_half(field, case.geometry(), case.fix_shape, case.flip_mask)) and same(got16.cpu().numpy(), r.astype(F16))
    check_against_reference(r, want, R.reference_bound(field, case.geometry(), case.fix_shape))
    # the fused path from a voxel field
    rng = np.random.default_rng(3)
    u = torch.from_numpy((rng.standard_normal((1, 3) + field.shape[:3]) * 3.0).astype(F32)).to(DEV)
    phys = cropfield.physical_displacement(u, PRE_FIX, PRE_MOV)
    assert tuple(phys.shape) == (1,) + field.shape and phys.dtype == torch.float32
    assert same(phys[0].cpu().numpy(), R.physical(np.moveaxis(u[0].cpu().numpy(), 0, 3), PRE_FIX, PRE_MOV))
    for dt in (torch.float16, torch.float32):
        fused = cropfield.submission_field(u, PRE_FIX, PRE_MOV, case, out_dtype=dt)
        assert same(fused.cpu().numpy(), cropfield.convert_crop_field(case, phys, out_dtype=dt).cpu().numpy())
        assert same(fused.cpu().numpy(), cropfield.submission_field(u[0], PRE_FIX, PRE_MOV, case, out_dtype=dt).cpu().numpy())
