"""The restatement of the crop-field contract (tests/cropfield_restatement.py) against the reference's own convert_crop_field, whose
float16 outputs tests/golden/cropfield.npz holds (captured by tests/golden/make_golden_cropfield.py), and against CPU F.interpolate.

Criterion per value: |float(r16) - r| <= 0.5 ulp16(r) + E, r16 the reference's float16, r the restatement's float32 value before its
own cast.  E bounds the reference's float32 chain against the contract's float64 one and is computed from the case's inputs
(reference_bound; derivation in DESIGN.md 27): 7e-5 .. 1.5e-4 mm for `small`, 6e-4 .. 2.5e-3 for `far`.  Observed maximum of
|float(r16) - r| - 0.5 ulp16(r): -6.6e-7 (small), -2.4e-6 (far) -- every golden value is the float16 nearest to the restatement's."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cropfield_restatement as R  # noqa: E402

COLUMNS = ("FixShape", "FixSpacing", "FixCrop", "MovShape", "MovSpacing", "MovCrop")
TAGS = ("small", "far")


def golden_case(golden, tag, tmp_path):
    """(CropCase, field (H, W, D, 3) float32, reference output float16) of one golden case, the case read back through read_cases"""
    from convexadam_amd.cropfield import read_cases
    g = golden("cropfield")
    path = os.path.join(str(tmp_path), "cases_%s.csv" % tag)
    with open(path, "w") as fh:
        fh.write("Id," + ",".join(COLUMNS) + "\n")
        fh.write(tag + "," + ",".join(str(g[tag + "_" + k]) for k in COLUMNS) + "\n")
    return read_cases(path)[tag], g[tag + "_field"][0], g[tag + "_out"]


def check_against_reference(r, r16, E):
    """the criterion; returns the largest |float(r16) - r| - 0.5 ulp16(r) per component"""
    assert r.dtype == np.float32 and r16.dtype == np.float16 and r.shape == r16.shape
    excess = np.abs(r16.astype(np.float64) - r.astype(np.float64)) - 0.5 * R.ulp16(r)
    worst = excess.reshape(3, -1).max(1)
    print("E", E, "max |r16 - r| - 0.5 ulp16(r)", worst, "max |r|", np.abs(r).reshape(3, -1).max(1))
    assert np.all(np.isfinite(r)) and np.all(worst <= E), (worst, E)
    return worst


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_meets_the_reference_within_the_derived_bound(golden, tag, tmp_path):
    case, field, want = golden_case(golden, tag, tmp_path)
    assert want.shape == (3,) + tuple(s // 2 for s in case.fix_shape) and case.flip == "xy" and case.flip_mask == 3
    geom = case.geometry()
    E = R.reference_bound(field, geom, case.fix_shape)
    r = R.crop_field_half(field, geom, case.fix_shape, case.flip_mask)
    assert np.all(E > 0) and np.all(E < 0.25 * R.ulp16(np.abs(r).reshape(3, -1).max(1)))          # the bound says something: far below a float16 step
    check_against_reference(r, want, E)
    if tag == "far":
        assert np.abs(r).max() > 32.0                              # tens of millimetres: float16 steps of 1/32 mm and more


def test_case_constants_follow_the_reference_arithmetic(golden, tmp_path):
    case, field, _ = golden_case(golden, "small", tmp_path)
    k = case.constants()
    assert all(v.dtype == np.float32 for v in k.values())
    assert tuple(k["new_shape"]) == tuple(field.shape[:3]) == (5, 5, 9)
    assert np.array_equal(k["fix_scale"], np.float32([5, 5, 9]) / np.float32([7, 7, 6]))
    assert np.array_equal(k["new_mov_spacing"], np.float32([1.2, 1.2, 2.5]) / (np.float32([5, 5, 9]) / np.float32([8, 9, 6])))
    geom = case.geometry()
    assert geom.dtype == np.float64 and geom.shape == (27,) and np.array_equal(geom[18:24], np.ones(6)) and tuple(geom[24:]) == (9.0, 8.0, 6.0)


@pytest.mark.parametrize("shape", [(2, 3, 4), (5, 7, 2), (4, 4, 4), (3, 5, 7), (7, 2, 5)])
def test_identity_mode_is_aten_scale_factor_half(shape):
    """extents 2, 3, 4, 5, 7 on every axis position; odd ones are where scale_factor=0.5 and size= part"""
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal((3,) + shape) * 50).astype(np.float32)
    want = F.interpolate(torch.from_numpy(x)[None], scale_factor=0.5, mode="trilinear", align_corners=False)[0].numpy()
    got = R.crop_field_half(np.moveaxis(x, 0, 3), None, shape, flip_mask=0, identity=True)
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(R.halve(x).view(np.uint32), want.view(np.uint32))
    half = R.crop_field_half(np.moveaxis(x, 0, 3), None, shape, flip_mask=0, identity=True, out_dtype=np.float16)
    assert half.dtype == np.float16 and np.array_equal(half.view(np.uint16), want.astype(np.float16).view(np.uint16))


def test_scale_factor_and_size_part_on_odd_axes():
    x = torch.arange(5.0).view(1, 1, 1, 1, 5).expand(1, 1, 2, 2, 5).contiguous()
    by_factor = F.interpolate(x, scale_factor=0.5, mode="trilinear", align_corners=False)[0, 0, 0, 0]
    by_size = F.interpolate(x, size=(1, 1, 2), mode="trilinear", align_corners=False)[0, 0, 0, 0]
    assert by_factor.tolist() == [0.5, 2.5] and by_size.tolist() == [0.75, 3.25]
    assert R.halve(x.numpy())[0, 0, 0, 0].tolist() == [0.5, 2.5]


def test_flips_reverse_the_axis_and_negate_its_component():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, 6, 5, 3)).astype(np.float32)
    for mask in range(8):
        want = torch.from_numpy(x.copy())[None]
        for a in range(3):
            if (mask >> a) & 1:
                want = want.flip(1 + a)
                want[..., a] = -want[..., a]
        want = F.interpolate(want.permute(0, 4, 1, 2, 3), scale_factor=0.5, mode="trilinear", align_corners=False)[0].numpy()
        got = R.crop_field_half(x, None, (4, 6, 5), flip_mask=mask, identity=True)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), mask
