"""CPU checks of the crop-field entry point (csrc/cropfield.hip): header and binding declare the symbol, the ABI version is unchanged,
every refusal returns its status code and message before anything is launched, and the Python layer answers bad shapes from tensor
metadata before it asks for a device.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cvx_crop_field_half_f32"
NAN, INF = float("nan"), float("inf")
VOXELS, OUT_F32, IDENTITY = 1, 2, 4
# fix_scale, fix_crop_lo, new_fix_spacing, new_mov_spacing, mov_scale, mov_crop_lo, pre_fix_spacing, pre_mov_spacing, fix_crop_hi:
# a crop of (8, 10, 12) voxels resized to the field's (4, 5, 6)
GEOM = [0.5, 0.5, 0.5, 1.0, 2.0, 3.0, 2.0, 2.0, 2.0, 2.5, 2.5, 2.5, 0.8, 0.8, 0.8, 0.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 9.0, 12.0, 15.0]


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    return _lib.lib()


def doubles(v):
    return (C.c_double * len(v))(*v)


def test_header_and_binding_declare_the_symbol(L):
    from convexadam_amd import _lib
    text = open(os.path.join(ROOT, "include", "convexadam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, src)
    assert decl, "%s is not declared in the header" % NAME
    assert NAME in _lib.SIGNATURES and hasattr(L, NAME)
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(decl.group(1).split(",")) == 14
    assert args[-1] is C.c_void_p                                       # the stream
    for flag, value in (("CVX_CROP_FIELD_VOXELS", VOXELS), ("CVX_CROP_OUT_F32", OUT_F32), ("CVX_CROP_IDENTITY", IDENTITY)):
        assert re.search(r"#define\s+%s\s+%d\b" % (flag, value), src)
    from convexadam_amd import cropfield
    assert (cropfield.CROP_FIELD_VOXELS, cropfield.CROP_OUT_F32, cropfield.CROP_IDENTITY) == (VOXELS, OUT_F32, IDENTITY)
    assert re.search(r"#define\s+CVX_ABI_VERSION\s+2\b", src)
    assert L.cvx_version() == 2 == _lib.ABI_VERSION
    assert "cropfield.hip" in __import__("convexadam_amd.csrc.build", fromlist=["SOURCES"]).SOURCES
    block = text[text.index("csrc/cropfield.hip"):text.index("#define CVX_CROP_FIELD_VOXELS")]
    for stated in ("g_a = fix_scale_a * (x_a - fix_crop_lo_a)", "/ new_mov_spacing_a) / mov_scale_a + mov_crop_lo_a", "d_a = m_a - x_a", "{1 - t, 1 - (1 - t)}"):
        assert stated in block, stated                                  # the arithmetic is written out where the symbol is declared


def test_refusals(L):
    f, o = C.c_void_p(1 << 20), C.c_void_p(2 << 20)
    V = 4 * 5 * 6

    def call(field=f, cs=1, vs=3, fext=(4, 5, 6), geom=GEOM, sext=(11, 14, 17), flip=3, flags=0, out=o):
        return L.cvx_crop_field_half_f32(field, cs, vs, *fext, doubles(geom) if geom is not None else None, *sext, flip, flags, out, None)

    def refused(word, **kw):
        rc = call(**kw)
        msg = L.cvx_last_error()
        assert rc == -1 and word in msg, (kw, rc, msg)

    refused(b"null", field=None)
    refused(b"null", out=None)
    refused(b"null", geom=None)
    refused(b"null", geom=None, flags=VOXELS | OUT_F32)
    for which in ("fext", "sext"):
        for i in range(3):
            for bad in (0, -2):
                ext = [4, 5, 6] if which == "fext" else [11, 14, 17]
                ext[i] = bad
                refused(b"extent", **{which: tuple(ext)})
    for i in range(3):                                                  # an axis of extent 1: empty output
        ext = [11, 14, 17]
        ext[i] = 1
        refused(b"extent", sext=tuple(ext))
        refused(b"extent", sext=tuple(ext), fext=tuple(ext), geom=None, flags=IDENTITY)
    big = (1 << 11, 1 << 10, 1 << 10)                                   # 2^31 voxels: one more than an int holds
    refused(b"2^31", fext=big)
    refused(b"2^31", sext=big)
    refused(b"2^31", sext=(1 << 16, 1 << 16, 2))
    for cs, vs in ((0, 3), (1, 0), (-1, 3), (1, -3), (1, 2), (V - 1, 1), (2, 5), (1 << 41, 1), (1, 1 << 21)):
        refused(b"strides", cs=cs, vs=vs)
    refused(b"overlaps", out=f)
    refused(b"overlaps", out=C.c_void_p((1 << 20) + 3 * V * 4 - 4))                                  # on the field's last element
    refused(b"overlaps", cs=V, vs=1, out=C.c_void_p((1 << 20) + 3 * V * 4 - 4))
    refused(b"overlaps", field=C.c_void_p((2 << 20) + 3 * 5 * 7 * 8 * 2 - 4))                        # on out's last float16
    refused(b"overlaps", field=C.c_void_p((2 << 20) + 3 * 5 * 7 * 8 * 4 - 4), flags=OUT_F32)         # ... its last float32
    refused(b"aligned", out=C.c_void_p((2 << 20) + 1))
    refused(b"aligned", out=C.c_void_p((2 << 20) + 2), flags=OUT_F32)
    refused(b"aligned", field=C.c_void_p((1 << 20) + 2))
    for k in range(27):
        for bad in (NAN, INF, -INF):
            g = list(GEOM)
            g[k] = bad
            refused(b"non-finite", geom=g)
    for k in list(range(0, 3)) + list(range(6, 15)) + list(range(18, 24)):                           # the scales and spacings
        g = list(GEOM)
        g[k] = 0.0
        refused(b"zero", geom=g)
    for flags in (8, 16, -1, 1 << 20, IDENTITY | 8):
        refused(b"unknown flag", flags=flags)
    refused(b"unknown flag", flags=IDENTITY | VOXELS, fext=(11, 14, 17))
    for flip in (-1, 8, 64):
        refused(b"flip", flip=flip)
    # the case's crop does not resize to the field's grid
    refused(b"shape mismatch", fext=(4, 5, 7))
    refused(b"shape mismatch", fext=(5, 5, 6))
    g = list(GEOM)
    g[25] = 13.0                                                        # fix_crop_hi of axis 1: 11 voxels * 0.5 = 5.5 -> 6, not 5
    refused(b"shape mismatch", geom=g)
    refused(b"shape mismatch", flags=IDENTITY, geom=None)               # identity mode: the field's grid is the original one
    refused(b"shape mismatch", flags=IDENTITY, fext=(11, 14, 16))


def test_python_layer_refuses_bad_shapes_before_the_device_check():
    from convexadam_amd import cropfield
    from convexadam_amd.convex_adam_utils import (CropCase, convert_crop_field, half_resolution_field, physical_displacement,  # noqa: F401
                                                  read_cases, submission_field)
    import convexAdam.convex_adam_utils as shim
    for name in ("CropCase", "read_cases", "physical_displacement", "convert_crop_field", "submission_field", "half_resolution_field"):
        assert getattr(shim, name) is getattr(cropfield, name)
    case = CropCase((11, 9, 7), (1.5, 1.5, 3.0), (2, 9, 1, 8, 0, 6), (12, 13, 9), (1.2, 1.2, 2.5), (1, 9, 2, 11, 1, 7))
    assert case.ref_spacing == 2.0 and case.flip == "xy" and case.flip_mask == 3
    Z = torch.zeros
    sp = (1.0, 1.0, 1.0)
    bad = {
        "convert_4d": lambda: convert_crop_field(case, Z(5, 5, 9, 3)),
        "convert_planar": lambda: convert_crop_field(case, Z(1, 3, 5, 5, 9)),
        "convert_batch_2": lambda: convert_crop_field(case, Z(2, 5, 5, 9, 3)),
        "convert_other_grid": lambda: convert_crop_field(case, Z(1, 5, 5, 8, 3)),
        "convert_dtype": lambda: convert_crop_field(case, Z(1, 5, 5, 9, 3), out_dtype=torch.float64),
        "submission_interleaved": lambda: submission_field(Z(1, 5, 5, 9, 3), sp, sp, case),
        "submission_other_grid": lambda: submission_field(Z(1, 3, 6, 5, 9), sp, sp, case),
        "submission_two_spacings": lambda: submission_field(Z(1, 3, 5, 5, 9), (1.0, 1.0), sp, case),
        "submission_zero_spacing": lambda: submission_field(Z(1, 3, 5, 5, 9), sp, (1.0, 0.0, 1.0), case),
        "physical_4d": lambda: physical_displacement(Z(3, 5, 5, 9), sp, sp),
        "physical_nan_spacing": lambda: physical_displacement(Z(1, 3, 5, 5, 9), (NAN, 1.0, 1.0), sp),
        "half_two_components": lambda: half_resolution_field(Z(1, 2, 4, 4, 4)),
        "half_3d": lambda: half_resolution_field(Z(4, 4, 4)),
        "half_extent_1": lambda: half_resolution_field(Z(3, 4, 1, 4)),
        "half_batch_2": lambda: half_resolution_field(Z(2, 3, 4, 4, 4)),
        "half_dtype": lambda: half_resolution_field(Z(3, 4, 4, 4), out_dtype=torch.bfloat16),
        "case_crop_five_numbers": lambda: CropCase((11, 9, 7), sp, (2, 9, 1, 8, 0), (12, 13, 9), sp, (1, 9, 2, 11, 1, 7)),
        "case_empty_crop": lambda: CropCase((11, 9, 7), sp, (2, 2, 1, 8, 0, 6), (12, 13, 9), sp, (1, 9, 2, 11, 1, 7)),
        "case_zero_spacing": lambda: CropCase((11, 9, 7), (1.5, 0.0, 3.0), (2, 9, 1, 8, 0, 6), (12, 13, 9), sp, (1, 9, 2, 11, 1, 7)),
        "case_flip_letter": lambda: CropCase((11, 9, 7), sp, (2, 9, 1, 8, 0, 6), (12, 13, 9), sp, (1, 9, 2, 11, 1, 7), flip="xw"),
        "case_extent_1": lambda: convert_crop_field(CropCase((11, 1, 7), (1.5, 1.5, 3.0), (2, 9, 1, 8, 0, 6), (12, 13, 9), (1.2, 1.2, 2.5),
                                                             (1, 9, 2, 11, 1, 7)), Z(1, 5, 5, 9, 3)),
    }
    for name in sorted(bad):
        with pytest.raises(ValueError):
            bad[name]()
            pytest.fail("%s was accepted" % name)
    with pytest.raises(TypeError):
        convert_crop_field("TCIA01", Z(1, 5, 5, 9, 3))
    # valid shapes on the CPU reach the device check: there is no CPU path
    for ok in (lambda: convert_crop_field(case, Z(1, 5, 5, 9, 3)), lambda: submission_field(Z(1, 3, 5, 5, 9), sp, sp, case),
               lambda: submission_field(Z(3, 5, 5, 9), sp, sp, case), lambda: physical_displacement(Z(1, 3, 5, 5, 9), sp, sp),
               lambda: half_resolution_field(Z(1, 3, 4, 5, 6)), lambda: half_resolution_field(Z(3, 4, 5, 6), out_dtype=torch.float16)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ok()


def test_read_cases_parses_a_row(tmp_path):
    from convexadam_amd.cropfield import CropCase, read_cases
    path = os.path.join(str(tmp_path), "cases.csv")
    with open(path, "w") as fh:
        fh.write("Id,FixShape,FixSpacing,FixCrop,MovShape,MovSpacing,MovCrop\n")
        fh.write("TCIA01,[512 512 149],[0.78 0.78 2.5],[70 440 110 400 3 140],[192 160 192],[2. 2. 2.],[0 192 0 160 0 192]\n")
        fh.write("TCIA03,[11 9 7],[1.5 1.5 3],[2 9 1 8 0 6],[12 13 9],[1.2 1.2 2.5],[1 9 2 11 1 7]\n")
    cases = read_cases(path)
    assert sorted(cases) == ["TCIA01", "TCIA03"] and all(isinstance(c, CropCase) for c in cases.values())
    c = cases["TCIA01"]
    assert c.fix_shape == (512, 512, 149) and c.fix_spacing == (0.78, 0.78, 2.5) and c.fix_crop == (70.0, 440.0, 110.0, 400.0, 3.0, 140.0)
    assert c.mov_shape == (192, 160, 192) and c.mov_spacing == (2.0, 2.0, 2.0) and c.mov_crop == (0.0, 192.0, 0.0, 160.0, 0.0, 192.0)
    assert c.ref_spacing == 2.0 and c.flip == "xy"
    k = c.constants()
    assert tuple(k["fix_crop_lo"]) == (70.0, 110.0, 3.0) and tuple(k["fix_crop_hi"]) == (440.0, 400.0, 140.0)      # view(3, 2): (lo, hi) per axis
    assert tuple(k["new_shape"]) == (144.0, 113.0, 171.0)               # round((370, 290, 137) * (0.39, 0.39, 1.25)) in float32
    assert cases["TCIA03"] == CropCase((11, 9, 7), (1.5, 1.5, 3.0), (2, 9, 1, 8, 0, 6), (12, 13, 9), (1.2, 1.2, 2.5), (1, 9, 2, 11, 1, 7))
    assert read_cases(path, flip="xyz")["TCIA03"].flip_mask == 7
    with open(path, "w") as fh:
        fh.write("Id,FixShape,FixSpacing,FixCrop,MovShape,MovSpacing\nTCIA01,[2 2 2],[1 1 1],[0 2 0 2 0 2],[2 2 2],[1 1 1]\n")
    with pytest.raises(ValueError, match="columns"):
        read_cases(path)
    with open(path, "w") as fh:
        fh.write("Id,FixShape,FixSpacing,FixCrop,MovShape,MovSpacing,MovCrop\nTCIA01,[2 2 2],[1 1 1],[0 2 0 2 0],[2 2 2],[1 1 1],[0 2 0 2 0 2]\n")
    with pytest.raises(ValueError, match="FixCrop"):
        read_cases(path)
