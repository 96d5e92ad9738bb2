"""The inputs of tests/certified_cases.py on the CPU: each case is inside the input contract and does what its name claims, the oracle
equals the reference's own captures on all of them (tests/golden/certified.npz, made by tests/golden/make_golden_certified.py), and the
constants that tests/test_gpu_certified_range.py restates are the ones certify.hip is compiled with.  Never part of the `-m gpu` selection."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import certified_cases as CC  # noqa: E402
from make_golden_live import digest  # noqa: E402

CERTIFY_HIP = os.path.join(os.path.dirname(HERE), "convexadam_amd", "csrc", "certify.hip")
FLAG = CC.FLAG
DENORMAL = 2.0 ** -126


def certify_constants(path=CERTIFY_HIP):
    """(eps, boxes, tiny, flag) as certify.hip's text states them: CLO / CHI = (1 -/+ eps) / boxes, CERT_TINY, the flag of the plain stream"""
    src = open(path).read()
    num = r"([0-9.eE+-]+)"
    lo = re.search(r"#define\s+CERT_CLO\s+\(\(float\)\(\(1\.0 - 1\.0 / %s\) / %s\)\)" % (num, num), src)
    hi = re.search(r"#define\s+CERT_CHI\s+\(\(float\)\(\(1\.0 \+ 1\.0 / %s\) / %s\)\)" % (num, num), src)
    tiny = re.search(r"#define\s+CERT_TINY\s+%sf" % num, src)
    flags = set(re.findall(r"\(c(?:4\[j\])? > 0\.0f\) & \(c(?:4\[j\])? < %sf\)" % num, src))
    assert lo and hi and tiny and len(flags) == 1, "certify.hip no longer states its constants in the form this test reads"
    assert lo.groups() == hi.groups()
    return 1.0 / float(lo.group(1)), float(lo.group(2)), float(tiny.group(1)), float(flags.pop())


@pytest.fixture(scope="module")
def ref(golden):
    return golden("certified")


@pytest.fixture(scope="module")
def volumes(orc):
    """name -> (ssd, argmin) of the oracle, computed once"""
    return {name: orc.correlate(f, m, hw) for name, C, shape, hw, f, m in CC.CASES}


def columns(ssd):
    return ssd.reshape(ssd.shape[0], -1).astype(np.float64)


def test_the_list_is_the_matrix_of_the_issue():
    names = set(CC.NAMES)
    assert 120 <= len(CC.CASES) <= 170 and 12 <= len(CC.PAIRS) <= 16
    for C, shape, hw in CC.SHAPES:
        for e in CC.SCALES:
            assert "textured@e%d/C%d" % (e, C) in names
        assert ("textured@e57/C%d" % C in names) == CC.scale_allowed(C, 57)
    assert any(n.startswith("textured@e57/") for n in names)
    for kind in CC.KINDS[1:]:
        for e in CC.SCALES_SHORT:
            assert any(n.startswith("%s@e%d/" % (kind, e)) for n in names), (kind, e)
    for head in ("textured@x1000", "textured@x3e-19", "signed", "signed@e-66", "signed@e55", "mixed_channels_textured", "nan_one_in_m", "nan_voxel_in_f",
                 "nan_scattered", "nan_first_voxel", "nan_last_voxel", "nan_zero_background"):
        assert any(n.startswith(head + "/") for n in names), head
    for which in "fm":
        for place in ("corner", "face", "edge", "inside_face", "interior"):
            assert "outlier_%s_%s/C12" % (which, place) in names and "outlier_%s_%s/C16" % (which, place) in names
    assert "nan_cascade/C16" in names and "nan_cascade/C33" in names
    assert {"mirror/C12", "mirror/C16", "mirror_perm_s10/C12", "mirror_perm_s11/C12"} <= names
    pairs = set(CC.PAIR_NAMES)
    assert {"pair_textured@e%d" % e for e in CC.PAIR_SCALES} <= pairs and "pair_signed@e0" in pairs
    assert {"pair_zero_background@e-8", "pair_zero_background@e8"} <= pairs and sum(n.startswith("pair_nan") for n in pairs) == 2
    for name, C, shape, hw, f, m in CC.CASES:
        assert (C, shape, hw) in CC.SHAPES and f.shape == m.shape == (C,) + shape and f.dtype == m.dtype == np.float32, name
    for name, f, m in CC.PAIRS:
        assert f.shape == m.shape == (CC.PAIR_SHAPE[0],) + CC.PAIR_SHAPE[1] and f.dtype == m.dtype == np.float32, name


def test_every_case_is_inside_the_contract():
    for name, C, shape, hw, f, m in CC.CASES:
        assert CC.inside_contract(C, f, m), name
    for name, f, m in CC.PAIRS:
        assert CC.inside_contract(CC.PAIR_SHAPE[0], f, m), name
    # the check itself: one step beyond the bound, and an infinity, are outside
    C, shape, hw = CC.SHAPES[0]
    f, m = CC.base("textured", C, shape)
    assert not CC.inside_contract(C, *CC.scaled((f, m), 2.0 ** 58))
    f[0, 0, 0, 0] = np.inf
    assert not CC.inside_contract(C, f, m)


def test_scaled_inputs_are_exact_multiples():
    for name, C, shape, hw, f, m in CC.CASES:
        e = CC.scale_exponent(name)
        if e:
            f0, m0 = CC.case(CC.unscaled_name(name))[4:]
            assert np.array_equal(f.astype(np.float64), f0.astype(np.float64) * 2.0 ** e) and np.array_equal(m.astype(np.float64), m0.astype(np.float64) * 2.0 ** e), name


def test_power_of_two_scales_leave_the_normal_range_alone(volumes):
    """ssd == 4^e ssd_0 exactly and the same argmin wherever the scaled volume stays at or above 2^-100"""
    checked = 0
    for name in CC.NAMES:
        e = CC.scale_exponent(name)
        if not e:
            continue
        ssd, am = volumes[name]
        if not float(ssd.min()) >= 2.0 ** -100:
            continue
        ssd0, am0 = volumes[CC.unscaled_name(name)]
        assert np.array_equal(ssd.astype(np.float64), ssd0.astype(np.float64) * 4.0 ** e), name
        assert np.array_equal(am, am0), name
        checked += 1
    assert checked >= 20, checked


def test_the_named_edges_are_in_the_list(volumes):
    # a column with 729 ssd entries on both sides of the flag
    u = 729.0 * columns(volumes["textured@e-64/C12"][0])
    assert int((((u > 0) & (u < FLAG)).any(0) & (u >= FLAG).any(0)).sum()) >= 100
    # ssd entirely denormal while 729 ssd is above the flag in some columns: only TINY keeps the interval sound there
    for name in ("textured@e-64/C4", "signed@e-66/C12"):
        s = columns(volumes[name][0])
        assert float(s.max()) < DENORMAL and int((729.0 * s > FLAG).any(0).sum()) >= 100, name
    # ATen's denormal roundings move the argmin
    for name in ("textured@e-70/C12", "textured@e-72/C4", "textured@e-74/C16", "textured@e-72/C33"):
        assert int((volumes[name][1] != volumes[CC.unscaled_name(name)][1]).sum()) >= 1, name
    # exact zeros next to positive entries in one column, in the denormal band: zeros of the input and zeros the roundings made
    for name in ("zero_background@e-66/C16", "textured@e-74/C12"):
        s = columns(volumes[name][0])
        assert float(s.max()) < DENORMAL and int(((s == 0).any(0) & (s > 0).any(0)).sum()) >= 100, name
    assert float(columns(volumes["textured@e-70/C12"][0]).min()) > 0          # (the roundings reach zero only below this scale here)
    # columns whose two smallest entries differ by their roundings only, and are not one sum twice
    for name in ("mirror/C12", "mirror/C16", "mirror_perm_s10/C12", "mirror_perm_s11/C12"):
        two = np.sort(columns(volumes[name][0]), 0)[:2]
        gap = (two[1] - two[0]) / two[0]
        assert int(((gap > 0) & (gap < 1e-6)).sum()) >= 40, name
    # NaN cases hold NaN columns and NaN-free columns, and NaNs next to exact zeros
    for name in CC.NAMES:
        if name.startswith("nan_"):
            nan_cols = np.isnan(columns(volumes[name][0])).any(0)
            assert nan_cols.any() and not nan_cols.all(), name
    s = columns(volumes["nan_zero_background/C12"][0])
    assert int((np.isnan(s).any(0) & (s == 0).any(0)).sum()) >= 10
    # negative features, channels of different magnitude, one dominating voxel
    assert float(CC.case("signed/C12")[4].min()) < -0.9 and float(CC.case("signed@e55/C33")[5].min()) < -0.9 * 2.0 ** 55
    f = CC.case("mixed_channels_textured/C12")[4]
    assert float(np.abs(f[11]).max()) >= 2.0 ** 50 * float(np.abs(f[0]).max())
    for n in CC.NAMES:
        if n.startswith("outlier_"):
            f, m = CC.case(n)[4:]
            t = np.sort((f if n.startswith("outlier_f") else m).reshape(-1))
            assert t[-1] >= 2.0 ** 19 and t[-2] < 1.1, n


def test_pair_scales_span_the_penalty_and_the_data_regime(orc):
    """the interval width grows with ssd while the penalties stay O(1): the scales must give different fields"""
    fields = [orc.convex_adam_pipeline(None, None, features=CC.pair("pair_textured@e%d" % e)[1:], **CC.PAIR_KW) for e in CC.PAIR_SCALES]
    assert all(np.isfinite(x).all() for x in fields)
    assert len({digest(x) for x in fields}) >= 5
    for name in CC.PAIR_NAMES:
        if name.startswith("pair_nan"):
            assert np.isfinite(orc.convex_adam_pipeline(None, None, features=CC.pair(name)[1:], **CC.PAIR_KW)).all(), name


def test_oracle_equals_the_reference_on_every_case(ref, volumes):
    assert {k.split(":")[0] for k in ref} == set(CC.NAMES) | set(CC.PAIR_NAMES), "tests/golden/certified.npz was made for another list: run make_golden_certified.py"
    for name in CC.NAMES:
        ssd, am = volumes[name]
        assert ref[name + ":argmin"].dtype == np.int16 and np.array_equal(ref[name + ":argmin"], am), name
        assert digest(ssd) == str(ref[name + ":ssd_digest"]), name


def test_oracle_equals_the_reference_on_every_pair(ref, orc):
    g, hw = CC.PAIR_KW["grid_sp"], CC.PAIR_KW["disp_hw"]
    mesh = orc.disp_mesh(hw)
    for name, f, m in CC.PAIRS:
        fs, ms = orc.avgpool_stride(f, g), orc.avgpool_stride(m, g)
        for tag, a, b in (("fwd", fs, ms), ("bwd", ms, fs)):
            ssd, am = orc.correlate(a, b, hw)
            assert np.array_equal(ref["%s:%s_argmin" % (name, tag)], am) and digest(ssd) == str(ref["%s:%s_ssd_digest" % (name, tag)]), (name, tag)
            soft = orc.coupled_convex(ssd, am, mesh, hw)
            if tag == "fwd":
                assert np.array_equal(ref[name + ":fwd_soft"], soft, equal_nan=True), name
            else:
                assert digest(soft) == str(ref[name + ":bwd_soft_digest"]), name


def test_constants_of_certify_hip():
    eps, boxes, tiny, flag = certify_constants()
    assert (eps, boxes, tiny, flag) == (2.0 ** -16, 729.0, 1.0e-40, FLAG)
    assert (CC.EPS, CC.BOXES, float(CC.TINY), CC.FLAG) == (eps, boxes, float(np.float32(tiny)), flag)
