"""The preprocessing kernels (csrc/prep.hip) against their numpy restatement (tests/prep_restatement.py), bit for bit (run on the MI355X
box with `-m gpu`).

Every comparison is equality of bits; a NaN equals a NaN (IEEE leaves its sign and payload open, and x86 and gfx950 choose differently).
Sizes: one element, two, below / at / one past a span of 4096 (the unit of the float64 addition order and of a workgroup's histogram),
a row length that is no multiple of anything (5 x 4 x 131), several spans with a ragged tail (33 x 31 x 37), and one volume of
2^24 + 5 elements, where the rank of a quantile is computed in float64."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 2, 201, 4095, 4096, 4097, 5 * 4 * 131, 33 * 31 * 37]
CT = dict(clamp_to=(-1000.0, 1500.0), qs=(0.005, 0.995))


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import prep
    return prep


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize]
        return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def make(kind, n, seed):
    g = np.random.default_rng(seed)
    x = g.normal(40.0, 600.0, n).astype(np.float32)
    if kind == "equal":
        x[:] = 37.5
    elif kind == "background":                      # 70 % below -1000: ONE key after the clamp
        bg = g.random(n) < 0.7
        x[bg] = (-1001.0 - 2000.0 * g.random(int(bg.sum()))).astype(np.float32)
    elif kind == "low10":                           # the keys differ only in their low 10 bits: the last pass decides
        x = (np.uint32(0x3F800000) | g.integers(0, 1024, n).astype(np.uint32)).view(np.float32)
    elif kind == "signs":                           # both signs and both zeros
        x = (g.choice(np.array([-2, -1, -0.0, 0.0, 1, 2], np.float32), n) * g.choice(np.array([1, 1, 0.5, 1e-30], np.float32), n)).astype(np.float32)
        x[::3] = np.float32(-0.0)
        x[1::7] = np.float32(0.0)
    elif kind == "inf":
        x[::5] = np.inf
        x[2::11] = -np.inf
    elif kind == "nan":
        x[n // 2] = np.nan
    return x


def device_stats(P, x, clamp_to=None, positive=False, qs=None):
    from convexadam_amd._prep import CVX_PREP_CLAMP, CVX_PREP_POSITIVE
    t = torch.from_numpy(x).to(DEV)
    flags = (CVX_PREP_CLAMP if clamp_to else 0) | (CVX_PREP_POSITIVE if positive else 0)
    params, mom = P._stats(t, flags, clamp_to or (0.0, 0.0), qs, moments=True)
    assert torch.equal(t.cpu(), torch.from_numpy(x)) or np.isnan(x).any()
    return params.cpu().numpy(), mom.cpu().numpy()


def check_stats(P, x, **kw):
    got_p, got_m = device_stats(P, x, **kw)
    want_p, (count, mean, ss) = R.stats(x, **kw)
    want_m = np.array([count, mean, ss], np.float64)
    assert same_bits(got_m, want_m), ("moments", x.shape, kw, got_m, want_m)
    assert same_bits(got_p, want_p), ("params", x.shape, kw, got_p, want_p)


@pytest.mark.parametrize("kind", ["random", "equal", "background", "low10", "signs", "inf", "nan"])
def test_moments_and_quantiles_equal_the_restatement(P, kind):
    for i, n in enumerate(SIZES):
        x = make(kind, n, 17 * i + 1)
        check_stats(P, x, **CT)                                   # nnUNetCTnorm's statistics
        check_stats(P, x, qs=(0.005, 0.995))                      # unclamped: infinities and tiny values reach the keys
        check_stats(P, x, qs=(0.0, 1.0))                          # minimum and maximum
        check_stats(P, x, positive=True)                          # nnUNetNorm's statistics
        check_stats(P, x)


def test_quantile_ranks_in_float64_above_2_pow_24(P):
    """the one extension: torch.quantile refuses this input; the rank is float64(float32(q)) * (n - 1)"""
    n = (1 << 24) + 5
    x = make("background", n, 5)
    below, above, w = R.rank_of(0.995, n)
    r32 = np.float32(np.float32(0.995) * np.float32(n - 1))                # what the float32 arithmetic would give: a whole number, weight 0
    assert above == below + 1 and 0 < w < 1 and r32 == np.floor(r32) and np.float64(r32) != np.float64(np.float32(0.995)) * (n - 1)
    check_stats(P, x, **CT)


def test_nnunet_ct_norm_equals_the_restatement(P):
    for shape, kind in (((33, 31, 37), "background"), ((5, 4, 131), "random"), ((1, 1, 2, 3, 7), "signs")):
        x = make(kind, int(np.prod(shape)), 9).reshape(shape)
        t = torch.from_numpy(x).to(DEV)
        out = P.nnUNetCTnorm(t)
        assert out.shape == t.shape and out.dtype == torch.float32 and out.data_ptr() != t.data_ptr()
        assert torch.equal(t.cpu(), torch.from_numpy(x)), "the input was modified"
        assert same_bits(out.cpu().numpy(), R.nnunet_ct_norm(x))
    # float64 in -> computed in float32, cast back; a non-contiguous view is taken as it reads
    x = make("background", 24 * 20 * 28, 3).reshape(24, 20, 28)
    out = P.nnUNetCTnorm(torch.from_numpy(x.astype(np.float64)).to(DEV))
    assert out.dtype == torch.float64 and same_bits(out.cpu().numpy(), R.nnunet_ct_norm(x).astype(np.float64))
    tv = torch.from_numpy(x).to(DEV).permute(2, 0, 1)
    assert same_bits(P.nnUNetCTnorm(tv).cpu().numpy(), R.nnunet_ct_norm(np.ascontiguousarray(x.transpose(2, 0, 1))))
    nan = x.copy()
    nan[3, 4, 5] = np.nan
    assert bool(torch.isnan(P.nnUNetCTnorm(torch.from_numpy(nan).to(DEV))).all())       # mean, std and both quantiles are NaN


def test_nnunet_norm_and_props_equal_the_restatement(P):
    props = {'mean': 93.25, 'sd': 217.625, 'percentile_00_5': -958.0, 'percentile_99_5': 1203.5}
    for shape in ((33, 31, 37), (5, 4, 131), (4097,), (3,)):
        x = make("random", int(np.prod(shape)), 21).reshape(shape)
        t = torch.from_numpy(x).to(DEV)
        assert same_bits(P.nnUNetNorm(t).cpu().numpy(), R.nnunet_norm(x))
        assert same_bits(P.nnUNetNormProps(t, props).cpu().numpy(), R.nnunet_norm_props(x, props))
        assert torch.equal(t.cpu(), torch.from_numpy(x)), "the input was modified"
        # an offset view: the pointers are not 16-byte aligned, the scalar kernel runs
        if x.size > 4:
            v = t.reshape(-1)[1:]
            assert v.data_ptr() % 16 and same_bits(P.nnUNetNormProps(v, props).cpu().numpy(), R.nnunet_norm_props(x.reshape(-1)[1:], props))


def test_nnunet_norm_edge_cases(P):
    x = -np.abs(make("random", 4097, 2))
    x[100] = 0.0
    out = P.nnUNetNorm(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert np.array_equal(out, np.zeros_like(x)), "no positive voxel: all zero"
    x[4000] = 7.0
    out = P.nnUNetNorm(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert np.isnan(out[4000]) and not np.delete(out, 4000).any(), "one positive voxel: NaN there (its std is NaN), zero elsewhere"
    assert same_bits(out, R.nnunet_norm(x))


# ---- mask, hole filling, box -------------------------------------------------------------------------------------------------------
def device_mask(P, data):
    """the raw call: mask, box, count, rounds"""
    from convexadam_amd._prep import lib
    L = lib()
    t = torch.from_numpy(np.ascontiguousarray(data, np.float32)).to(DEV)
    shape = data.shape[1:]
    H, W, D = ((1,) + shape) if len(shape) == 2 else shape
    mask = torch.empty(shape, dtype=torch.uint8, device=DEV)
    box = torch.empty(6, dtype=torch.int32, device=DEV)
    count = torch.empty(1, dtype=torch.int64, device=DEV)
    rounds = C.c_int(-1)
    nws = L.cvx_prep_nonzero_mask_workspace_bytes(H, W, D)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)
    rc = L.cvx_prep_nonzero_mask_u8(t.data_ptr(), data.shape[0], H, W, D, len(shape), mask.data_ptr(), box.data_ptr(), count.data_ptr(), C.byref(rounds),
                                    ws.data_ptr(), nws, None)
    assert rc == 0, L.cvx_last_error()
    torch.cuda.synchronize()
    return mask.cpu().numpy().astype(bool), box.cpu().numpy().tolist(), int(count.cpu()[0]), rounds.value


def check_mask(P, data):
    want, want_rounds = R.nonzero_mask(data)
    got, box, count, rounds = device_mask(P, data)
    assert np.array_equal(got, want), data.shape
    assert rounds == want_rounds and count == int(want.sum())
    t = torch.from_numpy(np.ascontiguousarray(data, np.float32)).to(DEV)
    m = P.create_nonzero_mask(t)
    assert m.dtype == torch.bool and m.device.type == "cuda" and np.array_equal(m.cpu().numpy(), want)
    if want.any() and want.ndim == 3:
        wb = R.bbox(want)
        assert box == [v for ax in wb for v in ax]
        got_box = P.get_bbox_from_mask(m)
        assert got_box == wb and all(type(v) is int for ax in got_box for v in ax)
        assert P.get_bbox_from_mask(m.float() * 2 + 1, outside_value=1) == wb        # any dtype, any outside value
        assert np.array_equal(P.crop_to_bbox(t[0], got_box).cpu().numpy(), R.crop(np.asarray(data[0], np.float32), wb))
    elif want.ndim == 3:
        assert box == [2 ** 31 - 1, 0] * 3
        with pytest.raises(ValueError):
            P.get_bbox_from_mask(m)
    return rounds, int(want.sum() - (np.asarray(data) != 0).any(0).sum())


def test_hole_filling_equals_the_restatement(P):
    g = np.random.default_rng(4)
    for shape, density in (((1, 1, 1), 0.5), ((1, 5, 7), 0.6), ((7, 9, 11), 0.6), ((5, 4, 131), 0.6), ((20, 21, 22), 0.8), ((12, 13), 0.7),
                           ((6, 7, 16), 0.6), ((9, 10, 24), 0.75), ((5, 6, 12), 0.6), ((11, 16), 0.7)):       # rows of whole 8- and 4-byte words: the D sweep's word kernels
        for rep in range(2):
            data = (g.random((1,) + shape) < density).astype(np.float32) * g.normal(size=(1,) + shape).astype(np.float32)
            check_mask(P, data)
    solid = np.zeros((1, 9, 9, 9), np.float32)
    solid[0, 2:7, 2:7, 2:7] = 1
    solid[0, 3:6, 3:6, 3:6] = 0
    assert check_mask(P, solid)[1] == 27


def test_hole_filling_serpentine_full_empty_and_channels(P):
    rounds, holes = check_mask(P, R.serpentine(False)[None].astype(np.float32))
    assert holes == 0 and rounds > 3, "the open tunnel takes several rounds and leaves no hole"
    rounds_sealed, holes = check_mask(P, R.serpentine(True)[None].astype(np.float32))
    assert holes == 49
    print("serpentine: %d rounds open, %d sealed" % (rounds, rounds_sealed))
    check_mask(P, np.ones((1, 3, 4, 5), np.float32))
    check_mask(P, np.zeros((1, 3, 4, 5), np.float32))
    # three channels: each holds one pair of opposite walls of a hollow box, only the union encloses the cavity; a NaN is non-zero
    data = np.zeros((3, 7, 8, 9), np.float32)
    data[0, 1, 1:7, 1:8] = data[0, 5, 1:7, 1:8] = 1
    data[1, 1:6, 1, 1:8] = data[1, 1:6, 6, 1:8] = -2
    data[2, 1:6, 1:7, 1] = data[2, 1:6, 1:7, 7] = np.nan
    for c in range(3):
        assert R.nonzero_mask(data[c:c + 1])[0].sum() == (data[c] != 0).sum(), "one channel alone encloses nothing"
    rounds, holes = check_mask(P, data)
    assert holes == 3 * 4 * 5
    # numpy in, numpy bool out
    m = P.create_nonzero_mask(data)
    assert isinstance(m, np.ndarray) and m.dtype == bool and np.array_equal(m, R.nonzero_mask(data)[0])


def test_normalise_and_crop_equals_the_chain_of_restatements(P):
    g = np.random.default_rng(8)
    img = np.zeros((14, 15, 37), np.float32)
    img[3:11, 2:13, 5:30] = make("background", 8 * 11 * 25, 6).reshape(8, 11, 25)
    img[5:8, 5:9, 10:20] = 0                                              # a cavity: the mask fills it, the crop keeps it
    img4 = np.stack([img, np.roll(img, 2, 2) * g.random(img.shape).astype(np.float32)])
    for kind, norm in (("ct", R.nnunet_ct_norm), ("nonzero", R.nnunet_norm)):
        for data in (img, img4):
            out, box = P.normalise_and_crop(torch.from_numpy(data).to(DEV), kind)
            d4 = data if data.ndim == 4 else data[None]
            wb = R.bbox(R.nonzero_mask(d4)[0])
            want = np.stack([norm(np.ascontiguousarray(R.crop(d4[c], wb))) for c in range(d4.shape[0])])
            assert box == wb and box != [[0, 14], [0, 15], [0, 37]]
            assert same_bits(out.cpu().numpy(), want if data.ndim == 4 else want[0])
