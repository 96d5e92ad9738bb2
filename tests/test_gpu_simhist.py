"""Joint histogram and value range on the device (run on the MI355X box with `-m gpu`): cvx_sim_range_f32 and cvx_joint_hist_f32 against the
numpy restatement of csrc/simhist_core.h, EXACTLY, for the histogram, the five counters and the range.

The matrix: shapes (1,1,1), (2,3,67), (3,5,7), (5,4,130) -- smaller than a wavefront, no multiple of 64 or 256 -- and (24,20,33), 62
workgroups that flush into the same bins; bins (2,2), (32,32), (64,64), (7,130), (128,128) = exactly the LDS limit with one copy, and
(129,128), (256,256) on the global path (LDS copies 4, 4, 2, 4, 1); each with and without a mask, without a field and with one in both
layouts and both element types, those with drop_outside 0 and 1 (the fields of simhist_restatement.field_for land coordinates exactly on
n - 1 and 0 and push others outside).  Then hot bins, planted non-finite values, an all-masked volume, stale outputs, repeatability,
the fused call against warp_device + the unfused one, the Python helpers, and a registration end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simhist_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def S():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import similarity
    return similarity


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def device_case(c):
    return dict(fixed=dev(c["fixed"]), moving=dev(c["moving"]), disp=dev(c["field"]), mask=dev(c["mask"]), drop_outside=c["drop_outside"])


@pytest.mark.parametrize("shape", R.SHAPES, ids=["x".join(map(str, s)) for s in R.SHAPES])
def test_device_equals_the_restatement_on_the_case_matrix(S, shape):
    n = 0
    for with_mask in (False, True):
        for fk in R.FIELDS:
            for drop in ((0, 1) if fk is not None else (0,)):
                c = R.case(shape, None, with_mask, fk, drop, seed=n)
                args = (c["fixed"], c["moving"])
                sampled = R.sample(*args, c["field"], c["mask"], c["drop_outside"])
                want_r, want_rs = R.value_range(*args, sampled=sampled)
                d = device_case(c)
                got_r, got_rs = S.value_range(d["fixed"], d["moving"], disp=d["disp"], mask=d["mask"], drop_outside=drop, return_info=True)
                name = (shape, with_mask, fk, drop)
                assert same_bits(host(got_r), want_r) and same_bits(host(got_rs), want_rs), name
                if fk is not None and min(shape) > 1:
                    assert (want_rs[R.OUTSIDE] > 0) == bool(drop), "the field must push coordinates outside"
                for b in R.BINS:
                    want_h, want_s = R.joint_hist(*args, b, want_r, sampled=sampled)
                    h, info = S.joint_histogram(d["fixed"], d["moving"], b, disp=d["disp"], mask=d["mask"], drop_outside=drop, return_info=True)
                    assert same_bits(host(h), want_h) and same_bits(host(info["stats"]), want_s), (name, b)
                    assert same_bits(host(info["range"]), want_r)
                    n += 1
    assert n == 18 * len(R.BINS)


def test_both_paths_are_taken(S):
    from convexadam_amd import _sim
    q = _sim.lib().cvx_joint_hist_lds_bytes
    assert [q(*b) for b in R.BINS] == [64, 16384, 32768, 14560, 65536, 0, 0]


def test_hot_bins(S):
    from convexadam_amd import phantom
    # an all-equal pair: one bin holds V exactly, on both paths, with a given range and with the pair's own (a constant image: scale 0)
    shape = (24, 20, 33)
    V = int(np.prod(shape))
    a = torch.full(shape, 0.3, device=DEV)
    for bins in ((32, 32), (256, 256)):
        h, info = S.joint_histogram(a, a, bins, value_range=(0.0, 1.0, 0.0, 1.0), return_info=True)
        want_h, want_s = R.joint_hist(host(a), host(a), bins, np.array([0, 1, 0, 1], F))
        assert same_bits(host(h), want_h) and int(h.max()) == V == int(h.sum()) and host(info["stats"]).tolist() == want_s.tolist() == [V, 0, 0, 0, 0]
        h = S.joint_histogram(a, a, bins)
        assert int(h[0, 0]) == V == int(h.sum())
    # a zero background: one cell holds two thirds of the voxels
    fix, mov = phantom.zero_background_pair((48, 48, 48))
    fix, mov = fix.numpy(), R.remap(mov.numpy())
    want_r, _ = R.value_range(fix, mov)
    for bins in ((32, 32), (129, 128)):
        want_h, want_s = R.joint_hist(fix, mov, bins, want_r)
        h, info = S.joint_histogram(dev(fix), dev(mov), bins, return_info=True)
        assert same_bits(host(h), want_h) and same_bits(host(info["stats"]), want_s) and same_bits(host(info["range"]), want_r)
        assert want_h.max() > 0.6 * fix.size


def test_planted_non_finite_values(S):
    c = R.planted_non_finite()
    want_r, want_rs, want_h, want_s = R.expected(c)
    assert want_rs[R.NON_FINITE] >= 9 and int(want_rs[:4].sum()) == c["fixed"].size
    d = device_case(c)
    r, rs = S.value_range(d["fixed"], d["moving"], disp=d["disp"], return_info=True)
    assert same_bits(host(r), want_r) and same_bits(host(rs), want_rs) and np.isfinite(host(r)).all()
    for bins in ((32, 32), (129, 128)):
        want_h, want_s = R.joint_hist(c["fixed"], c["moving"], bins, want_r, c["field"])
        h, info = S.joint_histogram(d["fixed"], d["moving"], bins, disp=d["disp"], return_info=True)
        assert same_bits(host(h), want_h) and same_bits(host(info["stats"]), want_s)
    # without the field: the images' own NaN and Inf only
    want_r, want_rs = R.value_range(c["fixed"], c["moving"])
    r, rs = S.value_range(d["fixed"], d["moving"], return_info=True)
    assert same_bits(host(r), want_r) and same_bits(host(rs), want_rs) and want_rs[R.NON_FINITE] == 7


def test_an_all_masked_volume(S):
    c = R.case((5, 4, 130), None, False, ("planar", "f32"), 1)
    d = device_case(c)
    mask = torch.zeros((5, 4, 130), dtype=torch.uint8, device=DEV)
    r, rs = S.value_range(d["fixed"], d["moving"], disp=d["disp"], mask=mask, drop_outside=True, return_info=True)
    assert host(r).tolist() == [np.inf, -np.inf, np.inf, -np.inf] and host(rs).tolist() == [0, 2600, 0, 0, 0]
    for bins in ((32, 32), (256, 256)):
        h, info = S.joint_histogram(d["fixed"], d["moving"], bins, disp=d["disp"], mask=mask, drop_outside=True, return_info=True)
        assert int(h.abs().sum()) == 0 and host(info["stats"]).tolist() == [0, 2600, 0, 0, 0]
        assert all(bool(torch.isnan(v)) for v in S.entropies(h)) and bool(torch.isnan(S.mutual_information(h)))
    # a boolean mask and a float one are read as non-zero = keep
    m = R.mask_for((5, 4, 130), 3)
    want = host(S.joint_histogram(d["fixed"], d["moving"], 32, mask=dev(m)))
    for other in (dev(m) != 0, dev(m).to(torch.float32)):
        assert same_bits(host(S.joint_histogram(d["fixed"], d["moving"], 32, mask=other)), want)


def test_stale_outputs_are_reset_and_two_runs_give_identical_bytes(S):
    from convexadam_amd import _sim
    L = _sim.lib()
    c = R.case((24, 20, 33), None, True, ("interleaved", "f32"), 1, seed=9)
    want_r, want_rs, _, _ = R.expected(dict(c, bins=(2, 2)))
    d = device_case(c)
    V = c["fixed"].size
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    field = (p(d["disp"]), 0, 1, 3)
    for bins in ((32, 32), (129, 128)):
        want_h, want_s = R.joint_hist(c["fixed"], c["moving"], bins, want_r, c["field"], c["mask"], True)
        runs = []
        for fill in (0x7F, 0xA5, 0x00):
            rng = torch.empty(4, dtype=torch.float32, device=DEV)
            rs, hs = torch.empty(5, dtype=torch.int64, device=DEV), torch.empty(5, dtype=torch.int64, device=DEV)
            h = torch.empty(bins, dtype=torch.int64, device=DEV)
            for t in (rng, rs, hs, h):
                t.view(torch.uint8).fill_(fill)
            assert L.cvx_sim_range_f32(p(d["fixed"]), p(d["moving"]), *field, p(d["mask"]), 24, 20, 33, 1, p(rng), p(rs), stream) == 0
            assert L.cvx_joint_hist_f32(p(d["fixed"]), p(d["moving"]), *field, p(d["mask"]), 24, 20, 33, bins[0], bins[1], p(rng), 1, p(h), p(hs), stream) == 0
            runs.append((host(rng), host(rs), host(h), host(hs)))
        for got in runs:
            assert same_bits(got[0], want_r) and same_bits(got[1], want_rs) and same_bits(got[2], want_h) and same_bits(got[3], want_s)
        assert int(want_s[:4].sum()) == V


def test_the_fused_call_equals_warp_device_and_the_unfused_call(S):
    from convexadam_amd.ssim import warp_device
    for shape, seed in (((5, 4, 130), 1), ((24, 20, 33), 2)):
        for fk in R.FIELDS[1:]:
            c = R.case(shape, None, True, fk, 0, seed=seed)
            d = device_case(c)
            warped = warp_device(d["moving"], d["disp"])
            for bins in ((32, 32), (129, 128)):
                r_f, s_f = S.value_range(d["fixed"], d["moving"], disp=d["disp"], mask=d["mask"], return_info=True)
                r_u, s_u = S.value_range(d["fixed"], warped, mask=d["mask"], return_info=True)
                assert torch.equal(r_f.view(torch.int32), r_u.view(torch.int32)) and torch.equal(s_f, s_u)
                h_f, i_f = S.joint_histogram(d["fixed"], d["moving"], bins, disp=d["disp"], mask=d["mask"], return_info=True)
                h_u, i_u = S.joint_histogram(d["fixed"], warped, bins, mask=d["mask"], return_info=True)
                assert torch.equal(h_f, h_u) and torch.equal(i_f["stats"], i_u["stats"]) and int(h_f.sum()) > 0


def test_python_helpers_and_registration_mi(S):
    c = R.case((24, 20, 33), None, False, ("planar", "f32"), 0, seed=4)
    d = device_case(c)
    h = S.joint_histogram(d["fixed"], d["moving"], (32, 16))
    assert tuple(h.shape) == (32, 16) and h.dtype == torch.int64 and h.is_cuda
    ents = S.entropies(h)
    want = R.entropies(host(h))
    for g, w, counts in zip(ents, want, (host(h).sum(1), host(h).sum(0), host(h))):
        assert g.is_cuda and g.dtype == torch.float64 and abs(float(g) - w) <= R.entropy_bound(counts)
    tol = sum(R.entropy_bound(x) for x in (host(h).sum(1), host(h).sum(0), host(h)))
    assert abs(float(S.mutual_information(h)) - R.mutual_information(host(h))) <= tol
    assert abs(float(S.mutual_information(d["fixed"], d["moving"], bins=(32, 16))) - R.mutual_information(host(h))) <= tol
    assert abs(float(S.normalized_mutual_information(h)) - R.normalized_mutual_information(host(h))) <= 4 * tol / want[2]
    # registration_mi: one range, that of the unwarped pair; drop_outside by default; equal to the pieces
    res = S.registration_mi(d["fixed"], d["moving"], d["disp"], bins=32)
    rng = S.value_range(d["fixed"], d["moving"])
    before = S.joint_histogram(d["fixed"], d["moving"], 32, value_range=rng)
    after, info = S.joint_histogram(d["fixed"], d["moving"], 32, disp=d["disp"], value_range=rng, drop_outside=True, return_info=True)
    assert int(info["stats"][R.OUTSIDE]) > 0 and int(info["stats"][R.CLAMPED]) >= 0
    want_after, want_s = R.joint_hist(c["fixed"], c["moving"], 32, host(rng), c["field"], None, True)
    assert same_bits(host(after), want_after) and same_bits(host(info["stats"]), want_s)
    assert float(res.mi_before) == float(S.mutual_information(before)) and float(res.mi_after) == float(S.mutual_information(after))
    assert float(res.nmi_before) == float(S.normalized_mutual_information(before))
    assert float(res.nmi_after) == float(S.normalized_mutual_information(after))
    assert all(v.is_cuda and v.dim() == 0 for v in res)
    # identical images: NMI = 2; a given range as four numbers
    same = S.joint_histogram(d["fixed"], d["fixed"], 32, value_range=(-3.0, 3.0, -3.0, 3.0))
    hs = host(same)
    tol_same = sum(R.entropy_bound(x) for x in (hs.sum(1), hs.sum(0), hs))
    assert abs(float(S.normalized_mutual_information(same)) - 2.0) <= 4 * tol_same / R.entropies(hs)[2] and int(same.sum()) == c["fixed"].size
    with pytest.raises(ValueError):
        S.joint_histogram(d["fixed"], d["moving"][:-1], 32)
    with pytest.raises(ValueError):
        S.joint_histogram(d["fixed"], d["moving"], 32, value_range=(0.0, 1.0))
    from convexadam_amd._lib import CvxError
    with pytest.raises(CvxError, match="bins"):
        S.joint_histogram(d["fixed"], d["moving"], 257)


def test_registration_raises_the_mutual_information_of_a_remapped_pair(S):
    """deformed_pair((48, 48, 48)), registered on the unremapped images with the convex_confidence test's settings (grid_sp 4, disp_hw 2);
    the criterion looks at the moving image through exp(-1.3 x) + 0.1 x^2, where SSIM has nothing to say."""
    from convexadam_amd import phantom
    from convexadam_amd.convex_adam_MIND import register_pair_device
    shape = (48, 48, 48)
    fix, mov = phantom.deformed_pair(shape)
    a, b = fix.to(DEV), mov.to(DEV)
    disp = register_pair_device(a, b, grid_sp=4, disp_hw=2)
    assert tuple(disp.shape) == (3,) + shape
    remapped = dev(R.remap(mov.numpy()))
    res = S.registration_mi(a, remapped, disp, bins=32)
    aligned = dev(R.remap(phantom.phantom(shape, 1, 110).numpy()))
    ceiling = S.mutual_information(a, aligned, bins=32)
    print("remapped 48^3 pair: MI before %.4f after %.4f (NMI %.4f -> %.4f); aligned ceiling %.4f"
          % (float(res.mi_before), float(res.mi_after), float(res.nmi_before), float(res.nmi_after), float(ceiling)))
    assert float(res.mi_after) > float(res.mi_before)
