"""The restatement of the preprocessing helpers (tests/prep_restatement.py) against the reference's captured outputs
(tests/golden/prep.npz, written by tests/golden/make_golden_prep.py) and against scipy itself.  CPU only, no kernel runs here.

What is equal and what is close, and why:
  * lo / hi (the two quantiles) are EQUAL: exact order statistics and torch's own lerp.
  * mean / std are within 2 float32 ulps of torch's: the restatement sums in float64 in a fixed order and rounds once, torch sums in
    float32 in an order that depends on how it splits the work.  make_golden_prep.py printed at most 1 ulp for the captured cases
    (mean 0, 1, 0 and std 0, 0, 0 for the CT cases; mean 1, 0 and std 0, 0 for the positive-voxel cases); one more is allowed for
    another split of torch's sum.
  * the elementwise step, fed the reference's captured mean / std / lo / hi, is EQUAL to the captured output bit for bit -- which also
    pins that nnUNetNormProps divides (torch's CPU path; the CUDA path multiplies by a reciprocal for a Python-scalar divisor).
"""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_restatement as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prep.npz")
NAMES = ["nnUNetNorm", "nnUNetNormProps", "nnUNetCTnorm", "compute_steps_for_sliding_window", "get_gaussian", "create_nonzero_mask",
         "get_bbox_from_mask", "crop_to_bbox", "pdist_squared"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


@pytest.mark.parametrize("i", [0, 1, 2])
def test_ct_statistics_against_the_reference(gold, i):
    x, ref = gold["ct%d_in" % i], gold["ct%d_params" % i]
    mine, _ = R.stats(x, clamp_to=(-1000.0, 1500.0), qs=(0.005, 0.995))
    print("ct case %d: mean %d ulp, std %d ulp" % (i, R.ulps(mine[0], ref[0]), R.ulps(mine[1], ref[1])))
    assert mine[2] == ref[2] and mine[3] == ref[3]
    assert R.ulps(mine[0], ref[0]) <= 2 and R.ulps(mine[1], ref[1]) <= 2


@pytest.mark.parametrize("i", [1, 2])
def test_positive_voxel_statistics_against_the_reference(gold, i):
    x, ref = gold["ct%d_in" % i], gold["norm%d_params" % i]
    mine, _ = R.stats(x, positive=True)
    print("norm case %d: mean %d ulp, std %d ulp" % (i, R.ulps(mine[0], ref[0]), R.ulps(mine[1], ref[1])))
    assert R.ulps(mine[0], ref[0]) <= 2 and R.ulps(mine[1], ref[1]) <= 2


@pytest.mark.parametrize("i", [0, 1, 2])
def test_ct_elementwise_step_with_the_reference_numbers_is_bit_equal(gold, i):
    out = R.normalise(gold["ct%d_in" % i], gold["ct%d_params" % i], 0)
    assert np.array_equal(bits(out), bits(gold["ct%d_out" % i]))


@pytest.mark.parametrize("i", [1, 2])
def test_positive_voxel_step_with_the_reference_numbers_is_bit_equal(gold, i):
    mean, std = gold["norm%d_params" % i]
    out = R.normalise(gold["ct%d_in" % i], [mean, std, 0, 0], 1)
    assert np.array_equal(bits(out), bits(gold["norm%d_out" % i]))


@pytest.mark.parametrize("i", [1, 2])
def test_props_step_divides_like_the_cpu_capture(gold, i):
    props = json.loads(str(gold["props"]))
    out = R.nnunet_norm_props(gold["ct%d_in" % i], props)
    assert np.array_equal(bits(out), bits(gold["props%d_out" % i]))


def test_quantiles_equal_torch_on_small_and_tied_inputs():
    g = np.random.default_rng(3)
    for n in (1, 2, 3, 201, 4097):
        for x in (g.normal(size=n).astype(np.float32), np.round(g.normal(size=n) * 2).astype(np.float32)):
            for q in (0.005, 0.5, 0.995, 0.0, 1.0):
                assert bits(R.quantiles(x, [q])[0]) == bits(torch.quantile(torch.from_numpy(x), q).numpy())
    assert np.isnan(R.quantiles(np.array([1, np.nan, 2], np.float32), [0.5])[0])


def test_moments_follow_torch_at_the_edges():
    """n = 0 gives NaN for the mean, n <= 1 NaN for the standard deviation -- as torch"""
    p, (count, _, _) = R.stats(np.array([-1, 0, -3], np.float32), positive=True)
    assert count == 0 and np.isnan(p[0]) and np.isnan(p[1])
    p, (count, _, _) = R.stats(np.array([-1, 5, -3], np.float32), positive=True)
    assert count == 1 and p[0] == 5 and np.isnan(p[1])
    t = torch.tensor([5.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")               # torch warns that one element has no degrees of freedom, and returns NaN
        assert torch.isnan(t.std()) and torch.isnan(t[t > 9].mean())
    assert np.array_equal(R.nnunet_norm(np.array([-1, 0, -3], np.float32)), np.zeros(3, np.float32))
    out = R.nnunet_norm(np.array([-1, 5, -3], np.float32))
    assert np.isnan(out[1]) and out[0] == 0 and out[2] == 0


# ---- hole filling against scipy itself ----------------------------------------------------------------------------------------------
def test_fill_holes_equals_scipy():
    from scipy.ndimage import binary_fill_holes
    g = np.random.default_rng(11)
    shapes = [(1, 1, 1), (1, 5, 7), (2, 2, 2), (3, 3, 3), (7, 9, 11), (5, 4, 131), (20, 21, 22), (6, 7), (12, 13)]
    most = 0
    for shape in shapes:
        for density in (0.3, 0.6, 0.8):
            m = g.random(shape) < density
            got, rounds = R.fill_holes(m)
            most = max(most, rounds)
            assert np.array_equal(got, binary_fill_holes(m)), (shape, density)
    print("most rounds on random masks:", most)
    for sealed, holes in ((False, 0), (True, 49)):
        m = R.serpentine(sealed)
        got, rounds = R.fill_holes(m)
        print("serpentine sealed=%s: %d rounds, %d holes" % (sealed, rounds, int(got.sum() - m.sum())))
        assert np.array_equal(got, binary_fill_holes(m)) and int(got.sum() - m.sum()) == holes
    full = np.ones((3, 4, 5), bool)
    assert np.array_equal(R.fill_holes(full)[0], full) and not R.fill_holes(~full)[0].any()


def test_mask_box_and_crop_equal_the_capture(gold):
    mask, _ = R.nonzero_mask(gold["mask3_in"])
    assert mask.dtype == bool and np.array_equal(mask, gold["mask3_out"])
    assert mask.sum() > (gold["mask3_in"] != 0).any(0).sum()                 # the cavity was filled
    box = R.bbox(mask)
    assert box == gold["bbox3"].tolist() and all(isinstance(v, int) for ax in box for v in ax)
    assert np.array_equal(R.crop(gold["mask3_in"][0], box), gold["crop3"])
    mask2, _ = R.nonzero_mask(gold["mask2_in"])
    assert np.array_equal(mask2, gold["mask2_out"]) and mask2.sum() > (gold["mask2_in"] != 0).any(0).sum()


# ---- host tables --------------------------------------------------------------------------------------------------------------------
def _scipy_gaussian(patch, sigma_scale=1.0 / 8):
    """scipy.ndimage.gaussian_filter itself on a unit impulse at patch // 2 (zeros outside the array), then the restatement's fix-ups"""
    from scipy.ndimage import gaussian_filter
    impulse = np.zeros(patch)
    impulse[tuple(n // 2 for n in patch)] = 1.0
    return R.finish_gaussian(gaussian_filter(impulse, sigma=[n * sigma_scale for n in patch], order=0, mode='constant', cval=0.0))


@pytest.mark.parametrize("patch", [(8, 8, 8), (5, 6, 7), (1, 3, 16), (32, 32, 32), (12, 20)])
def test_gaussian_table_equals_scipy_in_every_half_bit(patch):
    from convexadam_amd.prep import get_gaussian
    want = _scipy_gaussian(patch)
    assert np.array_equal(bits(R.gaussian_table(patch)), bits(want))
    got = get_gaussian(patch, device='cpu')
    assert got.dtype == torch.float16 and tuple(got.shape) == (1, 1) + tuple(patch)
    assert np.array_equal(bits(got.numpy()), bits(want))


def test_gaussian_table_equals_the_capture(gold):
    from convexadam_amd.prep import get_gaussian
    for name in "ab":
        patch = tuple(int(v) for v in gold["gauss_%s_patch" % name])
        assert np.array_equal(bits(get_gaussian(patch, device='cpu').numpy()), bits(gold["gauss_%s" % name]))
    assert int((gold["gauss_a"] == 0).sum()) == 13                             # the half cast underflows the tail of an 8^3 patch


def test_sliding_window_steps_equal_the_capture(gold):
    from convexadam_amd.prep import compute_steps_for_sliding_window
    for patch, size, step, want in json.loads(str(gold["steps"])):
        assert compute_steps_for_sliding_window(patch, size, step) == want == R.steps(patch, size, step)
    assert compute_steps_for_sliding_window((64,), (110,)) == [[0, 23, 46]]    # the example in the reference's comment


def test_host_side_box_crop_and_pdist_equal_the_capture(gold):
    from convexadam_amd.prep import crop_to_bbox, get_bbox_from_mask, pdist_squared
    box = get_bbox_from_mask(gold["mask3_out"])
    assert box == gold["bbox3"].tolist()
    assert np.array_equal(crop_to_bbox(gold["mask3_in"][0], box), gold["crop3"])
    assert torch.equal(crop_to_bbox(torch.from_numpy(gold["mask3_in"][0]), box), torch.from_numpy(gold["crop3"]))
    with pytest.raises(AssertionError, match="only supports 3d"):
        crop_to_bbox(gold["mask3_in"], box)
    with pytest.raises(ValueError):
        get_bbox_from_mask(np.zeros((3, 3, 3), bool))
    assert np.array_equal(bits(pdist_squared(torch.from_numpy(gold["pdist_in"])).numpy()), bits(gold["pdist_out"]))


def test_every_name_is_importable_under_the_reference_modules():
    """fails on the parent commit: none of these names existed"""
    import convexAdam.convex_adam_utils as U
    import convexAdam_hyper_util as Hy
    for n in NAMES:
        assert callable(getattr(U, n)), n
        assert callable(getattr(Hy, n)), n
    from convexAdam.convex_adam_utils import nnUNetCTnorm  # noqa: F401
    import inspect
    assert "device" in inspect.signature(U.get_gaussian).parameters and "device" not in inspect.signature(Hy.get_gaussian).parameters


def test_device_operators_refuse_cpu_tensors():
    from convexadam_amd import prep
    x = torch.zeros(4, 4, 4)
    for fn in (prep.nnUNetNorm, prep.nnUNetCTnorm, lambda t: prep.nnUNetNormProps(t, dict(mean=0, sd=1, percentile_00_5=0, percentile_99_5=1)),
               lambda t: prep.create_nonzero_mask(t[None]), prep.get_bbox_from_mask, prep.normalise_and_crop):
        with pytest.raises(RuntimeError, match="no CPU"):
            fn(x)
    with pytest.raises(AssertionError, match=r"data must have shape \(C, X, Y, Z\) or shape \(C, X, Y\)"):
        prep.create_nonzero_mask(torch.zeros(4, 4))
