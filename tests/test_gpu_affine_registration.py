"""convex_adam_affine and register_with_affine on the GPU (convexadam_amd/affine.py): the calls equal their parts bit for bit, and a known
affine motion with scale and shear -- which no rigid fit can absorb -- is recovered better than the identity and better than the rigid fit
on the same samples.

The phantom is 48 x 44 x 40 with grid_sp 4 and disp_hw 3.  The moving image is the fixed one pulled through F.affine_grid(A); A carries the
per-axis scale (1.06, 0.95, 1), a small shear and a translation of ONE WHOLE coarse cell (4 voxels) along every axis.  The figure is
||T A - I||_F on the 4 x 4 matrices in normalised coordinates: T approximates inverse(A).

Why the translation, and why one cell.  The convex stage searches whole cells (convex_adam_rigid's docstring).  The scale alone moves
nothing by more than 1.4 voxels in this phantom, under half a cell, so without a translation the stage returns the all-zero field and every
model the identity (measured: identity, rigid and affine all 0.0883).  A whole-cell translation is the one the stage represents exactly,
so the figure is not led by a half-cell translation error that both models share, and the scale shows as cells near the object's ends
whose winner changes.  The scale's signal stays below the stage's step, so ONE round cannot be expected to beat the rigid fit at every
translation: a least-squares slope through a displacement that is a step function of the position over- or undershoots the true slope
by as much as the slope itself.  Measured on the MI355X with the two moving modalities of this file (identity / rigid / affine / rounds 2):
    one cell (this file)           0.3296 / 0.0960 / 0.0868 / 0.0868
    one and a half cells           0.4886 / 0.1664 / 0.1937 / 0.1437     the step sits at the object's centre: the slope doubles
    two cells                      0.6412 / 0.2173 / 0.2438 / 0.2384
rounds = 2 is the remedy the function offers; the assertions below are made on the representable translation."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPE, G, HW = (48, 44, 40), 4, 3
A_TRUE = torch.tensor([[1.06, 0.03, 0.00, 2.0 * G / SHAPE[2]], [0.00, 0.95, 0.02, -2.0 * G / SHAPE[1]], [0.02, 0.00, 1.00, 2.0 * G / SHAPE[0]]], dtype=torch.float32)
PT_KW = dict(grid_sp=4, disp_hw=2, selected_niter=12, grid_sp_adam=2, dtype=torch.float32)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def figure(T):
    A4 = torch.eye(4, dtype=torch.float64)
    A4[:3] = A_TRUE.double()
    return float(torch.linalg.norm(T.double().cpu() @ A4 - torch.eye(4, dtype=torch.float64)))


@pytest.fixture(scope="module")
def case():
    """fixed, moving, a second modality of the moving image: device tensors, made once and never changed"""
    from convexadam_amd.phantom import ellipsoid_mask, zero_background_pair
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    fix, _ = zero_background_pair(SHAPE)
    fixed = ((40.0 * fix + 100.0) * ellipsoid_mask(SHAPE, 0.42)).contiguous()
    grid = F.affine_grid(A_TRUE[None], (1, 1) + SHAPE, align_corners=False)
    moving = F.grid_sample(fixed[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0, 0].contiguous()
    moving2 = torch.where(moving > 0, 300.0 - 0.004 * (moving - 100.0) ** 2 - moving, torch.zeros(())).clamp_min(0.0).contiguous()
    return fixed.to(DEV), moving.to(DEV), moving2.to(DEV)


@pytest.fixture(scope="module")
def parts(case):
    """mask, stage, samples of the case, from the single calls"""
    from convexadam_amd.convex_adam_utils import mind_pooled
    from convexadam_amd.rigid import convex_stage, rigid_samples, threshold_pool_mask
    fixed, moving, moving2 = case
    ff = mind_pooled(fixed[None, None], 3, 3, G)
    ff = torch.cat([ff, ff], 1)
    fm = torch.cat([mind_pooled(m[None, None], 3, 3, G) for m in (moving, moving2)], 1)
    mf, mm = threshold_pool_mask(fixed, 10.0, G), threshold_pool_mask(moving, 10.0, G)
    coarse, hr = convex_stage(ff, fm, G, HW, SHAPE, mf, mm, 5)
    T1, T2 = rigid_samples(coarse, mf, G, SHAPE)
    return mf, mm, hr, T1, T2


def test_convex_adam_affine_is_its_parts(case, parts):
    from convexadam_amd.affine import AffineRegistration, affine_from_field, convex_adam_affine, least_trimmed_affine
    fixed, moving, moving2 = case
    mf, mm, hr, T1, T2 = parts
    res = convex_adam_affine(fixed, [moving, moving2], grid_sp=G, disp_hw=HW)
    assert isinstance(res, AffineRegistration) and res.disp_hr is None and res.tre_affine is None and not hasattr(res, "tre_rigid")
    assert tuple(res.T.shape) == (4, 4) and res.T.dtype == torch.float32 and res.T.is_cuda
    assert torch.equal(res.mask_fix, mf) and torch.equal(res.mask_mov, mm) and float(mf.float().mean()) > 0.1
    assert bits_equal(res.T, least_trimmed_affine(T1, T2, 15))
    assert bits_equal(res.T[3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]))
    with_field = convex_adam_affine(fixed, [moving, moving2], grid_sp=G, disp_hw=HW, return_field=True, lts_iters=4)
    assert bits_equal(with_field.disp_hr, hr) and bits_equal(with_field.T, least_trimmed_affine(T1, T2, 4))
    assert bits_equal(affine_from_field(hr, mf, G, 4), with_field.T)                 # the rows of the up-sampled field are the same rows
    with pytest.raises(ValueError, match="mask_thresh"):
        convex_adam_affine(fixed, moving, grid_sp=G, disp_hw=HW, mask_thresh=1e9)
    with pytest.raises(ValueError, match="rounds"):
        convex_adam_affine(fixed, moving, grid_sp=G, disp_hw=HW, rounds=0)
    with pytest.raises(RuntimeError):
        convex_adam_affine(fixed.cpu(), moving.cpu(), grid_sp=G, disp_hw=HW)


def test_known_scale_and_shear_are_recovered_better_than_by_the_rigid_fit(case, parts):
    from convexadam_amd.affine import convex_adam_affine
    from convexadam_amd.rigid import least_trimmed_rigid
    fixed, moving, moving2 = case
    _, _, _, T1, T2 = parts
    one = convex_adam_affine(fixed, [moving, moving2], grid_sp=G, disp_hw=HW).T
    two = convex_adam_affine(fixed, [moving, moving2], grid_sp=G, disp_hw=HW, rounds=2).T
    rigid = least_trimmed_rigid(T1, T2, 15)
    f_id, f_rigid, f_one, f_two = figure(torch.eye(4)), figure(rigid), figure(one), figure(two)
    print("||T A - I||_F: identity %.4f, rigid fit %.4f, affine fit %.4f, two rounds %.4f" % (f_id, f_rigid, f_one, f_two))
    assert f_one < f_id
    assert f_one < f_rigid
    assert f_two <= f_one
    assert bits_equal(two[3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]))


def test_tre_fields_have_the_rigid_calls_dtype_and_length(case):
    from convexadam_amd.affine import convex_adam_affine
    from convexadam_amd.rigid import affine_warp, convex_adam_rigid, landmark_tre
    fixed, moving, _ = case
    seg = torch.zeros(SHAPE)
    rng = np.random.default_rng(2)
    for l in range(1, 7):
        c = [int(rng.integers(s // 3, 2 * s // 3)) for s in SHAPE]
        seg[c[0] - 2:c[0] + 3, c[1] - 2:c[1] + 3, c[2] - 2:c[2] + 3] = l
    seg_m = F.grid_sample(seg[None, None], F.affine_grid(A_TRUE[None], (1, 1) + SHAPE, align_corners=False), mode="nearest", align_corners=False)[0, 0]
    a = convex_adam_affine(fixed, moving, grid_sp=G, disp_hw=HW, seg_fixed=seg.to(DEV), seg_moving=seg_m.to(DEV))
    r = convex_adam_rigid(fixed, moving, grid_sp=G, disp_hw=HW, seg_fixed=seg.to(DEV), seg_moving=seg_m.to(DEV))
    assert a.disp_hr is not None and bits_equal(a.disp_hr, r.disp_hr)
    for mine, theirs in ((a.tre_before, r.tre_before), (a.tre_deformable, r.tre_deformable), (a.tre_affine, r.tre_rigid)):
        assert mine.dtype == theirs.dtype == torch.float64 and tuple(mine.shape) == tuple(theirs.shape) == (int(seg_m.max()),) and not mine.is_cuda
    assert torch.equal(torch.nan_to_num(a.tre_before), torch.nan_to_num(r.tre_before))
    assert torch.equal(torch.nan_to_num(a.tre_deformable), torch.nan_to_num(r.tre_deformable))
    assert torch.equal(torch.nan_to_num(a.tre_affine),
                       torch.nan_to_num(landmark_tre(seg.to(DEV), affine_warp(seg_m.to(DEV)[None], a.T, mode="nearest")[0], int(seg_m.max()))))
    print("landmark TRE (mean): before %.2f, deformable %.2f, rigid %.2f, affine %.2f voxels"
          % tuple(float(np.nanmean(t.numpy())) for t in (a.tre_before, a.tre_deformable, r.tre_rigid, a.tre_affine)))


def test_register_with_affine_is_its_parts(case):
    from convexadam_amd.affine import affine_to_field, convex_adam_affine, register_with_affine
    from convexadam_amd.apply_convex import apply_convex
    from convexadam_amd.convex_adam_MIND import convex_adam_pt
    from convexadam_amd.rigid import affine_warp
    fixed, moving, _ = case
    ak = dict(grid_sp=G, disp_hw=HW, lts_iters=5)
    field, T = register_with_affine(fixed, moving, affine_kwargs=ak, **PT_KW)
    assert field.is_cuda and field.dtype == torch.float64 and tuple(field.shape) == SHAPE + (3,)
    res = convex_adam_affine(fixed, moving, **ak)
    assert bits_equal(T, res.T)
    deformable = convex_adam_pt(fixed, affine_warp(moving[None], res.T)[0], device=fixed.device, **PT_KW)
    assert isinstance(deformable, np.ndarray) and deformable.shape == SHAPE + (3,)
    assert bits_equal(field, affine_to_field(res.T, SHAPE, field=deformable))
    assert np.array_equal(field.cpu().numpy(), R.field(res.T.cpu().numpy(), SHAPE, deformable))
    # ONE pull-back field that apply_convex takes as it is: closer to the fixed image than the moving image was
    warped = apply_convex(field, moving)
    inside = fixed.cpu().numpy() > 0
    before = float(np.abs(moving.cpu().numpy() - fixed.cpu().numpy())[inside].mean())
    after = float(np.abs(warped - fixed.cpu().numpy())[inside].mean())
    print("mean |moving - fixed| inside the object: %.2f before, %.2f after register_with_affine" % (before, after))
    assert after < before


def test_register_with_affine_with_the_identity_returns_the_deformable_field(case, monkeypatch):
    from convexadam_amd import affine
    from convexadam_amd.convex_adam_MIND import convex_adam_pt
    from convexadam_amd.rigid import affine_warp
    fixed, moving, _ = case
    eye = torch.eye(4, device=DEV)
    monkeypatch.setattr(affine, "convex_adam_affine", lambda *a, **k: affine.AffineRegistration(eye, None, None))
    field, T = affine.register_with_affine(fixed, moving, **PT_KW)
    assert T is eye
    deformable = convex_adam_pt(fixed, affine_warp(moving[None], eye)[0], device=fixed.device, **PT_KW)
    bound = R.identity_bound(SHAPE)
    assert bound == 16.0 * 48 * 2.0 ** -53 and float(np.abs(deformable).max()) > 0.1
    assert float(np.abs(field.cpu().numpy() - deformable).max()) <= bound
