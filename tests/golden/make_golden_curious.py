"""Golden of the CuRIOUS rigid registration (tests/test_gpu_rigid_registration.py, tests/test_oracle_curious.py), captured by EXECUTING
the reference's own code on the CPU in float32 (run ONLY in the build container):

    python tests/golden/make_golden_curious.py        # -> tests/golden/curious.npz

l2r_2020_convexAdam_CuRIOUS.py runs a whole challenge case at import time, so it cannot be imported; its `correlate`, `coupled_convex` and
`inverse_consistency` FunctionDef nodes are lifted out of the parsed file with `ast`, compiled as they stand and called (patched only
as make_golden_variants.py patches: torch.cuda.synchronize, prints).  MINDSSC, find_rigid_3d and least_trimmed_rigid come from the
reference's convex_adam_utils.  No reference text is stored: only the small coarse inputs and the outputs.

Case: 48 x 42 x 54 zero-background phantom (40 x + 100 inside the ellipsoid, so that the script's threshold 10 separates it from the
background), moved by 4 degrees and about 4 voxels per axis (more than half a coarse cell everywhere: a smaller motion gives an all-zero
coarse field at grid_sp 6), a second moving modality by a non-linear intensity map; grid_sp 6, disp_hw 3, MINDSSC(., 3, 3), 5
inverse-consistency steps, float32 throughout (the script's .half() storage is not part of the parity mode).  Script lines :323-365.
Stored: mask_fix, mask_mov, feat_fix, feat_mov (24 channels), soft_fwd, soft_rev (masked disp_soft of both directions), soft_fwd_plain
(unmasked), disp_ice, coarse (disp_ice.flip(1) * scale * grid_sp), every third plane of disp_hr + the int64 sum of all its bit patterns (an order-independent checksum), T1, T2, R.
"""
import ast
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from _ref_import import REF_ROOT, import_reference  # noqa: E402

SCRIPT = "l2r_2020_convexAdam_CuRIOUS.py"
SHAPE, GRID_SP, DISP_HW, IC_ITERS, LTS_ITERS, THRESH = (48, 42, 54), 6, 3, 5, 15, 10.0


def lift(name):
    tree = ast.parse(open(os.path.join(REF_ROOT, SCRIPT)).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    ns = dict(torch=torch, F=F, time=time, np=np, gpu_usage=lambda: None, print=lambda *a, **k: None)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), SCRIPT, "exec"), ns)
    return ns[name]


def images():
    """The pair of tests/test_gpu_rigid_registration.py::phantom_case (the same expressions, torch CPU)."""
    from convexadam_amd.phantom import ellipsoid_mask, zero_background_pair
    fix, _ = zero_background_pair(SHAPE)
    fixed = ((40.0 * fix + 100.0) * ellipsoid_mask(SHAPE, 0.42)).contiguous()
    ang = np.deg2rad(4.0)
    A = torch.tensor([[np.cos(ang), -np.sin(ang), 0.0, 0.15], [np.sin(ang), np.cos(ang), 0.0, -0.16], [0.0, 0.0, 1.0, 0.14]], dtype=torch.float32)
    grid = F.affine_grid(A[None], (1, 1) + SHAPE, align_corners=False)
    moving = F.grid_sample(fixed[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0, 0].contiguous()
    moving2 = torch.where(moving > 0, 300.0 - 0.004 * (moving - 100.0) ** 2 - moving, torch.zeros(())).clamp_min(0.0).contiguous()
    return fixed, moving, moving2


def main():
    torch.set_num_threads(8)
    torch.cuda.synchronize = lambda *a, **k: None
    utils, _ = import_reference()
    correlate, coupled_convex, inverse_consistency = lift("correlate"), lift("coupled_convex"), lift("inverse_consistency")
    H, W, D = SHAPE
    g, hw = GRID_SP, DISP_HW
    fixed, moving, moving2 = images()
    with torch.no_grad():
        # :323-330
        pool = lambda img: F.avg_pool3d(utils.MINDSSC(img[None, None], 3, 3, device="cpu"), g, stride=g)   # noqa: E731
        pf = pool(fixed)
        mind_fix = torch.cat((pf, pf), 1)
        mind_mov = torch.cat((pool(moving), pool(moving2)), 1)
        mask_mov = F.avg_pool3d((moving > THRESH).float()[None, None], g, stride=g) > .5
        mask_fix = F.avg_pool3d((fixed > THRESH).float()[None, None], g, stride=g) > .5
        for m in (mask_fix, mask_mov):
            assert 0.25 < float(m.float().mean()) < 0.75, "a mask keeps %.0f %% of the cells" % (100 * float(m.float().mean()))
        scale = torch.tensor([H // g - 1, W // g - 1, D // g - 1]).view(1, 3, 1, 1, 1).float() / 2                  # :332 (float32)
        # :335-338
        ssd, ssd_argmin = correlate(mind_fix, mind_mov, hw, g, (H, W, D))
        disp_mesh_t = F.affine_grid(hw * torch.eye(3, 4).unsqueeze(0), (1, 1, hw * 2 + 1, hw * 2 + 1, hw * 2 + 1), align_corners=True).permute(0, 4, 1, 2, 3).reshape(3, -1, 1)
        soft_plain = coupled_convex(ssd.clone(), ssd_argmin, disp_mesh_t, g, (H, W, D))
        ssd *= mask_fix.squeeze(1)
        disp_soft = coupled_convex(ssd, ssd_argmin, disp_mesh_t, g, (H, W, D))
        assert not torch.equal(disp_soft, soft_plain), "the mask changes nothing: the fixture could pass with the mask ignored"
        # :348-354
        ssd_, ssd_argmin_ = correlate(mind_mov, mind_fix, hw, g, (H, W, D))
        ssd_ *= mask_mov.squeeze(1)
        disp_soft_ = coupled_convex(ssd_, ssd_argmin_, disp_mesh_t, g, (H, W, D))
        disp_ice, _ = inverse_consistency((disp_soft / scale).flip(1), (disp_soft_ / scale).flip(1), iter=IC_ITERS)
        coarse = disp_ice.flip(1) * scale * g
        assert float(coarse.abs().max()) > 0, "all-zero coarse field"
        disp_hr = F.interpolate(coarse, size=(H, W, D), mode="trilinear", align_corners=False)
        # :356-367
        disp0 = disp_hr.float().permute(0, 2, 3, 4, 1) / torch.tensor([H - 1, W - 1, D - 1]).view(1, 1, 1, 1, 3) * 2
        disp0 = disp0.flip(4)
        affine = F.affine_grid(torch.eye(3, 4).unsqueeze(0), (1, 1, H, W, D), align_corners=False)
        affine_sp = F.affine_grid(torch.eye(3, 4).unsqueeze(0), (1, 1, H // g, W // g, D // g), align_corners=False)
        affine_sp = affine_sp.reshape(-1, 3)[torch.nonzero(mask_fix.reshape(-1)), :]
        T1 = F.grid_sample(affine.permute(0, 4, 1, 2, 3), affine_sp.reshape(1, -1, 1, 1, 3))
        T2 = F.grid_sample((affine + disp0).permute(0, 4, 1, 2, 3), affine_sp.reshape(1, -1, 1, 1, 3))
        T1 = torch.cat((T1.squeeze().t(), torch.ones(affine_sp.shape[0], 1)), 1)
        T2 = torch.cat((T2.squeeze().t(), torch.ones(affine_sp.shape[0], 1)), 1)
        R = utils.least_trimmed_rigid(T1, T2, LTS_ITERS)
    out = dict(shape=np.array(SHAPE, np.int64), grid_sp=np.int64(g), disp_hw=np.int64(hw), ic_iters=np.int64(IC_ITERS), lts_iters=np.int64(LTS_ITERS),
               mask_fix=mask_fix[0, 0].numpy(), mask_mov=mask_mov[0, 0].numpy(), feat_fix=mind_fix[0].numpy(), feat_mov=mind_mov[0].numpy(),
               soft_fwd=disp_soft[0].numpy(), soft_rev=disp_soft_[0].numpy(), soft_fwd_plain=soft_plain[0].numpy(), disp_ice=disp_ice[0].numpy(),
               coarse=coarse[0].numpy(), disp_hr_z3=disp_hr[0, :, ::3].contiguous().numpy(), disp_hr_bitsum=np.int64(disp_hr.contiguous().view(torch.int32).long().sum().item()),
               T1=T1.contiguous().numpy(), T2=T2.contiguous().numpy(), R=R.numpy())
    path = os.path.join(HERE, "curious.npz")
    np.savez_compressed(path, **out)
    print("wrote curious.npz %.1f KB; masks keep %.0f %% / %.0f %%; |coarse| max %.2f voxels; %d points"
          % (os.path.getsize(path) / 1024, 100 * float(mask_fix.float().mean()), 100 * float(mask_mov.float().mean()), float(coarse.abs().max()), T1.shape[0]))


if __name__ == "__main__":
    main()
