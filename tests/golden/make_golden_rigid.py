"""Golden of the rigid fits (tests/test_gpu_rigid.py), captured by EXECUTING the reference's own find_rigid_3d and least_trimmed_rigid
(convex_adam_utils.py:173-193) on CPU in float32 (run ONLY in the build container):

    python tests/golden/make_golden_rigid.py        # -> tests/golden/rigid.npz

Only inputs and outputs are stored.  Cases (homogeneous (N, 4) points, unit scale):
  clean      a rigid motion of an anisotropic cloud plus 1e-3 noise;
  outliers   the same with a third of the points moved far away (gross outliers);
  reflection moving = fixed mirrored in z (the det(V U^T) = -1 branch of the reference);
  planar     fixed points in the plane z = 0.3;
  field      a CuRIOUS-like case (l2r_2020_convexAdam_CuRIOUS.py:349-367): a smooth random field plus a rotation of a few degrees on a
             40 x 36 x 44 volume, the identity and identity + field coordinates sampled by F.grid_sample at the F.affine_grid centres of
             the coarse (grid_sp 2) cells inside an ellipsoid mask.
Per case: find_rigid_3d on all points (key <tag>_find) and least_trimmed_rigid for iter = 1, 2, 5, 15 (<tag>_lts<k>).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import import_reference  # noqa: E402

ITERS = (1, 2, 5, 15)


def rotation(g, degrees):
    axis = torch.randn(3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm()
    a = np.deg2rad(degrees)
    K = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def homog(p):
    return torch.cat([p, torch.ones(p.shape[0], 1, dtype=p.dtype)], 1).float().contiguous()


def cloud(g, n):
    return torch.randn(n, 3, generator=g, dtype=torch.float64) * torch.tensor([0.6, 0.35, 0.2], dtype=torch.float64)


def field_case(g):
    H, W, D, sp = 40, 36, 44, 2
    R = rotation(g, 4.0)
    ident = F.affine_grid(torch.eye(3, 4).unsqueeze(0), (1, 1, H, W, D), align_corners=False)
    smooth = F.interpolate(torch.randn(1, 3, 5, 5, 6, generator=g) * 0.02, (H, W, D), mode="trilinear", align_corners=False)
    rig = (ident.view(-1, 3).double() @ R.T - ident.view(-1, 3).double()).float().view(1, H, W, D, 3) + 0.01
    disp0 = rig + smooth.permute(0, 2, 3, 4, 1)
    sp_grid = F.affine_grid(torch.eye(3, 4).unsqueeze(0), (1, 1, H // sp, W // sp, D // sp), align_corners=False)
    mask = (sp_grid ** 2).sum(-1).view(-1) < 0.7
    pts = sp_grid.reshape(-1, 3)[torch.nonzero(mask).squeeze(1), :]
    T1 = F.grid_sample(ident.permute(0, 4, 1, 2, 3), pts.reshape(1, -1, 1, 1, 3), align_corners=False)
    T2 = F.grid_sample((ident + disp0).permute(0, 4, 1, 2, 3), pts.reshape(1, -1, 1, 1, 3), align_corners=False)
    T1 = torch.cat((T1.squeeze().t(), torch.ones(pts.shape[0], 1)), 1)
    T2 = torch.cat((T2.squeeze().t(), torch.ones(pts.shape[0], 1)), 1)
    return T1.contiguous(), T2.contiguous()


def main():
    utils, _ = import_reference()
    g = torch.Generator().manual_seed(2020)
    cases = {}
    x = cloud(g, 3000)
    R, t = rotation(g, 25.0), torch.tensor([0.1, -0.05, 0.2], dtype=torch.float64)
    cases["clean"] = (homog(x), homog(x @ R.T + t + 1e-3 * torch.randn(3000, 3, generator=g, dtype=torch.float64)))
    x = cloud(g, 3000)
    R, t = rotation(g, 40.0), torch.tensor([-0.2, 0.15, 0.05], dtype=torch.float64)
    y = x @ R.T + t + 1e-2 * torch.randn(3000, 3, generator=g, dtype=torch.float64)
    out = torch.randperm(3000, generator=g)[:1000]
    y[out] += torch.randn(1000, 3, generator=g, dtype=torch.float64) * 0.8
    cases["outliers"] = (homog(x), homog(y))
    x = cloud(g, 1500)
    cases["reflection"] = (homog(x), homog(x * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)
                                          + 1e-3 * torch.randn(1500, 3, generator=g, dtype=torch.float64)))
    x = cloud(g, 1200)
    x[:, 2] = 0.3
    R, t = rotation(g, 15.0), torch.tensor([0.0, 0.1, -0.1], dtype=torch.float64)
    cases["planar"] = (homog(x), homog(x @ R.T + t + 1e-3 * torch.randn(1200, 3, generator=g, dtype=torch.float64)))
    cases["field"] = field_case(g)
    res = {}
    for tag, (f, m) in cases.items():
        res[tag + "_fixed"], res[tag + "_moving"] = f.numpy(), m.numpy()
        res[tag + "_find"] = utils.find_rigid_3d(f, m).numpy()
        for k in ITERS:
            res["%s_lts%d" % (tag, k)] = utils.least_trimmed_rigid(f, m, k).numpy()
    path = os.path.join(HERE, "rigid.npz")
    np.savez_compressed(path, **res)
    print("wrote rigid.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
