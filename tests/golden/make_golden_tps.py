"""Golden of the thin-plate-spline densification (tests/test_gpu_tps.py), captured by EXECUTING the reference's own definitions (run
ONLY in the build container, on CPU):

    python tests/golden/make_golden_tps.py        # -> tests/golden/tps.npz

l2r_2021_convexAdam_task1_docker.py runs a whole challenge case at import time, so it cannot be imported: its `TPS` ClassDef and
`thin_plate_dense` FunctionDef nodes are lifted out of the parsed file with `ast`, compiled as they stand and run with this script's
globals.  `torch.solve(B, A)` (removed from torch) is provided as torch.linalg.solve(A, B) -- the same LU with partial pivoting.  No
reference text is stored.  Cases: n = 256 centres on (48, 40, 56) and n = 2048 on (160, 192, 224), step 4, centres drawn like task1
(a random subset of the masked stride-3 align_corners=True lattice), values a smooth random field plus noise.  To keep the file small
the output is stored at SAMPLES voxels per case (a seeded draw, always including the eight corners), with their flat indices.
"""
import ast
import math
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CONVEXADAM_REFERENCE", "/root/reference")
SCRIPT = "l2r_2021_convexAdam_task1_docker.py"
SAMPLES = 4096


def lift():
    tree = ast.parse(open(os.path.join(REF, SCRIPT)).read())
    nodes = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in ("TPS", "thin_plate_dense")]
    assert len(nodes) == 2
    torch_ns = types.ModuleType("torch_with_solve")
    torch_ns.__dict__.update({k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})
    torch_ns.solve = lambda B, A: (torch.linalg.solve(A, B), None)
    ns = dict(torch=torch_ns, F=F, math=math)
    exec(compile(ast.Module(body=nodes, type_ignores=[]), SCRIPT, "exec"), ns)
    return ns["TPS"], ns["thin_plate_dense"]


def centres_and_values(shape, n, g):
    """A task1-like draw: the stride-3 align_corners=True lattice inside an ellipsoid mask, n of its points by randperm; values a
    smooth field (a few sines, normalised-displacement scale) plus noise."""
    H, W, D = shape
    ident = F.affine_grid(torch.eye(3, 4).unsqueeze(0), (1, 1, H // 3, W // 3, D // 3), align_corners=True).view(-1, 3)
    inside = (ident ** 2).sum(1) < 0.85
    pts = ident[inside]
    x1 = pts[torch.randperm(pts.shape[0], generator=g)[:n]]
    a = torch.rand(3, 3, generator=g) * 3 + 1
    ph = torch.rand(3, 3, generator=g) * 6
    y1 = torch.stack([sum(0.02 * torch.sin(a[k, i] * x1[:, i] + ph[k, i]) for i in range(3)) for k in range(3)], 1)
    y1 = y1 + 0.002 * torch.randn(n, 3, generator=g)
    return x1.contiguous(), y1.contiguous()


def main():
    _, thin_plate_dense = lift()
    g = torch.Generator().manual_seed(2021)
    out = {}
    for tag, n, shape in (("small", 256, (48, 40, 56)), ("large", 2048, (160, 192, 224))):
        x1, y1 = centres_and_values(shape, n, g)
        dense = thin_plate_dense(x1.unsqueeze(0), y1.unsqueeze(0), shape, 4, 0.)[0].reshape(-1, 3)
        H, W, D = shape
        corners = torch.tensor([(a * (H - 1) * W + b * (W - 1)) * D + e * (D - 1) for a in (0, 1) for b in (0, 1) for e in (0, 1)])
        idx = torch.unique(torch.cat([corners, torch.randperm(H * W * D, generator=g)[:SAMPLES - 8]]))
        out.update({tag + "_x1": x1.numpy(), tag + "_y1": y1.numpy(), tag + "_shape": np.array(shape, np.int64),
                    tag + "_idx": idx.numpy().astype(np.int32), tag + "_dense": dense[idx].contiguous().numpy()})
    path = os.path.join(HERE, "tps.npz")
    np.savez_compressed(path, **out)
    print("wrote tps.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
