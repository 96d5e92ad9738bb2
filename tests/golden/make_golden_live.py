"""Goldens for tests/test_oracle_vs_reference_live.py: the reference's outputs on inputs that are in no other golden file, captured from
the reference itself (run ONLY in the build container, the reference tree is not on the other hosts):

    python tests/golden/make_golden_live.py        # -> tests/golden/live.npz

Inputs are regenerated from seeds by the tests (torch.Generator / numpy default_rng / convexadam_amd.phantom); only the reference's
outputs are stored, the large ones as a sha256 of their bits (`digest`: shape, dtype and bytes, every NaN and zero made canonical,
which is what np.array_equal(..., equal_nan=True) compares) and the small ones as arrays.  The reference runs with this host's MKL
(asserted equal to the golden host's tables, so the tests replay it with mkl.golden_tables()); the whole pipelines at 3 and 8 torch
threads, everything else at 8."""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from convexadam_amd.phantom import ellipsoid_mask, phantom  # noqa: E402

# shared with tests/test_oracle_vs_reference_live.py (imported from here)
OPS_SHAPE, OPS_HW, OPS_C = (7, 9, 10), 3, 12
CONVEX_KW = dict(mind_r=1, mind_d=2, lambda_weight=0, grid_sp=4, disp_hw=3, ic=True)
BITS_CASES = (((44, 40, 48), 5, dict(mind_r=1, mind_d=2, lambda_weight=1.25, grid_sp=4, disp_hw=3, selected_niter=25, selected_smooth=3, grid_sp_adam=2, ic=True)),
              ((40, 48, 36), 9, dict(mind_r=2, mind_d=1, lambda_weight=0.5, grid_sp=3, disp_hw=2, selected_niter=12, selected_smooth=0, grid_sp_adam=1, ic=False)))
BITS_THREADS = (3, 8)
NAN_SHAPE, NAN_HW = (5, 6, 7), 2


def ops_inputs():
    g = torch.Generator().manual_seed(4242)
    f = torch.rand(1, OPS_C, *OPS_SHAPE, generator=g)
    m = torch.rand(1, OPS_C, *OPS_SHAPE, generator=g)
    a = 0.3 * torch.randn(1, 3, *OPS_SHAPE, generator=g)
    b = 0.3 * torch.randn(1, 3, *OPS_SHAPE, generator=g)
    return f, m, a, b


def mind_input():
    return torch.randn(1, 1, 14, 15, 33, generator=torch.Generator().manual_seed(77))


def convex_pair():
    return phantom((36, 32, 40), 31, 41), torch.roll(phantom((36, 32, 40), 31, 42), (2, -2, 1), (0, 1, 2))


def bits_pair(shape, seed):
    m = ellipsoid_mask(shape, 0.35)
    return phantom(shape, seed, 41) * m, torch.roll(phantom(shape, seed, 42), (2, -1, 1), (0, 1, 2)) * m


def nan_inputs():
    """The four NaN / Inf cases: (f, m) float32 (12, 5, 6, 7) each."""
    rng = np.random.default_rng(0)
    cases = []
    for case in range(4):
        f = rng.random((12,) + NAN_SHAPE, dtype=np.float32)
        m = rng.random((12,) + NAN_SHAPE, dtype=np.float32)
        if case == 0:
            m[3, 2, 3, 4] = np.nan                                        # some displacements of the neighbouring voxels see the NaN
        elif case == 1:
            m[0, 0, 0, 0] = np.nan
            f[5, 4, 5, 6] = np.inf
        elif case == 2:
            m[7, 1, 1, 1] = np.inf
            m[2, 3, 3, 3] = -np.inf
        else:
            f[:, 2, 2, 2] = np.nan                                        # every displacement of the neighbourhood is NaN
        cases.append((f, m))
    return cases


def digest(a):
    """sha256 of an array's shape, dtype and bits with every NaN made the default NaN and -0 made +0: two arrays have the same digest
    exactly when np.array_equal(a, b, equal_nan=True) holds and their shapes and dtypes agree."""
    x = np.ascontiguousarray(a)
    if x.dtype.kind == "f":
        x = np.ascontiguousarray(np.where(np.isnan(x), x.dtype.type(np.nan), x) + x.dtype.type(0))
    h = hashlib.sha256(("%s%s" % (x.dtype.str, x.shape)).encode())
    h.update(x.tobytes())
    return h.hexdigest()


def main():
    from _ref_import import import_reference
    utils, mind = import_reference()
    import mkl_tables
    from oracle import oracle
    assert mkl_tables.host_tables(oracle)["matches_golden_host"], "this host's MKL tables differ from the golden host's"
    torch.set_num_threads(8)
    out = {}
    # operators on random features: correlate -> coupled_convex, inverse_consistency
    f, m, a, b = ops_inputs()
    ssd, am = utils.correlate(f, m, OPS_HW, 1, OPS_SHAPE, OPS_C)
    out["ops_ssd_digest"], out["ops_argmin"] = np.array(digest(ssd.numpy())), am.numpy()
    n = 2 * OPS_HW + 1
    mesh_t = torch.nn.functional.affine_grid(OPS_HW * torch.eye(3, 4).unsqueeze(0), (1, 1, n, n, n), align_corners=True).permute(0, 4, 1, 2, 3).reshape(3, -1, 1)
    out["ops_soft"] = utils.coupled_convex(ssd, am, mesh_t, 1, OPS_SHAPE)[0].numpy()
    r1, r2 = utils.inverse_consistency(a, b, iter=7)
    out["ops_ic1"], out["ops_ic2"] = r1[0].numpy(), r2[0].numpy()
    # MIND-SSC
    out["mind_digest"] = np.array(digest(utils.MINDSSC(mind_input(), 1, 2, device="cpu")[0].numpy()))
    # the convex stage of the whole pipeline
    fix, mov = convex_pair()
    out["convex_field_digest"] = np.array(digest(mind.convex_adam_pt(fix, mov, dtype=torch.float32, device=torch.device("cpu"), **CONVEX_KW)))
    # whole pipelines, bits of the reference at 3 and 8 threads
    for i, (shape, seed, kw) in enumerate(BITS_CASES):
        fix, mov = bits_pair(shape, seed)
        for t in BITS_THREADS:
            torch.set_num_threads(t)
            r = mind.convex_adam_pt(fix, mov, dtype=torch.float32, device=torch.device("cpu"), **kw)
            out["bits%d_t%d_digest" % (i, t)] = np.array(digest(r))
    torch.set_num_threads(8)
    # NaN / Inf in the cost volume
    mesh = oracle.disp_mesh(NAN_HW)
    for case, (f, m) in enumerate(nan_inputs()):
        ssd, am = utils.correlate(torch.from_numpy(f)[None], torch.from_numpy(m)[None], NAN_HW, 1, NAN_SHAPE, 12)
        out["nan%d_ssd_digest" % case], out["nan%d_argmin" % case] = np.array(digest(ssd.numpy())), am.numpy()
        out["nan%d_soft" % case] = utils.coupled_convex(ssd, am, torch.from_numpy(mesh)[:, :, None], 1, NAN_SHAPE).numpy()[0]
    np.savez_compressed(os.path.join(HERE, "live.npz"), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == "__main__":
    main()
