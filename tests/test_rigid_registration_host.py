"""Host-side contract of the rigid-registration pieces (convexadam_amd/rigid.py, coupled_convex's cell_mask): shapes and arguments are
checked from tensor metadata before any device is touched, so a bad call is a ValueError for CPU tensors too; a good call on CPU tensors
is refused (there is no CPU path); the new entry points are declared, bound and exported.  No kernel is launched here."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_points_are_declared_bound_and_exported():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "convexadam_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ("cvx_threshold_pool_mask_u8", "cvx_coupled_convex_masked_f32", "cvx_label_centroids_i64"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    import convexadam_amd.convex_adam_utils as u
    for name in ("threshold_pool_mask", "label_centroids", "landmark_tre"):
        assert callable(getattr(u, name)), name


def test_library_refuses_bad_arguments_without_a_device():
    """Argument checks of the C entry points answer before any launch (null pointers, ranges)."""
    from convexadam_amd import _lib
    L = _lib.lib()
    assert L.cvx_threshold_pool_mask_u8(None, 8, 8, 8, 1.0, 2, None, None) == _lib.CVX_ERR_INVALID_ARG
    assert L.cvx_label_centroids_i64(None, 8, 8, 8, 3, None, None) == _lib.CVX_ERR_INVALID_ARG
    assert L.cvx_coupled_convex_masked_f32(None, None, None, None, 4, 4, 4, 2, None, None, 0, None) == _lib.CVX_ERR_INVALID_ARG
    assert b"null" in L.cvx_last_error()


@pytest.mark.parametrize("shape", [(8, 8), (2, 8, 8, 8), (8, 0, 8), ()])
def test_threshold_pool_mask_checks_the_shape(shape):
    from convexadam_amd.rigid import threshold_pool_mask
    with pytest.raises(ValueError):
        threshold_pool_mask(torch.zeros(shape), 10.0, 2)


@pytest.mark.parametrize("g", [0, -1, 65, 9, "x", None])
def test_threshold_pool_mask_checks_the_grid_spacing(g):
    from convexadam_amd.rigid import threshold_pool_mask
    with pytest.raises(ValueError):
        threshold_pool_mask(torch.zeros(8, 8, 8), 10.0, g)


def test_good_calls_on_cpu_tensors_are_refused_not_emulated():
    from convexadam_amd.rigid import label_centroids, landmark_tre, threshold_pool_mask
    with pytest.raises(RuntimeError, match="no CPU path"):
        threshold_pool_mask(torch.zeros(8, 8, 8), 10.0, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        label_centroids(torch.zeros(8, 8, 8), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        landmark_tre(torch.zeros(8, 8, 8), torch.zeros(8, 8, 8), 3)
    with pytest.raises(TypeError):
        threshold_pool_mask([[1.0]], 10.0, 1)


@pytest.mark.parametrize("max_label", [-1, 1024, "many", None])
def test_label_centroids_checks_max_label(max_label):
    from convexadam_amd.rigid import label_centroids
    with pytest.raises(ValueError):
        label_centroids(torch.zeros(4, 4, 4), max_label)


def test_label_centroids_and_tre_check_shapes():
    from convexadam_amd.rigid import label_centroids, landmark_tre
    with pytest.raises(ValueError):
        label_centroids(torch.zeros(4, 4), 3)
    with pytest.raises(ValueError):
        label_centroids(torch.zeros(3, 4, 4, 4), 3)
    with pytest.raises(ValueError, match="same extent"):
        landmark_tre(torch.zeros(4, 4, 4), torch.zeros(4, 4, 5), 3)
    with pytest.raises(ValueError):
        landmark_tre(torch.zeros(4, 4, 4), torch.zeros(4, 4, 4), 5000)


def test_coupled_convex_checks_the_cell_mask_before_the_device():
    from convexadam_amd.convex_adam_utils import coupled_convex
    ssd, am, mesh = torch.zeros(27, 4, 5, 6), torch.zeros(4, 5, 6, dtype=torch.int64), torch.zeros(3, 27, 1)
    for bad in (torch.ones(4, 5), torch.ones(4, 5, 7), torch.ones(2, 4, 5, 6), torch.ones(6, 5, 4)):
        with pytest.raises(ValueError, match="cell_mask"):
            coupled_convex(ssd, am, mesh, 2, (8, 10, 12), cell_mask=bad)
    with pytest.raises(ValueError, match="float32"):
        coupled_convex(ssd.half(), am, mesh, 2, (8, 10, 12), cell_mask=torch.ones(4, 5, 6))
    with pytest.raises(TypeError):
        coupled_convex(ssd, am, mesh, 2, (8, 10, 12), cell_mask=[1])
    with pytest.raises(RuntimeError, match="no CPU path"):                       # a good mask: the usual refusal of CPU tensors
        coupled_convex(ssd, am, mesh, 2, (8, 10, 12), cell_mask=torch.ones(1, 4, 5, 6, dtype=torch.bool))


def test_convex_stage_checks_shapes_before_the_device():
    from convexadam_amd.rigid import convex_stage
    ff, fm = torch.zeros(1, 24, 4, 5, 6), torch.zeros(1, 24, 4, 5, 6)
    shape = (8, 10, 12)
    for bad in (dict(feat_mov=torch.zeros(1, 12, 4, 5, 6)), dict(feat_fix=torch.zeros(24, 4, 5)), dict(shape=(8, 10)), dict(shape=(8, 10, 14)),
                dict(grid_sp=0), dict(disp_hw=-1), dict(ic_iters=-1), dict(mask_fix=torch.ones(4, 5, 7)), dict(mask_mov=torch.ones(2, 4, 5, 6)),
                dict(disp_hw=400)):
        kw = dict(feat_fix=ff, feat_mov=fm, grid_sp=2, disp_hw=2, shape=shape)
        kw.update(bad)
        with pytest.raises(ValueError):
            convex_stage(**kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        convex_stage(ff, fm, 2, 2, shape, mask_fix=torch.ones(4, 5, 6), ic_iters=5)


def test_convex_stage_params_mirror_the_header_and_refuse_a_reserved_tail():
    import ctypes as C
    from convexadam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "convexadam_hip.h")).read()
    body = re.search(r"typedef struct cvx_convex_stage_params \{(.*?)\} cvx_convex_stage_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*\]", "", piece.strip().split()[-1].lstrip("*")) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    assert names == [f[0] for f in _lib.StageParams._fields_]
    assert C.sizeof(_lib.StageParams) == 10 * 4 + 8 + 4 * 4
    L = _lib.lib()
    p = _lib.StageParams(24, 7, 7, 9, 3, 6, 5, 42, 42, 54)
    assert L.cvx_convex_stage_workspace_bytes(C.byref(p)) > 27 * 27 * 7 * 7 * 9 * 4
    q = _lib.StageParams(24, 7, 7, 9, 3, 6, 0, 42, 42, 54)
    assert 0 < L.cvx_convex_stage_workspace_bytes(C.byref(q)) < L.cvx_convex_stage_workspace_bytes(C.byref(p))
    p.reserved_[2] = 1
    assert L.cvx_convex_stage_workspace_bytes(C.byref(p)) == 0 and b"reserved" in L.cvx_last_error()
    assert L.cvx_convex_stage_f32(None, None, None, None, C.byref(q), None, None, None, 0, None) == _lib.CVX_ERR_INVALID_ARG


def test_convex_adam_rigid_checks_its_arguments_before_the_device():
    from convexadam_amd.rigid import convex_adam_rigid
    img = torch.zeros(24, 24, 30)
    for args, kw in (((img, torch.zeros(24, 24, 31)), {}), ((img, []), {}), ((img, [img, torch.zeros(24, 24)]), {}), ((torch.zeros(2, 24, 24, 30), img), {}),
                     ((img, img), dict(grid_sp=0)), ((img, img), dict(grid_sp=13)), ((img, img), dict(lts_iters=0)), ((img, img), dict(ic_iters=-2)),
                     ((img, img), dict(seg_fixed=img)), ((img, img), dict(seg_fixed=img, seg_moving=torch.zeros(24, 24, 29))), ((img, img), dict(mask_thresh="high"))):
        with pytest.raises(ValueError):
            convex_adam_rigid(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        convex_adam_rigid(img, [img, img])


def test_rigid_samples_checks_shapes_before_the_device():
    from convexadam_amd.rigid import rigid_samples
    coarse, mask = torch.zeros(1, 3, 4, 5, 6), torch.ones(4, 5, 6)
    for args in ((torch.zeros(1, 2, 4, 5, 6), mask, 2, (8, 10, 12)), (coarse, torch.ones(4, 5), 2, (8, 10, 12)), (coarse, mask, 3, (8, 10, 12)),
                 (coarse, mask, 0, (8, 10, 12)), (coarse, mask, 2, (8, 10)), (torch.zeros(3, 4, 5), mask, 2, (8, 10, 12))):
        with pytest.raises(ValueError):
            rigid_samples(*args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rigid_samples(coarse, mask, 2, (8, 10, 12))
    from convexadam_amd import _lib
    L = _lib.lib()
    assert L.cvx_rigid_samples_workspace_bytes(4, 5, 6, 8, 10, 12) > 4 * 120
    assert L.cvx_rigid_samples_f32(None, None, 4, 5, 6, 8, 10, 12, None, None, None, None, 0, None) == _lib.CVX_ERR_INVALID_ARG
