"""CPU checks of the rigid-fit and affine-warp entry points (csrc/rigid.hip): the library exports them, the ctypes table and the header
agree, argument validation answers before any launch, the Python layer rejects bad shapes from tensor metadata, and the reference's
module names expose find_rigid_3d / least_trimmed_rigid (no GPU is touched here)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "convexadam_hip.h")
NEW = ("cvx_rigid_lts_workspace_bytes", "cvx_rigid_lts_f32", "cvx_affine_warp_f32")
FAKE = C.c_void_p(256)        # never dereferenced: every call below fails validation on the host


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    return _lib.lib()


def test_header_table_and_library_agree_on_the_rigid_entry_points(L):
    from convexadam_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
    assert L.cvx_version() == 2 == _lib.ABI_VERSION


def test_lts_workspace_query(L):
    assert L.cvx_rigid_lts_workspace_bytes(1) == 0
    assert L.cvx_rigid_lts_workspace_bytes((1 << 28) + 1) == 0
    assert L.cvx_rigid_lts_workspace_bytes(85000) >= 85000 * 5


def test_lts_validates_arguments(L):
    from convexadam_amd._lib import CVX_ERR_INVALID_ARG, CVX_ERR_WORKSPACE
    nws = L.cvx_rigid_lts_workspace_bytes(100)
    lts = L.cvx_rigid_lts_f32
    assert lts(None, 4, FAKE, 4, 100, 5, FAKE, None, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert lts(FAKE, 4, None, 4, 100, 5, FAKE, None, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert lts(FAKE, 4, FAKE, 4, 100, 5, None, None, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert lts(FAKE, 4, FAKE, 4, 100, 5, FAKE, None, None, nws, None) == CVX_ERR_INVALID_ARG
    assert lts(FAKE, 4, FAKE, 4, 1, 5, FAKE, None, FAKE, nws, None) == CVX_ERR_INVALID_ARG          # n < 2
    assert lts(FAKE, 4, FAKE, 4, 100, 0, FAKE, None, FAKE, nws, None) == CVX_ERR_INVALID_ARG        # iters < 1
    assert lts(FAKE, 2, FAKE, 3, 100, 1, FAKE, None, FAKE, nws, None) == CVX_ERR_INVALID_ARG        # single fit: ld >= 3
    assert lts(FAKE, 3, FAKE, 4, 100, 5, FAKE, None, FAKE, nws, None) == CVX_ERR_INVALID_ARG        # trimmed fit: ld == 4
    assert lts(FAKE, 4, FAKE, 5, 100, 2, FAKE, None, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert lts(FAKE, 4, FAKE, 4, 100, 5, FAKE, None, FAKE, nws - 1, None) == CVX_ERR_WORKSPACE
    assert b"workspace" in L.cvx_last_error()


def test_warp_validates_arguments(L):
    from convexadam_amd._lib import CVX_ERR_INVALID_ARG, CVX_ERR_UNSUPPORTED
    warp = L.cvx_affine_warp_f32
    assert warp(None, 1, 4, 4, 4, FAKE, 4, 4, 4, 0, FAKE, None) == CVX_ERR_INVALID_ARG
    assert warp(FAKE, 1, 4, 4, 4, None, 4, 4, 4, 0, FAKE, None) == CVX_ERR_INVALID_ARG
    assert warp(FAKE, 1, 4, 4, 4, FAKE, 4, 4, 4, 0, None, None) == CVX_ERR_INVALID_ARG
    assert warp(FAKE, 0, 4, 4, 4, FAKE, 4, 4, 4, 0, FAKE, None) == CVX_ERR_INVALID_ARG
    assert warp(FAKE, 1, 4, 0, 4, FAKE, 4, 4, 4, 0, FAKE, None) == CVX_ERR_INVALID_ARG
    assert warp(FAKE, 1, 4, 4, 4, FAKE, 4, 4, 0, 0, FAKE, None) == CVX_ERR_INVALID_ARG
    assert warp(FAKE, 1, 4, 4, 4, FAKE, 4, 4, 4, 2, FAKE, None) == CVX_ERR_INVALID_ARG             # mode
    assert warp(FAKE, 1, 4, 4, 4, FAKE, 4, 4, 4, -1, FAKE, None) == CVX_ERR_INVALID_ARG
    assert b"mode" in L.cvx_last_error()
    assert warp(FAKE, 1, 4, 4, 4, FAKE, 2048, 2048, 1025, 0, FAKE, None) == CVX_ERR_UNSUPPORTED    # > 2^32 outputs


def test_python_layer_has_no_cpu_path():
    from convexadam_amd.rigid import affine_warp, find_rigid_3d, least_trimmed_rigid, rigid_from_field
    with pytest.raises(RuntimeError, match="no CPU path"):
        find_rigid_3d(torch.rand(10, 3), torch.rand(10, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        least_trimmed_rigid(torch.rand(10, 4), torch.rand(10, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        affine_warp(torch.rand(1, 4, 4, 4), torch.eye(4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        rigid_from_field(torch.rand(3, 8, 8, 8), torch.ones(2, 2, 2), 4)


@pytest.mark.parametrize("x, y", [((10,), (10, 3)), ((10, 2), (10, 3)), ((1, 3), (1, 3)), ((10, 3), (9, 3)), ((2, 10, 3), (10, 3))])
def test_find_rigid_3d_rejects_shapes(x, y):
    from convexadam_amd.rigid import find_rigid_3d
    with pytest.raises(ValueError):
        find_rigid_3d(torch.rand(*x), torch.rand(*y))


def test_find_rigid_3d_takes_wide_points_on_the_shape_check():
    from convexadam_amd.rigid import find_rigid_3d
    with pytest.raises(RuntimeError, match="no CPU path"):           # (N, 4) and (N, 5) pass the shape check, then the device check
        find_rigid_3d(torch.rand(10, 4), torch.rand(10, 5))


@pytest.mark.parametrize("f, m, it", [((10, 3), (10, 3), 5), ((10, 4), (10, 5), 5), ((10, 4), (9, 4), 5), ((1, 4), (1, 4), 5),
                                      ((10, 4), (10, 4), 0), ((10, 4), (10, 4), -3)])
def test_least_trimmed_rigid_rejects_shapes_and_iter(f, m, it):
    from convexadam_amd.rigid import least_trimmed_rigid
    with pytest.raises(ValueError):
        least_trimmed_rigid(torch.rand(*f), torch.rand(*m), it)


@pytest.mark.parametrize("vol, theta, kw", [((4, 4, 4), (3, 4), {}), ((2, 1, 4, 4, 4), (3, 4), {}), ((1, 4, 4, 4), (2, 4), {}),
                                            ((1, 4, 4, 4), (2, 3, 4), {}), ((1, 4, 4, 4), (3, 4), {"mode": "bicubic"}),
                                            ((1, 4, 4, 4), (3, 4), {"size": (4, 4)}), ((1, 4, 4, 4), (3, 4), {"size": (4, 0, 4)}),
                                            ((0, 4, 4, 4), (3, 4), {})])
def test_affine_warp_rejects_shapes(vol, theta, kw):
    from convexadam_amd.rigid import affine_warp
    with pytest.raises(ValueError):
        affine_warp(torch.rand(*vol), torch.rand(*theta), **kw)


@pytest.mark.parametrize("disp, mask, g", [((2, 8, 8, 8), (2, 2, 2), 4), ((3, 8, 8, 8), (2, 2, 3), 4), ((3, 8, 8, 8), (2, 2, 2), 16),
                                           ((2, 3, 8, 8, 8), (2, 2, 2), 4), ((3, 8, 8, 8), (2, 2, 2, 2), 4)])
def test_rigid_from_field_rejects_shapes(disp, mask, g):
    from convexadam_amd.rigid import rigid_from_field
    with pytest.raises(ValueError):
        rigid_from_field(torch.rand(*disp), torch.ones(*mask), g)


def test_reference_module_names_expose_the_rigid_fits():
    from convexAdam.convex_adam_utils import find_rigid_3d, least_trimmed_rigid
    import convexAdam.convex_adam_utils as shim
    from convexadam_amd import rigid
    assert find_rigid_3d is rigid.find_rigid_3d and least_trimmed_rigid is rigid.least_trimmed_rigid
    assert {"find_rigid_3d", "least_trimmed_rigid", "affine_warp", "rigid_from_field"} <= set(shim.__all__)
    from convexAdam_hyper_util import find_rigid_3d as f2, least_trimmed_rigid as l2
    assert f2 is rigid.find_rigid_3d and l2 is rigid.least_trimmed_rigid
