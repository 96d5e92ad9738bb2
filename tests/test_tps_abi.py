"""CPU checks of the thin-plate-spline entry points (csrc/tps.hip): the library exports them, the ctypes table and the header agree,
and argument validation answers before any launch (no GPU is touched here)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "convexadam_hip.h")
NEW = ("cvx_tps_fit_workspace_bytes", "cvx_tps_fit_f32", "cvx_tps_eval_f32", "cvx_tps_dense_f32", "cvx_resize_trilinear_ac_f32")
FAKE = C.c_void_p(256)        # never dereferenced: every call below fails validation on the host


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    return _lib.lib()


def test_header_table_and_library_agree_on_the_tps_entry_points(L):
    from convexadam_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
    assert L.cvx_version() == 2 == _lib.ABI_VERSION


def test_fit_workspace_query(L):
    assert L.cvx_tps_fit_workspace_bytes(0, 3) == 0
    assert L.cvx_tps_fit_workspace_bytes(16385, 3) == 0
    assert L.cvx_tps_fit_workspace_bytes(10, 0) == 0 and L.cvx_tps_fit_workspace_bytes(10, 5) == 0
    small, big = L.cvx_tps_fit_workspace_bytes(100, 3), L.cvx_tps_fit_workspace_bytes(8192, 3)
    assert small >= 104 * 107 * 4
    assert big >= 8196 * 8199 * 4


def test_fit_validates_arguments(L):
    from convexadam_amd._lib import CVX_ERR_INVALID_ARG, CVX_ERR_WORKSPACE
    nws = L.cvx_tps_fit_workspace_bytes(50, 3)
    fit = L.cvx_tps_fit_f32
    assert fit(None, FAKE, 50, 3, 0.0, FAKE, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert fit(FAKE, FAKE, 50, 3, 0.0, None, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert fit(FAKE, FAKE, 50, 3, 0.0, FAKE, None, nws, None) == CVX_ERR_INVALID_ARG
    assert fit(FAKE, FAKE, 0, 3, 0.0, FAKE, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert fit(FAKE, FAKE, 50, 0, 0.0, FAKE, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert fit(FAKE, FAKE, 50, 5, 0.0, FAKE, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert fit(FAKE, FAKE, 50, 3, float("nan"), FAKE, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert fit(FAKE, FAKE, 50, 3, float("inf"), FAKE, FAKE, nws, None) == CVX_ERR_INVALID_ARG
    assert fit(FAKE, FAKE, 50, 3, 0.0, FAKE, FAKE, nws - 1, None) == CVX_ERR_WORKSPACE
    assert b"workspace" in L.cvx_last_error()


def test_eval_dense_and_resize_validate_arguments(L):
    from convexadam_amd._lib import CVX_ERR_INVALID_ARG
    assert L.cvx_tps_eval_f32(None, 10, FAKE, FAKE, 5, 3, FAKE, None) == CVX_ERR_INVALID_ARG
    assert L.cvx_tps_eval_f32(FAKE, -1, FAKE, FAKE, 5, 3, FAKE, None) == CVX_ERR_INVALID_ARG
    assert L.cvx_tps_eval_f32(FAKE, 10, FAKE, FAKE, 0, 3, FAKE, None) == CVX_ERR_INVALID_ARG
    assert L.cvx_tps_eval_f32(FAKE, 10, FAKE, FAKE, 5, 5, FAKE, None) == CVX_ERR_INVALID_ARG
    assert L.cvx_tps_eval_f32(FAKE, 0, FAKE, FAKE, 5, 3, FAKE, None) == 0          # nothing to do, nothing launched
    assert L.cvx_tps_dense_f32(0, 4, 4, FAKE, FAKE, 5, 3, FAKE, None) == CVX_ERR_INVALID_ARG
    assert L.cvx_tps_dense_f32(4, 4, 4, None, FAKE, 5, 3, FAKE, None) == CVX_ERR_INVALID_ARG
    assert L.cvx_tps_dense_f32(4, 4, 4, FAKE, FAKE, 0, 3, FAKE, None) == CVX_ERR_INVALID_ARG
    assert L.cvx_tps_dense_f32(4, 4, 4, FAKE, FAKE, 5, 0, FAKE, None) == CVX_ERR_INVALID_ARG
    assert L.cvx_resize_trilinear_ac_f32(None, 3, 2, 2, 2, FAKE, 4, 4, 4, None) == CVX_ERR_INVALID_ARG
    assert L.cvx_resize_trilinear_ac_f32(FAKE, 3, 2, 0, 2, FAKE, 4, 4, 4, None) == CVX_ERR_INVALID_ARG
    assert L.cvx_resize_trilinear_ac_f32(FAKE, 0, 2, 2, 2, FAKE, 4, 4, 4, None) == CVX_ERR_INVALID_ARG


def test_python_layer_has_no_cpu_path():
    from convexadam_amd.convex_adam_utils import TPS, thin_plate_dense
    c = torch.rand(8, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        TPS.fit(c, torch.rand(8, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        thin_plate_dense(c.unsqueeze(0), torch.rand(1, 8, 3), (8, 8, 8), 2)


# ---- shape validation in tps.py: answered from tensor metadata before the device check, so CPU tensors with bad shapes raise ValueError
def _fit(c, f):
    from convexadam_amd.tps import TPS
    return TPS.fit(c, f)


def _z(x, c, theta):
    from convexadam_amd.tps import TPS
    return TPS.z(x, c, theta)


def _dense(c, theta, size):
    from convexadam_amd.tps import tps_dense
    return tps_dense(c, theta, size)


def _resize(x, size):
    from convexadam_amd.tps import resize_trilinear_ac
    return resize_trilinear_ac(x, size)


R = torch.rand
BAD_SHAPES = {
    "fit_c_no_centres": lambda: _fit(R(0, 3), R(0, 3)),
    "fit_c_two_coords": lambda: _fit(R(8, 2), R(8, 3)),
    "fit_c_1d": lambda: _fit(R(24), R(8, 3)),
    "fit_f_rows": lambda: _fit(R(8, 3), R(7, 3)),
    "fit_f_no_columns": lambda: _fit(R(8, 3), R(8, 0)),
    "fit_f_1d": lambda: _fit(R(8, 3), R(8)),
    "z_x_two_coords": lambda: _z(R(10, 2), R(8, 3), R(12, 3)),
    "z_x_1d": lambda: _z(R(30), R(8, 3), R(12, 3)),
    "z_c_two_coords": lambda: _z(R(10, 3), R(8, 2), R(12, 3)),
    "z_c_no_centres": lambda: _z(R(10, 3), R(0, 3), R(4, 3)),
    "z_theta_no_affine_rows": lambda: _z(R(10, 3), R(8, 3), R(8, 3)),
    "z_theta_no_columns": lambda: _z(R(10, 3), R(8, 3), R(12, 0)),
    "z_theta_1d": lambda: _z(R(10, 3), R(8, 3), R(12)),
    "dense_c_two_coords": lambda: _dense(R(8, 2), R(12, 3), (4, 4, 4)),
    "dense_theta_no_affine_rows": lambda: _dense(R(8, 3), R(8, 3), (4, 4, 4)),
    "dense_theta_no_columns": lambda: _dense(R(8, 3), R(12, 0), (4, 4, 4)),
    "dense_size_two_ints": lambda: _dense(R(8, 3), R(12, 3), (4, 4)),
    "dense_size_zero": lambda: _dense(R(8, 3), R(12, 3), (4, 0, 4)),
    "dense_size_negative": lambda: _dense(R(8, 3), R(12, 3), (4, 4, -2)),
    "dense_size_not_a_sequence": lambda: _dense(R(8, 3), R(12, 3), 4),
    "resize_x_4d": lambda: _resize(R(3, 4, 4, 4), (8, 8, 8)),
    "resize_x_6d": lambda: _resize(R(1, 1, 3, 4, 4, 4), (8, 8, 8)),
}


@pytest.mark.parametrize("case", sorted(BAD_SHAPES))
def test_bad_shapes_raise_value_error_before_the_device_check(case):
    with pytest.raises(ValueError):
        BAD_SHAPES[case]()


def test_valid_shapes_on_cpu_still_reach_the_device_check():
    from convexadam_amd.tps import TPS, resize_trilinear_ac, tps_dense
    c = torch.rand(8, 3)
    for call in (lambda: TPS.fit(c, torch.rand(8, 5)), lambda: TPS.z(torch.rand(10, 3), c, torch.rand(12, 2)),
                 lambda: tps_dense(c, torch.rand(12, 1), (4, 5, 6)), lambda: resize_trilinear_ac(torch.rand(2, 3, 4, 4, 4), (8, 8, 8))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
