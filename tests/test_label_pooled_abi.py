"""CPU checks of the label entries (no kernel is launched): cvx_label_features_pooled_f32, cvx_register_label_pair_workspace_bytes and
cvx_register_label_pair_f32 are exported, declared and bound; every argument they refuse is refused with a negative status and a
message before a device is touched; the label pair's workspace is the feature pair's and far below one one-hot volume."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "convexadam_hip.h")
NEW = ("cvx_label_features_pooled_f32", "cvx_register_label_pair_workspace_bytes", "cvx_register_label_pair_f32")


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    return _lib.lib()


def params(shape=(48, 48, 48), C_=40, grid_sp=4, disp_hw=2, grid_sp_adam=2, lambda_weight=1.25, niter=2, ic=1):
    from convexadam_amd._lib import PairParams
    return PairParams(shape[0], shape[1], shape[2], 1, 2, lambda_weight, grid_sp, disp_hw, niter, 0, grid_sp_adam, ic, C_, 12.0)


def test_symbols_exported_declared_and_bound(L):
    from convexadam_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), "libconvexadam_hip.so does not export %s" % name
        assert re.search(r"\b%s\s*\(" % name, hdr), "header does not declare %s" % name
        assert name in _lib.SIGNATURES
    assert int(re.search(r"#define\s+CVX_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2 == L.cvx_version()      # symbols added, no struct changed
    # the argument counts of the header's prototypes and of the ctypes table agree
    for name in NEW:
        proto = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name


def refused(L, rc, word):
    assert rc < 0, rc
    assert word in L.cvx_last_error(), L.cvx_last_error()


def test_pooled_operator_refuses_bad_arguments(L):
    d, e = C.c_void_p(256), C.c_void_p(512)
    f = L.cvx_label_features_pooled_f32
    ok_tail = (C.c_float(10.0), 2, d, 0, None, None)
    refused(L, f(None, 8, 8, 8, 3, d, d, *ok_tail), b"null")
    refused(L, f(d, 8, 8, 8, 3, None, d, *ok_tail), b"null")
    refused(L, f(d, 8, 8, 8, 3, d, None, *ok_tail), b"null")
    refused(L, f(d, 8, 8, 8, 3, d, d, C.c_float(10.0), 2, None, 0, None, None), b"null")
    refused(L, f(d, 8, 0, 8, 3, d, d, *ok_tail), b"extent")
    for bad_c in (0, -1, 256, 1000):
        refused(L, f(d, 8, 8, 8, bad_c, d, d, *ok_tail), b"1 .. 255")
    refused(L, f(d, 8, 8, 8, 3, d, d, C.c_float(10.0), 0, d, 0, None, None), b"g1 >= 1")
    refused(L, f(d, 8, 8, 8, 3, d, d, C.c_float(10.0), 2, d, -1, e, None), b"g2 >= 0")
    refused(L, f(d, 8, 8, 7, 3, d, d, C.c_float(10.0), 8, d, 0, None, None), b"larger than the volume")
    refused(L, f(d, 8, 8, 8, 3, d, d, C.c_float(10.0), 2, d, 9, e, None), b"larger than the volume")
    refused(L, f(d, 8, 8, 8, 3, d, d, C.c_float(10.0), 4, d, 2, None, None), b"out2 NULL iff g2 == 0")
    refused(L, f(d, 8, 8, 8, 3, d, d, C.c_float(10.0), 4, d, 0, e, None), b"out2 NULL iff g2 == 0")


def test_label_pair_refuses_bad_arguments(L):
    d = C.c_void_p(256)
    f = L.cvx_register_label_pair_f32
    p = params()
    nws = L.cvx_register_label_pair_workspace_bytes(C.byref(p))
    assert nws > 0
    big = 1 << 40
    for missing in range(4):                                           # either label map, the channel labels, the weights
        a = [d, d, d, d]
        a[missing] = None
        refused(L, f(*a, C.c_float(10.0), C.byref(p), d, None, d, big, None), b"missing")
    refused(L, f(d, d, d, d, C.c_float(10.0), None, d, None, d, big, None), b"null params")
    refused(L, f(d, d, d, d, C.c_float(10.0), C.byref(p), None, None, d, big, None), b"null")
    refused(L, f(d, d, d, d, C.c_float(10.0), C.byref(p), d, None, None, big, None), b"null")
    assert f(d, d, d, d, C.c_float(10.0), C.byref(p), d, None, d, nws - 1, None) == -2 and b"workspace" in L.cvx_last_error()
    zero = params(C_=0)
    refused(L, f(d, d, d, d, C.c_float(10.0), C.byref(zero), d, None, d, big, None), b"n_feat")
    assert L.cvx_register_label_pair_workspace_bytes(C.byref(zero)) == 0 and b"n_feat" in L.cvx_last_error()
    many = params(C_=256)
    refused(L, f(d, d, d, d, C.c_float(10.0), C.byref(many), d, None, d, big, None), b"n_feat")
    assert L.cvx_register_label_pair_workspace_bytes(C.byref(many)) == 0
    small = params(shape=(4, 48, 48), grid_sp=4)                       # one coarse cell along H
    refused(L, f(d, d, d, d, C.c_float(10.0), C.byref(small), d, None, d, big, None), b"too small")
    assert L.cvx_register_label_pair_workspace_bytes(None) == 0


@pytest.mark.parametrize("kw", [dict(), dict(lambda_weight=0.0), dict(ic=0), dict(lambda_weight=0.0, ic=0), dict(grid_sp=5, shape=(50, 45, 55)),
                                dict(C_=1), dict(C_=255, shape=(16, 16, 16))])
def test_label_pair_workspace_is_the_feature_pair_workspace(L, kw):
    """The pair layout for n_feat = C holds no full-resolution feature buffer and the label kernel uses no table: the two queries agree
    (the bound allows the S_k tables [2][C][g^3 + 1] a table-based kernel would add)."""
    p = params(**kw)
    a, b = L.cvx_register_pair_workspace_bytes(C.byref(p)), L.cvx_register_label_pair_workspace_bytes(C.byref(p))
    table_bytes = 4 * p.n_feat * ((p.grid_sp ** 3 + 1) + (p.grid_sp_adam ** 3 + 1)) + 2 * 256
    assert a > 0 and a <= b <= a + table_bytes


def test_label_pair_workspace_is_far_below_one_onehot_volume(L):
    shape, C_ = (48, 48, 48), 40
    p = params(shape=shape, C_=C_, grid_sp=4, disp_hw=2, grid_sp_adam=2, niter=2)
    nws = L.cvx_register_label_pair_workspace_bytes(C.byref(p))
    onehot = C_ * shape[0] * shape[1] * shape[2] * 4
    out_bytes = 3 * shape[0] * shape[1] * shape[2] * 4
    # the bound of the GPU memory test (workspace + field + 1 MB) is itself below ONE one-hot volume; the feature entry needs two of
    # them on top of the same workspace.  (No tighter constant: the two images' features pooled at grid_sp_adam = 2 and the Adam loop's
    # records of them are C V / 8 floats each, half a one-hot volume together, and belong to the workspace by design.)
    assert 0 < nws + out_bytes + (1 << 20) < onehot
    assert nws == L.cvx_register_pair_workspace_bytes(C.byref(p))


def test_python_entries_exist_and_refuse_the_cpu():
    import torch
    from convexadam_amd import convex_adam_nnUNet as N
    import convexAdam.convex_adam_nnUNet as shim
    for name in ("label_features_pooled", "register_labels_device", "extract_features", "convex_adam_pt", "convex_adam"):
        assert callable(getattr(N, name)) and getattr(shim, name) is getattr(N, name)
    if not torch.cuda.is_available():
        with pytest.raises(Exception):
            N.register_labels_device(torch.zeros(8, 8, 8), torch.zeros(8, 8, 8), grid_sp=2, disp_hw=1)
