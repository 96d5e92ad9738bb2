"""CPU checks of the field-mean entry points (csrc/fieldmean.hip) and of the device= keyword of convex_adam_translation: header, binding
and exports agree, the ABI version is unchanged, every refusal returns its status code and message before anything is launched, the
Python layer refuses CPU tensors, and device=None still takes the host path.  No kernel is launched here.

Status codes: CVX_ERR_INVALID_ARG (-1) for every refused argument; a workspace below the query's size is CVX_ERR_WORKSPACE (-2), the code
the header defines for exactly that and every other operator with a workspace returns (tests/test_ssim_abi.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
IDENT = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
MAP = IDENT + [0.0, 0.0, 0.0]


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    return _lib.lib()


def doubles(v):
    return (C.c_double * len(v))(*v)


def test_header_binding_and_exports_agree(L):
    from convexadam_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "convexadam_hip.h")).read(), flags=re.S)
    for name, restype, cres in (("cvx_field_mean_f64", "int", C.c_int), ("cvx_field_mean_workspace_bytes", "size_t", C.c_size_t)):
        decl = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (restype, name), src)
        assert decl, "%s is not declared in the header" % name
        assert name in _lib.SIGNATURES and hasattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert res is cres and len(args) == len(decl.group(1).split(","))
    assert _lib.SIGNATURES["cvx_field_mean_f64"][1][-1] is C.c_void_p                       # the stream
    assert re.search(r"#define\s+CVX_ABI_VERSION\s+2\b", src)
    assert L.cvx_version() == 2 == _lib.ABI_VERSION
    assert "fieldmean.hip" in __import__("convexadam_amd.csrc.build", fromlist=["SOURCES"]).SOURCES


def test_refusals(L):
    f, mk, sg, out, ws = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), 5 << 20, C.c_void_p(6 << 20)
    V = 4 * 5 * 6
    need = L.cvx_field_mean_workspace_bytes(4, 5, 6)
    assert need > 0

    def call(field=f, f64=0, cs=V, vs=1, ext=(4, 5, 6), quantize=0, mask=None, seg=None, kind=0, sext=(3, 4, 5), m=None, sums=C.c_void_p(out),
             count=C.c_void_p(out + 24), wsp=ws, nbytes=1 << 20):
        return L.cvx_field_mean_f64(field, f64, cs, vs, *ext, quantize, mask, seg, kind, *sext, doubles(m) if m is not None else None, sums, count, wsp,
                                    nbytes, None)

    assert call(field=None) == -1 and b"null" in L.cvx_last_error()
    assert call(sums=None) == -1 and b"null" in L.cvx_last_error()
    assert call(count=None) == -1 and b"null" in L.cvx_last_error()
    for i in range(3):
        for bad in (0, -2):
            ext = [4, 5, 6]
            ext[i] = bad
            assert call(ext=tuple(ext)) == -1 and b"extent" in L.cvx_last_error(), (i, bad)
            assert call(seg=sg, m=MAP, sext=tuple(ext)) == -1 and b"extent" in L.cvx_last_error(), (i, bad)
    big = (1 << 11, 1 << 10, 1 << 10)                                   # 2^31 voxels: one more than an int holds
    assert call(ext=big) == -1 and b"2^31" in L.cvx_last_error()
    assert call(ext=(1 << 16, 1 << 16, 1)) == -1 and b"2^31" in L.cvx_last_error()
    assert call(seg=sg, m=MAP, sext=big) == -1 and b"2^31" in L.cvx_last_error()
    for cs, vs in ((0, 3), (1, 0), (-1, 3), (1, -3), (1, 2), (V - 1, 1), (2, 5), (1 << 41, 1), (1, 1 << 21)):
        assert call(cs=cs, vs=vs) == -1 and b"strides" in L.cvx_last_error(), (cs, vs)
    for k in range(12):
        for bad in (NAN, INF, -INF):
            m = list(MAP)
            m[k] = bad
            assert call(seg=sg, m=m) == -1 and b"non-finite" in L.cvx_last_error(), (k, bad)
    assert call(seg=sg) == -1 and b"index map" in L.cvx_last_error()                       # seg without map12
    assert call(mask=mk, seg=sg, m=MAP) == -1 and b"both" in L.cvx_last_error()
    assert call(quantize=1, f64=1, cs=1, vs=3) == -1 and b"float32" in L.cvx_last_error()
    for q in (-1, 2):
        assert call(quantize=q) == -1 and b"quantize" in L.cvx_last_error()
    for kind in (-1, 3):
        assert call(seg=sg, m=MAP, kind=kind) == -1 and b"seg_kind" in L.cvx_last_error()
    # outputs on inputs
    at = lambda base, off: C.c_void_p((base << 20) + off)             # noqa: E731
    assert call(sums=f) == -1 and b"overlaps an input" in L.cvx_last_error()
    assert call(count=at(1, 3 * V * 4 - 4)) == -1 and b"overlaps an input" in L.cvx_last_error()                 # on the planar field's last element
    assert call(f64=1, cs=1, vs=3, count=at(1, 3 * V * 8 - 8)) == -1 and b"overlaps an input" in L.cvx_last_error()   # ... the interleaved one's
    assert call(mask=mk, sums=at(2, V - 1)) == -1 and b"overlaps an input" in L.cvx_last_error()                 # on the mask's last byte
    assert call(seg=sg, m=MAP, count=at(3, 3 * 4 * 5 * 8 - 8)) == -1 and b"overlaps an input" in L.cvx_last_error()
    assert call(seg=sg, m=MAP, kind=1, count=at(3, 3 * 4 * 5 * 4 - 4)) == -1 and b"overlaps an input" in L.cvx_last_error()
    assert call(wsp=at(1, 64)) == -1 and b"overlaps an input" in L.cvx_last_error()
    assert call(wsp=at(1, -(need - 1))) == -1 and b"overlaps an input" in L.cvx_last_error()                     # its last byte on the field's first
    # ... and on each other
    assert call(count=C.c_void_p(out + 16)) == -1 and b"each other" in L.cvx_last_error()
    assert call(wsp=C.c_void_p(out + 8)) == -1 and b"each other" in L.cvx_last_error()
    assert call(wsp=C.c_void_p(out + 24 - (need - 1))) == -1 and b"each other" in L.cvx_last_error()             # its last byte on the count
    # a workspace below the query's size
    assert call(nbytes=need - 1) == -2 and b"workspace" in L.cvx_last_error()
    assert call(nbytes=0) == -2 and call(wsp=None) == -2
    # refused arguments come before the workspace is looked at
    assert call(ext=(0, 5, 6), nbytes=0) == -1 and call(sums=None, wsp=None) == -1


def test_workspace_query(L):
    from translation_restatement import S
    q = L.cvx_field_mean_workspace_bytes
    assert q(1, 1, 1) > 0 and q(160, 192, 224) > 4 * 8 * (160 * 192 * 224 // S) and q(160, 192, 224) < (1 << 20)
    assert q(1, 1, S) == q(1, 1, 1) and q(1, 1, S + 1) > q(1, 1, S)                          # one block, then two
    last = 0
    for n in (1, 2, 17, 256, 257, 4096):
        cur = q(n, 16, 16)
        assert cur >= last
        last = cur
    assert q(0, 5, 6) == 0 and b"extent" in L.cvx_last_error()
    assert q(4, -1, 6) == 0 and q(1 << 11, 1 << 10, 1 << 10) == 0


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from convexadam_amd import geometry
    from convexadam_amd.convex_adam_utils import field_mean_device
    import convexAdam.convex_adam_utils as shim
    assert shim.field_mean_device is geometry.field_mean_device is field_mean_device
    g = geometry.Grid((6, 5, 4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(IDENT))
    with pytest.raises(RuntimeError, match="no CPU"):
        geometry.field_mean_device(torch.zeros(4, 5, 6, 3), g)
    with pytest.raises(RuntimeError, match="no CPU"):
        geometry.field_mean_device(torch.zeros(3, 4, 5, 6), g, quantize=torch.float16)
    with pytest.raises(TypeError):
        geometry.field_mean_device(np.zeros((4, 5, 6, 3)), g)


def test_translation_keeps_the_host_path_without_a_device(monkeypatch):
    """device=None: resample_img, resample_moving_to_fixed, convex_adam_pt and the numpy mean, as before; nothing of the device path"""
    import inspect
    from convexadam_amd import convex_adam_translation as T
    from convexadam_amd.imageio import Image
    import convexAdam.convex_adam_translation as shim
    assert shim.convex_adam_translation is T.convex_adam_translation
    for fn in (T.convex_adam_translation, T.convex_adam_translation_from_file):
        assert inspect.signature(fn).parameters["device"].default is None
    assert list(inspect.signature(T.convex_adam_translation).parameters) == ["fixed_image", "moving_image", "segmentation", "co_moving_images", "device"]
    calls = []
    field = np.zeros((4, 5, 6, 3))
    field[..., 0], field[..., 2] = 2.2, -0.9

    def fake_pt(img_fixed, img_moving, **kw):
        calls.append("convex_adam_pt")
        assert not kw and img_fixed.array.shape == (4, 5, 6)
        return field

    def no_device(*a, **k):
        raise AssertionError("the device path ran")

    monkeypatch.setattr(T, "convex_adam_pt", fake_pt)
    monkeypatch.setattr(T, "translation_mean_device", no_device)
    monkeypatch.setattr(T, "register_on_1mm_device", no_device)
    img = Image(np.zeros((4, 5, 6), np.float32))
    co = [Image(np.zeros((4, 5, 6), np.float32), origin=(1.0, 2.0, 3.0))]
    t_xyz, moved, co_out = T.convex_adam_translation(img, img, co_moving_images=co)
    assert calls == ["convex_adam_pt"] and t_xyz == (-1.0, 0.0, 2.0)
    assert moved.GetOrigin() == (1.0, 0.0, -2.0) and co_out[0].GetOrigin() == (2.0, 2.0, 1.0)
    assert T.field_to_translation(field, (1.0, 1.0, 2.0)) == (-1.0, 0.0, 2.0)
    assert T.field_to_translation(field, (1.0, 1.0, 1.0), np.ones((4, 5, 6), bool)) == (-1.0, 0.0, 2.0)
    # the command line hands --device on, and leaves it None without the flag
    seen = []
    monkeypatch.setattr(T, "convex_adam_translation_from_file", lambda *a, **k: seen.append(k.get("device")) or (0.0, 0.0, 0.0))
    assert T.main(["--fixed_path", "a", "--moving_path", "b"]) == 0 and T.main(["--fixed_path", "a", "--moving_path", "b", "--device", "cuda"]) == 0
    assert seen == [None, "cuda"]
    # a device that is not a HIP device is refused, not quietly run on the host
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="HIP"):
        T.convex_adam_translation(img, img, device="cpu")
