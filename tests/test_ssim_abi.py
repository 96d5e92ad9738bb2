"""CPU checks of the SSIM entry points (csrc/ssim.hip): every refusal with its status code and message, the workspace query, the
"no CPU" rule of the Python functions, and the tile extents ssim.py repeats for the tests.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    return _lib.lib()


def test_refusals(L):
    a, b, m, ws = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)
    big = C.c_size_t(1 << 30)

    def call(img1=a, img2=b, ext=(1, 1, 8, 8, 8), win=11, out_map=m, mean=None, slices=None, wsp=ws, nbytes=big):
        return L.cvx_ssim3d_f32(img1, img2, *ext, win, out_map, mean, slices, wsp, nbytes, None)

    assert call(img1=None) == -1 and b"null" in L.cvx_last_error()
    assert call(img2=None) == -1 and b"null" in L.cvx_last_error()
    for i in range(5):                                   # zero and negative extents, every axis
        for bad in (0, -3):
            ext = [2, 2, 8, 8, 8]
            ext[i] = bad
            assert call(ext=tuple(ext)) == -1 and b"extent" in L.cvx_last_error()
    assert call(out_map=None) == -1 and b"no output" in L.cvx_last_error()
    assert call(out_map=a) == -1 and b"overlaps" in L.cvx_last_error()                       # map on img1
    assert call(out_map=b) == -1 and b"overlaps" in L.cvx_last_error()                       # map on img2
    assert call(out_map=C.c_void_p((2 << 20) + 8 * 8 * 8 * 4 - 4)) == -1 and b"overlaps" in L.cvx_last_error()   # ... on its last voxel
    for win in (0, 2, 10, 12):
        assert call(win=win) == -1 and b"odd" in L.cvx_last_error(), win
    assert call(win=-1) == -1
    for win in (13, 15, 101):
        assert call(win=win) == -4 and b"at most 11" in L.cvx_last_error(), win
    # the means need the workspace of the query; the map alone needs none
    need = L.cvx_ssim3d_workspace_bytes(1, 1, 8, 8, 8, 11)
    assert call(out_map=None, mean=m, nbytes=C.c_size_t(need - 1)) == -2 and b"workspace" in L.cvx_last_error()
    assert call(out_map=None, slices=m, nbytes=C.c_size_t(0)) == -2
    assert call(out_map=None, mean=m, wsp=None) == -2
    # refusals come before the workspace is looked at
    assert call(win=4, out_map=None, mean=m, nbytes=C.c_size_t(0)) == -1 and call(win=13, out_map=None, mean=m, nbytes=C.c_size_t(0)) == -4


def test_workspace_query(L):
    q = L.cvx_ssim3d_workspace_bytes
    assert q(1, 1, 160, 192, 224, 11) > 0 and q(1, 1, 1, 1, 1, 1) > 0 and q(64, 1, 40, 40, 40, 11) < (1 << 22)
    for ext in ((5, 4, 3), (40, 40, 40), (33, 17, 65), (160, 192, 224)):
        last = 0
        for nc in (1, 2, 3, 5, 7, 8, 16, 63, 64, 65, 256, 1000):               # monotone in n * c, and a function of the product only
            cur = q(nc, 1, *ext, 11)
            assert cur >= last > -1 and cur > 0, (ext, nc)
            assert q(1, nc, *ext, 11) == cur
            last = cur
        assert q(6, 1, *ext, 11) == q(2, 3, *ext, 11) == q(3, 2, *ext, 11)
    # refused arguments have no size
    assert q(1, 1, 8, 8, 8, 4) == 0 and b"odd" in L.cvx_last_error()
    assert q(1, 1, 8, 8, 8, 13) == 0 and q(0, 1, 8, 8, 8, 11) == 0 and q(1, 1, 8, -1, 8, 11) == 0


def test_no_cpu_path():
    from convexadam_amd import convexAdam_hyper_util as U
    from convexadam_amd import ssim
    assert U.ssim3D is ssim.ssim3D and U.ssim3D_map is ssim.ssim3D_map and U.registration_ssim is ssim.registration_ssim
    x = torch.zeros(1, 1, 8, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ssim.ssim3D(x, x)
    with pytest.raises(RuntimeError, match="no CPU"):
        ssim.ssim3D(x, x, size_average=False)
    with pytest.raises(RuntimeError, match="no CPU"):
        ssim.ssim3D_map(x, x, 7)
    with pytest.raises(RuntimeError, match="no CPU"):
        ssim.registration_ssim(x[0, 0], x[0, 0], torch.zeros(3, 8, 8, 8))


def test_window_builders_are_the_references():
    """gaussian / create_window_3D: the reference's operations (helper_functions.py:102-112), float32, normalised."""
    from convexadam_amd.ssim import create_window_3D, gaussian
    g = gaussian(11, 1.5)
    assert g.dtype == torch.float32 and g.shape == (11,) and abs(float(g.double().sum()) - 1.0) < 1e-6
    assert torch.equal(g, g.flip(0)) and float(g[5]) == float(g.max())
    w = create_window_3D(7, 3)
    g7 = gaussian(7, 1.5)
    assert w.shape == (3, 1, 7, 7, 7) and w.dtype == torch.float32 and w.is_contiguous()
    assert torch.equal(w[0], w[2])
    outer = g7.double().view(7, 1, 1) * g7.double().view(1, 7, 1) * g7.double().view(1, 1, 7)
    assert float((w[0, 0].double() - outer).abs().max()) < 1e-8


def test_python_tile_constant_matches_the_kernel():
    """tests/test_gpu_ssim.py takes the kernel's tile extents from convexadam_amd.ssim.TILE: it must say what csrc/ssim.hip is built with."""
    from convexadam_amd.ssim import TILE
    src = open(os.path.join(ROOT, "convexadam_amd", "csrc", "ssim.hip")).read()
    val = lambda name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, src).group(1))      # noqa: E731
    assert TILE == (val("SSIM_MIN_HCHUNK"), val("SSIM_TW"), val("SSIM_TD"))
