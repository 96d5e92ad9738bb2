"""Write-through stores of the Adam loop (option adam_wt; helpers in cvx_common.h), bit for bit against the CPU oracle.  One bit per kernel:
  1 = U of the forward box tiles, 2 = gU of k_warp_grad, 4 = P, m, v and the gradient copy of the adjoint + Adam box tiles,
  8 = the fast modes' kernels (k_warp_grad_fast, k_box3_fast).
Only the cache policy of a store changes, so U, G, P, m and v must equal the oracle's with every mask, signs of zeros included; the arms of
the plan that the option does not name (marching kernels, sweep smoothers) must not change either."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCUMENTED_DEFAULT = 1          # include/convexadam_hip.h, "adam_wt"
NITER, C = 3, 5
_REF = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _lib
    return _lib.lib()


def case(orc, shape, mode="exact"):
    """Inputs of one control grid and the oracle's result for `mode`, computed once and shared."""
    key = (shape, mode)
    if key not in _REF:
        rng = np.random.default_rng(sum(shape))
        F2 = rng.random((C,) + shape, dtype=np.float32)
        M2 = rng.random((C,) + shape, dtype=np.float32)
        P0 = (0.7 * rng.standard_normal((3,) + shape)).astype(np.float32)
        _REF[key] = F2, M2, P0, orc.adam_run(F2, M2, P0, 1.25, NITER, want_grad=True, mode=mode)
    return _REF[key]


class options:
    """Sets options of the default context and restores them."""

    def __init__(self, L, **kw):
        self.L, self.kw = L, kw

    def __enter__(self):
        self.old = {n: self.L.cvx_get_option(n.encode()) for n in self.kw}
        for n, v in self.kw.items():
            assert self.L.cvx_set_option(n.encode(), v) == 0, n

    def __exit__(self, *exc):
        for n, v in self.old.items():
            self.L.cvx_set_option(n.encode(), v)


def check(got, r):
    for name, t in got:
        a, b = host(t).reshape(r[name].shape), r[name]
        assert np.array_equal(a, b), "%s differs: %d elements, max |diff| %g" % (name, int((a != b).sum()), float(np.abs(a - b).max()))
        assert np.array_equal(np.signbit(a), np.signbit(b)), name


def run_and_check(L, orc, shape, mode="exact", **opts):
    from convexadam_amd import convex_adam_utils as U
    F2, M2, P0, r = case(orc, shape, mode)
    with options(L, **opts):
        Ud, st = U.adam_run(dev(F2)[None], dev(M2)[None], dev(P0)[None], 1.25, NITER, return_state=True, mode=mode)
        torch.cuda.synchronize()
    check((("U", Ud), ("G", st["G"]), ("P", st["P"]), ("m", st["m"]), ("v", st["v"])), r)


# (13, 17, 60): one voxel past a 12 x 16 tile in z and y and four past 56 in x -- every tile ragged, every store guard exercised;
# (5, 3, 8): smaller than one tile; (14, 20, 132): rows beyond the marching kernel's 126 voxels, three x tiles
@pytest.mark.parametrize("wt", [0, 1, 2, 4, 7])
@pytest.mark.parametrize("variant", [2000, 1000])
@pytest.mark.parametrize("shape", [(13, 17, 60), (5, 3, 8), (14, 20, 132)])
def test_exact_mode_on_tiles(L, orc, shape, variant, wt):
    run_and_check(L, orc, shape, box_fwd_tile=variant, box_bwd_tile=variant, adam_wt=wt)


def test_mixed_plans_misaligned_gradient_copy(L, orc):
    """grad_out 4 bytes off a 16-byte boundary: the last iteration's adjoint leaves the tiles (and its warp kernel the pre-division) while
    the forward pass stays on them -- write-through and plain kernels in one run, adam_wt = 7."""
    from convexadam_amd import _lib
    from convexadam_amd import convex_adam_utils as U
    shape = (5, 3, 8)
    h, w, d = shape
    F2, M2, P0, r = case(orc, shape)
    n = 3 * h * w * d

    def buf(offset):                                               # n floats, `offset` floats behind a 16-byte boundary
        t = torch.zeros(n + 4, device=DEV)[offset:offset + n]
        assert t.data_ptr() % 16 == 4 * offset
        return t
    P, m, v, G, Ud = buf(0), buf(0), buf(0), buf(1), buf(0)
    P.copy_(dev(P0).reshape(-1))
    F2d, M2d = dev(F2), dev(M2)
    bh, bw, bd = U._base_tables(h, w, d, DEV)
    nws = L.cvx_adam_workspace_bytes(C, h, w, d)
    ws = _lib.workspace(nws, torch.device(DEV))
    a = (_lib.ptr(F2d), _lib.ptr(M2d), C, h, w, d, _lib.ptr(P), _lib.ptr(m), _lib.ptr(v), 1.25, NITER, 0, 12.0, _lib.ptr(bh),
         _lib.ptr(bw), _lib.ptr(bd), _lib.ptr(Ud), _lib.ptr(G), None, 0, None, _lib.ptr(ws), nws, _lib.stream_ptr(torch.device(DEV)))
    with options(L, box_fwd_tile=2000, box_bwd_tile=2000, adam_wt=7):
        _lib.check(L.cvx_adam_run_f32(*a))
        torch.cuda.synchronize()
    check((("U", Ud), ("G", G), ("P", P), ("m", m), ("v", v)), r)


def test_fallback_arms_ignore_the_option(L, orc):
    """No tiles in either direction (marching kernels): adam_wt = 7 reaches only the warp kernel."""
    run_and_check(L, orc, (6, 9, 32), box_fwd_tile=0, box_bwd_tile=0, adam_wt=7)


@pytest.mark.parametrize("wt", [0, 8])
@pytest.mark.parametrize("shape", [(6, 9, 32), (25, 17, 60)])
def test_fast_mode(L, orc, shape, wt):
    run_and_check(L, orc, shape, mode="fast", adam_wt=wt)


def _pair(L, shape, **opts):
    from convexadam_amd import convex_adam_MIND as M
    from convexadam_amd.phantom import phantom
    fix = phantom(shape, 1, 10).to(DEV)
    mov = torch.roll(phantom(shape, 1, 11), (2, -1, 1), (0, 1, 2)).to(DEV)
    kw = dict(mind_r=1, mind_d=2, lambda_weight=1.25, grid_sp=4, disp_hw=3, selected_niter=4, grid_sp_adam=2, ic=True)
    with options(L, **opts):
        out = M.register_pair_device(fix, mov, **kw).clone()
        torch.cuda.synchronize()
    return out


def test_whole_pair_default_equals_plain_stores(L):
    """40 x 36 x 44, the smallest pair of the pipeline tests: the shipped default and adam_wt = 0 give the same field."""
    shape = (40, 36, 44)
    assert torch.equal(_pair(L, shape, adam_wt=L.cvx_get_option(b"adam_wt")), _pair(L, shape, adam_wt=0))


def test_whole_pair_on_tiles_every_bit(L):
    """40 x 36 x 48: a control grid of whole quads per row (20 x 18 x 24), tiles asked for -- every exact-mode bit against none."""
    shape = (40, 36, 48)
    tiles = dict(box_fwd_tile=2000, box_bwd_tile=2000)
    assert torch.equal(_pair(L, shape, adam_wt=7, **tiles), _pair(L, shape, adam_wt=0, **tiles))


_CHILD = "from convexadam_amd import _lib; print(_lib.lib().cvx_get_option(b'adam_wt'))"


def _child(env):
    return int(subprocess.run([sys.executable, "-c", _CHILD], env=env, stdout=subprocess.PIPE, text=True, check=True).stdout.strip())


def test_option_default_and_environment(L):
    """The default context starts from the documented default, reads CVX_ADAM_WT, and the option round-trips through cvx_set_option."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CVX_")}
    env["PYTHONPATH"] = ROOT
    assert _child(env) == DOCUMENTED_DEFAULT
    assert _child(dict(env, CVX_ADAM_WT="13")) == 13
    old = L.cvx_get_option(b"adam_wt")
    try:
        assert L.cvx_set_option(b"adam_wt", 5) == 0 and L.cvx_get_option(b"adam_wt") == 5
    finally:
        L.cvx_set_option(b"adam_wt", old)
