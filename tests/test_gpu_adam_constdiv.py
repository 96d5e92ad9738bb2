"""div_const in the exact Adam loop (cvx_common.h, csrc/constdiv.hip): k_warp_grad's six divisions by (n - 1) / 2 and adam_update's division
by sqrt(1 - beta2^step) as three operations where the host has proven the divisor and no lane of the wavefront holds a dividend outside
2^-76 <= |x| <= 2^76, the IEEE sequence otherwise.  Only instructions change, so U, G, P, m and v must equal the CPU oracle's bit for bit,
signs of zeros included, on every arm that runs the update (box tiles, marching kernel, k_box3x3), for bias corrections from 0.03 to
nearly 1, with dividends that leave the guard on a few lanes, and with every divisor forced to the IEEE path."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NITER, C = 3, 5
_REF = {}

# (13, 17, 60): every 12 x 16 x 56 tile ragged, divisors 6, 8, 29.5; (5, 3, 8): smaller than a tile; (14, 20, 132): three x tiles, rows beyond
# the marching kernel's 126 voxels
SHAPES = [(13, 17, 60), (5, 3, 8), (14, 20, 132)]
ARMS = {"tiles": dict(box_fwd_tile=2000, box_bwd_tile=2000), "tiles1000": dict(box_fwd_tile=1000, box_bwd_tile=1000),
        "march": dict(box_fwd_tile=0, box_bwd_tile=0), "box3x3": dict(box_tiled=1)}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _lib
    return _lib.lib()


def inputs(shape, kind):
    rng = np.random.default_rng(sum(shape) + 7)
    F2 = rng.random((C,) + shape, dtype=np.float32)
    M2 = rng.random((C,) + shape, dtype=np.float32)
    P0 = (0.7 * rng.standard_normal((3,) + shape)).astype(np.float32)
    m0 = (1e-3 * rng.standard_normal((3,) + shape)).astype(np.float32)
    v0 = (1e-6 * rng.random((3,) + shape, dtype=np.float32)).astype(np.float32)
    if kind == "outside_guard":
        # one spike of 2^90 in the H channel (one channel only: the trilinear weights are products of three coordinate differences and must
        # stay finite): U = box(box(box(P))) exceeds 2^76 on most of the 7^3 voxels around it, and the regulariser's gradient there squares
        # to +Inf in v (the root's own fallback); and a block of zeros around a spike of -2^-100: U below 2^-76, and exact zeros
        h, w, d = shape
        P0[0, h // 4, w // 4, d // 4] = np.float32(2.0 ** 90)
        P0[:, h // 2:, w // 2:, d // 2:] = 0
        P0[:, 3 * h // 4, 3 * w // 4, 3 * d // 4] = np.float32(-2.0 ** -100)
    return F2, M2, P0, m0, v0


def case(orc, shape, step0, kind="plain"):
    """Inputs of one control grid and the oracle's result from step0, computed once and shared."""
    key = (shape, step0, kind)
    if key not in _REF:
        F2, M2, P0, m0, v0 = inputs(shape, kind)
        _REF[key] = F2, M2, P0, m0, v0, orc.adam_run(F2, M2, P0, 1.25, NITER, m=m0, v=v0, step0=step0, want_grad=True)
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
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        assert same.all(), "%s differs: %d elements" % (name, int((~same).sum()))
        assert np.array_equal(np.signbit(a), np.signbit(b)), name


def run(L, shape, step0, F2, M2, P0, m0, v0, mode=0, **opts):
    """cvx_adam_run_mode_f32 (mode 0 = exact, + 32 = every ConstDiv with ok = 0) from step0 with the state P0, m0, v0."""
    from convexadam_amd import _lib
    from convexadam_amd import convex_adam_utils as U
    h, w, d = shape
    P, m, v = dev(P0).clone(), dev(m0).clone(), dev(v0).clone()
    Ud, G = torch.zeros_like(P), torch.zeros_like(P)
    F2d, M2d = dev(F2), dev(M2)
    bh, bw, bd = U._base_tables(h, w, d, DEV)
    nws = L.cvx_adam_workspace_bytes(C, h, w, d)
    ws = _lib.workspace(nws, torch.device(DEV))
    with options(L, **opts):
        _lib.check(L.cvx_adam_run_mode_f32(_lib.ptr(F2d), _lib.ptr(M2d), C, h, w, d, _lib.ptr(P), _lib.ptr(m), _lib.ptr(v), 1.25, NITER, step0, 12.0,
                                           _lib.ptr(bh), _lib.ptr(bw), _lib.ptr(bd), _lib.ptr(Ud), _lib.ptr(G), None, 0, None, None, mode,
                                           _lib.ptr(ws), nws, _lib.stream_ptr(torch.device(DEV))))
        torch.cuda.synchronize()
    return (("U", Ud), ("G", G), ("P", P), ("m", m), ("v", v))


def proven(L, d):
    import ctypes as C_
    r, ok = C_.c_float(), C_.c_int(-1)
    assert L.cvx_const_div_make(C_.c_float(d), 1, C_.byref(r), C_.byref(ok)) == 0
    return ok.value == 1


def cases():
    for shape in SHAPES:
        for step0 in (0, 500, 5000):
            for arm in ARMS:
                if arm == "march" and shape[2] > 126:
                    continue                                   # (no marching kernel for such rows: the plan takes k_box3x3, the next arm)
                if arm == "tiles1000" and step0 != 0:
                    continue
                yield pytest.param(shape, step0, arm, id="%dx%dx%d-step%d-%s" % (shape + (step0, arm)))


@pytest.mark.parametrize("shape,step0,arm", list(cases()))
def test_every_arm_equals_the_oracle(L, orc, shape, step0, arm):
    F2, M2, P0, m0, v0, r = case(orc, shape, step0)
    check(run(L, shape, step0, F2, M2, P0, m0, v0, **ARMS[arm]), r)
    # ... and it was the three-operation path that ran: the grid's divisors and the steps' bias corrections all qualify
    assert all(proven(L, (n - 1) / 2.0) for n in shape)
    assert all(proven(L, float(np.float32(math.sqrt(1.0 - math.pow(0.999, float(step0 + i + 1)))))) for i in range(NITER))


@pytest.mark.parametrize("arm", ["tiles", "march", "box3x3"])
def test_lanes_outside_the_guard_take_their_wavefront_to_the_ieee_path(L, orc, arm):
    shape = (13, 17, 60)
    F2, M2, P0, m0, v0, r = case(orc, shape, 0, "outside_guard")
    U0 = orc.box_zero(orc.box_zero(orc.box_zero(P0)))                       # what the first iteration's warp kernel divides
    big, tiny = np.abs(U0) > 2.0 ** 76, (U0 != 0) & (np.abs(U0) < 2.0 ** -76)
    assert 0 < big.mean() < 0.02 and tiny.any() and (U0 == 0).any() and np.isposinf(r["v"]).any() and not np.isnan(r["P"]).any()
    assert 0 < (np.abs(r["U"]) > 2.0 ** 76).mean() < 0.02                   # ... and the last one's
    check(run(L, shape, 0, F2, M2, P0, m0, v0, **ARMS[arm]), r)


@pytest.mark.parametrize("arm", ["tiles", "march", "box3x3"])
def test_unproven_divisors_keep_the_ieee_division(L, orc, arm):
    """No grid has (n - 1) / 2 equal to a divisor that fails (tests/test_constdiv.py: none fails below 2^49), so ok = 0 is forced through the
    entry point's test-only mode bit."""
    shape = (13, 17, 60)
    F2, M2, P0, m0, v0, r = case(orc, shape, 500)
    check(run(L, shape, 500, F2, M2, P0, m0, v0, mode=32, **ARMS[arm]), r)


def test_whole_pair_equals_the_oracle(orc):
    """40 x 36 x 44, the smallest pair of the pipeline tests, four Adam iterations on its 20 x 18 x 22 control grid."""
    from convexadam_amd import convex_adam_MIND as M
    from convexadam_amd.phantom import phantom
    shape = (40, 36, 44)
    fix = phantom(shape, 1, 10)
    mov = torch.roll(phantom(shape, 1, 11), (3, -2, 1), (0, 1, 2))
    kw = dict(mind_r=1, mind_d=2, lambda_weight=1.25, grid_sp=4, disp_hw=3, selected_niter=4, grid_sp_adam=2, ic=True)
    out = M.convex_adam_pt(fix, mov, dtype=torch.float32, device=torch.device(DEV), **kw)
    assert np.array_equal(out, orc.convex_adam_pipeline(fix.numpy(), mov.numpy(), **kw))
