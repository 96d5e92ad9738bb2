"""The coupled-convex stage under every outcome of its plan (coupled_plan, convex.hip), every assertion an equality of bytes
(run on the MI355X box with `-m gpu`).  The file pins behaviour: it passes against the library from before the plan existed as well.

  operators   cvx_coupled_convex_f32 / _f16 / _masked_f32 under the four option sets the stage reads, at v % 4 != 0 (5x6x7: the scalar
              kernels), v % 4 == 0 (4x6x8: the 16-byte kernels) and with 27 displacements (one chunk per box) = the oracle's coupled_convex
              on the values the kernels see (the half-rounded volume; ssd * mask)
  re-planning the same thread, inputs and workspace under default, no_prune, default, prune_stream_above = 0: a stage that kept any part of
              an earlier call's choices would run passes on counters and keys the other part did not prepare
  per call    a whole pair whose options arrive only through cvx_pair_params.ctx, in both directions against the thread's options: every
              part of the stage (set-up launch, plain argmin, correlation plan, the solves) must read the call's context
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp16_edge_cases as E  # noqa: E402
from test_gpu_fp16_edges import dev, host, option  # noqa: E402
from test_gpu_rigid_registration import check_masked, random_volume  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPTION_SETS = [("no_prune", 0), ("no_prune", 1), ("prune_stream_above", 0), ("prune_refine", 0)]       # (no_prune, 0) = the defaults
GEOMETRIES = [((5, 6, 7), 2), ((4, 6, 8), 2), ((5, 6, 7), 1)]
assert (5 * 6 * 7) % 4 != 0 and (4 * 6 * 8) % 4 == 0


def gid(v):
    return "%s=%d" % v if isinstance(v[0], str) else "%s-hw%d" % ("x".join(map(str, v[0])), v[1])


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _lib
    return _lib.lib()


_cases = {}


def case(orc, entry, shape, hw):
    """(volume, seed winners, cell mask or None, the oracle's field) of a case: computed once, read-only"""
    key = (entry, shape, hw)
    if key not in _cases:
        rng = np.random.default_rng(1000 * hw + shape[2])
        vol = random_volume(rng, hw, shape)
        mask = (rng.random(shape) < 0.6).astype(np.uint8) if entry == "masked" else None
        seen = E.widen(vol) if entry == "f16" else vol
        am = np.argmin(seen, 0).astype(np.int64)                        # (masked: of the UNMASKED volume, as the script passes it)
        want = orc.coupled_convex(seen if mask is None else seen * mask[None].astype(np.float32), am, orc.disp_mesh(hw), hw)
        for a in (vol, am, want) + (() if mask is None else (mask,)):
            a.setflags(write=False)
        _cases[key] = (vol, am, mask, want)
    return _cases[key]


@pytest.mark.parametrize("opt", OPTION_SETS, ids=gid)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=gid)
@pytest.mark.parametrize("entry", ["f32", "f16", "masked"])
def test_operator_equals_oracle_under_every_plan(L, orc, entry, geo, opt):
    from convexadam_amd import convex_adam_utils as U
    shape, hw = geo
    vol, am, mask, want = case(orc, entry, shape, hw)
    with option(L, *opt):
        if entry == "masked":
            got = check_masked(orc, np.array(vol), hw, np.array(mask), np.array(am))      # (copies: the helper wraps them without one; it asserts against the oracle on ssd * mask itself)
        else:
            vd = dev(E.to_half(vol)) if entry == "f16" else dev(vol)
            assert vd.dtype == (torch.float16 if entry == "f16" else torch.float32)
            got = host(U.coupled_convex(vd, dev(am), dev(orc.disp_mesh(hw))[:, :, None], 1, shape))[0]
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("geo", GEOMETRIES[:2], ids=gid)
def test_options_changed_between_calls_on_one_workspace(L, orc, geo):
    from convexadam_amd import _lib
    (h, w, d), hw = geo
    vol, am, _, want = case(orc, "f32", (h, w, d), hw)
    vd, amd, mesh = dev(vol), dev(am), dev(orc.disp_mesh(hw))
    n = L.cvx_coupled_convex_workspace_bytes(h, w, d, hw)
    ws = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)          # filled once, never again
    outs = []
    for opt in (("no_prune", 0), ("no_prune", 1), ("no_prune", 0), ("prune_stream_above", 0)):
        out = torch.full((3, h, w, d), 7.0, device=DEV)
        with option(L, *opt):
            assert L.cvx_coupled_convex_f32(_lib.ptr(vd), _lib.ptr(amd), _lib.ptr(mesh), h, w, d, hw, _lib.ptr(out), _lib.ptr(ws), n, _lib.stream_ptr(DEV)) == 0
        outs.append(host(out).tobytes())
    assert outs[1] == outs[0] and outs[2] == outs[0] and outs[3] == outs[0]
    assert outs[0] == want.tobytes()


def test_options_carried_by_the_call(L):
    from convexadam_amd import _lib
    from convexadam_amd.context import Context
    H, W, D = 24, 28, 20
    gen = torch.Generator().manual_seed(11)
    fix, mov = torch.rand((H, W, D), generator=gen).to(DEV), torch.rand((H, W, D), generator=gen).to(DEV)

    def pair(ctx):
        pp = _lib.PairParams(H, W, D, 1, 2, 0.0, 2, 2, 3, 0, 2, 1, 0, 1.0, 0, 2, 0, 0, 0)       # ic = 1, lambda_weight = 0: the convex stage decides the field
        if ctx is not None:
            pp.ctx = ctx.handle
        n = L.cvx_register_pair_workspace_bytes(C.byref(pp))
        assert n > 0
        ws, out = torch.empty(n, dtype=torch.uint8, device=DEV), torch.full((3, H, W, D), 7.0, device=DEV)
        rc = L.cvx_register_pair_f32(_lib.ptr(fix), _lib.ptr(mov), None, None, C.byref(pp), _lib.ptr(out), None, _lib.ptr(ws), n, _lib.stream_ptr(DEV))
        assert rc == 0, L.cvx_last_error()
        return host(out).tobytes()

    assert L.cvx_get_option(b"no_prune") == 0
    a = pair(None)
    b = pair(Context(no_prune=1, corr_cert=0))                          # the thread's options are the defaults
    with option(L, "no_prune", 1):
        c = pair(Context(no_prune=0))
    assert b == a and c == a
