"""The entry points of include/convexadam_soft.h between fences (run on the MI355X box with `-m gpu`), with the helpers of tests/fences.py
as they are:

  check_fences       each operand between two moats of at least 64 KiB; plain allocations, NaN (loud) input moats, zero (quiet) input moats;
                     moats intact, outputs byte-identical across the three runs, inputs unchanged.  The workspace is a scratch operand: it
                     starts as stale bytes (0x3C plain, 0xA5 fenced) in every run, never zeroed; the counter is an output that the call
                     itself has to reset.
  check_side_stream  the same call on a fresh stream behind a bounded delay, inputs arriving late on that stream: the counter's reset and
                     both kernels must be enqueued behind the delay.
  check_unaligned    every operand one element behind the 256-byte boundary, all at once and each alone: the header grants no refusal for
                     that (elements stay aligned to their size), so the call runs with the same bits.

Every entry of the volume and of the field is read and nothing else, so a read outside an operand would meet a NaN, and a NaN reaches all
twelve outputs of its cell.  The plain run is then compared with the restatement.  The last test reads SOFT_SIGNATURES: every launching
name is a row here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softstats_restatement as R  # noqa: E402
from fences import IN, OUT, SCRATCH, Delay, check_fences, check_side_stream, check_unaligned, plain_run  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = []
NOT_LAUNCHING = {"cvx_soft_stats_workspace_bytes": "a size query: it takes no pointer and launches nothing (tests/test_softstats_abi.py checks its values)"}


def row(entry, case):
    def deco(build):
        ROWS.append((entry, case, build))
        return build
    return deco


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _soft
    return _soft.lib()


@pytest.fixture(scope="module")
def delay(L):
    return Delay(DEV)


def p(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


for grid, hw in (((3, 5, 7), 2), ((2, 3, 67), 1)):
    for half in (False, True):
        for with_field in (True, False):
            def build_stats(L, grid=grid, hw=hw, half=half, with_field=with_field):
                ssd = R.random_volume(hw, grid, 500 + hw, half)
                field = R.random_field(hw, grid, 500 + hw) if with_field else None
                beta, coupling = R.beta_for(half), (1.0 if with_field else 0.0)
                nws = L.cvx_soft_stats_workspace_bytes(*grid, hw)
                ops = {"ssd": IN(torch.from_numpy(ssd).to(DEV)), "out": OUT((12,) + grid, torch.float32), "stats": OUT((1,), torch.int64),
                       "ws": SCRATCH(nws)}
                if with_field:
                    ops["field"] = IN(torch.from_numpy(field).to(DEV))

                def call(t):
                    return L.cvx_soft_stats_f32(p(t["ssd"]), int(half), p(t["field"]) if with_field else None, coupling, beta, *grid, hw, p(t["out"]),
                                                p(t["stats"]), p(t["ws"]), nws, stream())

                def verify(t):
                    want, bad = R.soft_stats(ssd, hw, beta, field, coupling)
                    assert int(t["stats"].item()) == bad == 0
                    assert same_bits(t["out"].cpu().numpy(), want), "differs from the restatement"
                return ops, call, verify
            row("cvx_soft_stats_f32", "%s-hw%d-%s-%s" % ("x".join(map(str, grid)), hw, "f16" if half else "f32", "field" if with_field else "null"))(build_stats)


@pytest.mark.parametrize("r", ROWS, ids=["%s-%s" % (r[0][4:], r[1]) for r in ROWS])
def test_fenced(L, delay, r):
    entry, _, build = r
    operands, call, verify = build(L)
    plain = check_fences(operands, call, DEV)
    for k, op in operands.items():                       # the plain run holds no NaN: one in the loud run would come from a moat
        if op.kind == "out" and op.dtype.is_floating_point:
            assert not bool(torch.isnan(plain[k]).any()), "the plain run's %r holds a NaN: the inputs of this row are badly chosen" % k
    verify(plain)
    ref = plain_run(operands, call, DEV)
    for k, op in operands.items():
        if op.kind == "out":
            assert torch.equal(ref[0][k].view(torch.uint8), plain[k].view(torch.uint8)), "two plain runs differ in %r" % k
    # on a side stream, behind a delay
    _, armed = check_side_stream(operands, call, DEV, delay, reference=ref)
    if not armed:                                        # the host was held up while it enqueued: once more behind the longest delay
        _, armed = check_side_stream(operands, call, DEV, delay, reference=ref, delay_ms=delay.cap_ms)
    assert armed, "side-stream run: the call returned to the host only after the delay had drained"
    # at unaligned addresses: all operands at once, then each alone (the counter moves by its own 8 bytes)
    movable = [k for k, op in operands.items() if op.kind != "scratch"]
    assert check_unaligned(operands, call, DEV, movable, reference=ref)[1] == "ran"
    for k in movable:
        assert check_unaligned(operands, call, DEV, [k], reference=ref)[1] == "ran"


def test_every_soft_export_is_fenced():
    from convexadam_amd._soft import SOFT_SIGNATURES
    rows = {r[0] for r in ROWS}
    assert rows | set(NOT_LAUNCHING) == set(SOFT_SIGNATURES) and not rows & set(NOT_LAUNCHING), \
        "exported without a fence row or a written reason: %s" % sorted(set(SOFT_SIGNATURES) - rows - set(NOT_LAUNCHING))
    assert all(isinstance(v, str) and len(v) > 20 for v in NOT_LAUNCHING.values())
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS), "duplicate row ids"
