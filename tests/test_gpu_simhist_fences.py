"""The entry points of include/convexadam_sim.h between fences (run on the MI355X box with `-m gpu`), with the helpers of tests/fences.py as
they are:

  check_fences       each operand between two moats of at least 64 KiB; plain allocations, NaN (loud) input moats, zero (quiet) input moats;
                     moats intact, outputs byte-identical across the three runs, inputs unchanged.  The histogram, the counters and the
                     range are outputs that the call itself has to reset: they start as stale bytes (0x3C plain, 0xA5 fenced) in every run.
  check_side_stream  the same call on a fresh stream behind a bounded delay, inputs arriving late on that stream: the resets and every
                     kernel must be enqueued behind the delay.
  check_unaligned    every operand one element behind the 256-byte boundary, all at once and each alone: the header grants no refusal for
                     that (elements stay aligned to their size), so the call runs with the same bits.

A read outside the fixed image, the field or the range would meet a NaN, and a NaN voxel leaves the histogram for the non-finite counter; a
read outside the moving image reaches the taps.  The mask is an integer input: its loud moat value is 1, a valid entry that differs from
the quiet moat's 0, so a read outside it flips a voxel between kept and masked.  The plain run is then compared with the restatement.  The last test reads SIM_SIGNATURES:
every launching name is a row here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simhist_restatement as R  # noqa: E402
from fences import IN, OUT, Delay, check_fences, check_side_stream, check_unaligned, plain_run  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = []
NOT_LAUNCHING = {"cvx_joint_hist_lds_bytes": "a query of two integers: it takes no pointer and launches nothing (tests/test_simhist_abi.py checks its values)"}


def row(entry, case):
    def deco(build):
        ROWS.append((entry, case, build))
        return build
    return deco


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _sim
    return _sim.lib()


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


def operands(c):
    ops = {"fixed": IN(torch.from_numpy(c["fixed"]).to(DEV)), "moving": IN(torch.from_numpy(c["moving"]).to(DEV))}
    if c["field"] is not None:
        ops["field"] = IN(torch.from_numpy(c["field"]).to(DEV))
    if c["mask"] is not None:
        ops["mask"] = IN(torch.from_numpy(c["mask"]).to(DEV), loud=1)
    return ops


def field_args(c, t):
    if c["field"] is None:
        return (None, 0, 0, 0)
    V = c["fixed"].size
    planar = c["field"].shape == (3,) + c["fixed"].shape
    return (p(t["field"]), int(c["field"].dtype == np.float64), V if planar else 1, 1 if planar else 3)


# both entry points at both shapes, the field present (one layout and element type per shape, so that all four occur) and NULL, the mask
# present and NULL; the histogram on its LDS path, at the LDS limit and on the global path
for shape, fk in (((3, 5, 7), ("planar", "f64")), ((2, 3, 67), ("interleaved", "f32"))):
    for with_field in (True, False):
        for with_mask in (True, False):
            tag = "%s-%s-%s" % ("x".join(map(str, shape)), "-".join(fk) if with_field else "null", "mask" if with_mask else "nomask")

            def build_range(L, shape=shape, fk=fk, with_field=with_field, with_mask=with_mask):
                c = R.case(shape, None, with_mask, fk if with_field else None, 1, seed=21)
                ops = dict(operands(c), range=OUT((4,), torch.float32), stats=OUT((5,), torch.int64))

                def call(t):
                    return L.cvx_sim_range_f32(p(t["fixed"]), p(t["moving"]), *field_args(c, t), p(t["mask"]) if with_mask else None, *shape, 1,
                                               p(t["range"]), p(t["stats"]), stream())

                def verify(t):
                    want_r, want_s = R.value_range(c["fixed"], c["moving"], c["field"], c["mask"], True)
                    assert same_bits(t["range"].cpu().numpy(), want_r) and same_bits(t["stats"].cpu().numpy(), want_s), "differs from the restatement"
                return ops, call, verify
            row("cvx_sim_range_f32", tag)(build_range)

            for bins in ((32, 32), (128, 128), (129, 128)):
                def build_hist(L, shape=shape, fk=fk, with_field=with_field, with_mask=with_mask, bins=bins):
                    c = R.case(shape, None, with_mask, fk if with_field else None, 1, seed=22)
                    rng, _ = R.value_range(c["fixed"], c["moving"], c["field"], c["mask"], True)
                    assert np.isfinite(rng).all()
                    ops = dict(operands(c), range=IN(torch.from_numpy(rng).to(DEV)), hist=OUT(bins, torch.int64), stats=OUT((5,), torch.int64))

                    def call(t):
                        return L.cvx_joint_hist_f32(p(t["fixed"]), p(t["moving"]), *field_args(c, t), p(t["mask"]) if with_mask else None, *shape, *bins,
                                                    p(t["range"]), 1, p(t["hist"]), p(t["stats"]), stream())

                    def verify(t):
                        want_h, want_s = R.joint_hist(c["fixed"], c["moving"], bins, rng, c["field"], c["mask"], True)
                        assert want_s[R.KEPT] > 0
                        assert same_bits(t["hist"].cpu().numpy(), want_h) and same_bits(t["stats"].cpu().numpy(), want_s), "differs from the restatement"
                    return ops, call, verify
                row("cvx_joint_hist_f32", "%s-b%dx%d" % (tag, bins[0], bins[1]))(build_hist)


@pytest.mark.parametrize("r", ROWS, ids=["%s-%s" % (r[0][4:], r[1]) for r in ROWS])
def test_fenced(L, delay, r):
    entry, _, build = r
    operands_, call, verify = build(L)
    plain = check_fences(operands_, call, DEV)
    verify(plain)
    ref = plain_run(operands_, call, DEV)
    for k, op in operands_.items():
        if op.kind == "out":
            assert torch.equal(ref[0][k].view(torch.uint8), plain[k].view(torch.uint8)), "two plain runs differ in %r" % k
    # on a side stream, behind a delay
    _, armed = check_side_stream(operands_, call, DEV, delay, reference=ref)
    if not armed:                                        # the host was held up while it enqueued: once more behind the longest delay
        _, armed = check_side_stream(operands_, call, DEV, delay, reference=ref, delay_ms=delay.cap_ms)
    assert armed, "side-stream run: the call returned to the host only after the delay had drained"
    # at unaligned addresses: all operands at once, then each alone
    movable = list(operands_)
    assert check_unaligned(operands_, call, DEV, movable, reference=ref)[1] == "ran"
    for k in movable:
        assert check_unaligned(operands_, call, DEV, [k], reference=ref)[1] == "ran"


def test_every_sim_export_is_fenced():
    from convexadam_amd._sim import SIM_SIGNATURES
    rows = {r[0] for r in ROWS}
    assert rows | set(NOT_LAUNCHING) == set(SIM_SIGNATURES) and not rows & set(NOT_LAUNCHING), \
        "exported without a fence row or a written reason: %s" % sorted(set(SIM_SIGNATURES) - rows - set(NOT_LAUNCHING))
    assert all(isinstance(v, str) and len(v) > 20 for v in NOT_LAUNCHING.values())
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS), "duplicate row ids"
