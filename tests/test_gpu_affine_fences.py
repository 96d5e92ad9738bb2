"""The entry points of include/convexadam_affine.h between fences (run on the MI355X box with `-m gpu`), with the helpers of tests/fences.py
as they are:

  check_fences       each operand between two moats of at least 64 KiB; plain allocations, NaN (loud) input moats, zero (quiet) input moats;
                     moats intact, outputs byte-identical across the three runs, inputs unchanged.  The workspace of the fit is a scratch
                     operand: it starts as stale bytes (0x3C plain, 0xA5 fenced) in every run, never zeroed.
  check_side_stream  the same call on a fresh stream behind a bounded delay, inputs arriving late on that stream.  cvx_affine_lts_f32
                     synchronises its stream once to read the fit's status, so for it the check holds up to that synchronisation (the
                     kernel is its only launch and comes before it); cvx_affine_field_f64 must be enqueued behind the delay as a whole.
  check_unaligned    every operand one element behind the 256-byte boundary, all at once and each alone: the header grants no refusal for
                     that (elements stay aligned to their size), so the call runs with the same bits.

The point rows of the ld = 7 cases carry NaN in their unused columns, the fields are read at every voxel and nowhere else, so a read
outside an operand would meet a NaN.  The plain run is then compared with the restatement.  The last test reads AFFINE_SIGNATURES: every
launching name is a row here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as R  # noqa: E402
from fences import IN, OUT, SCRATCH, Delay, check_fences, check_side_stream, check_unaligned, plain_run  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = []
SYNCHRONISES = {"cvx_affine_lts_f32"}
NOT_LAUNCHING = {"cvx_affine_lts_workspace_bytes": "a size query: it takes no pointer and launches nothing (tests/test_affine_abi.py checks its values)"}


def row(entry, case):
    def deco(build):
        ROWS.append((entry, case, build))
        return build
    return deco


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _affine
    return _affine.lib()


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


for n, ld, iters, normal, mask in ((65, 4, 3, 0, True), (65, 7, 3, 1, True), (2049, 7, 4, 0, True), (2049, 4, 4, 1, False), (1024, 3, 1, 0, True)):
    def build_lts(L, n=n, ld=ld, iters=iters, normal=normal, mask=mask):
        f, m, _ = R.points(n, seed=8, outliers=0.25, ld=ld)
        nws = L.cvx_affine_lts_workspace_bytes(n)
        ops = {"f": IN(torch.from_numpy(np.array(f)).to(DEV)), "m": IN(torch.from_numpy(np.array(m)).to(DEV)), "X": OUT((4, 4), torch.float32),
               "ws": SCRATCH(nws)}
        if mask:
            ops["inliers"] = OUT((n,), torch.uint8)

        def call(t):
            return L.cvx_affine_lts_f32(p(t["f"]), ld, p(t["m"]), ld, n, iters, normal, p(t["X"]), p(t["inliers"]) if mask else None, p(t["ws"]), nws,
                                        stream())

        def verify(t):
            X = t["X"].cpu().numpy()
            inl = t["inliers"] if mask else torch.empty(n, dtype=torch.uint8, device=DEV)
            if not mask:                                 # the set is not returned: the same call with a mask gives it, and the same X
                X2 = torch.empty_like(t["X"])
                assert L.cvx_affine_lts_f32(p(t["f"]), ld, p(t["m"]), ld, n, iters, normal, p(X2), p(inl), p(t["ws"]), nws, stream()) == 0
                assert same_bits(X2.cpu().numpy(), X)
            sel = inl.cpu().numpy().astype(bool)
            assert int(sel.sum()) == (n if iters == 1 else n // 2)
            want, cond = R.fit64(f[sel], m[sel], normal)
            assert cond < 1e6 and (np.abs(X - want) <= R.x_bound(want, cond)).all()
        return ops, call, verify
    row("cvx_affine_lts_f32", "n%d-ld%d-it%d-normal%d-%s" % (n, ld, iters, normal, "mask" if mask else "null"))(build_lts)

for shape in ((7, 1, 9), (5, 4, 131)):
    for planar in (0, 1):
        for with_u in (True, False):
            def build_field(L, shape=shape, planar=planar, with_u=with_u):
                V = int(np.prod(shape))
                u = R.smooth_field(shape).astype(np.float32)
                # float in, double out in the other layout: the two strides and the two element sizes differ
                ops = {"theta": IN(torch.from_numpy(R.THETA.copy()).to(DEV)), "out": OUT(((3,) + shape) if not planar else (shape + (3,)), torch.float64)}
                if with_u:
                    ops["u"] = IN(torch.from_numpy(R.layouts(u, np.float32, planar)).to(DEV))
                us, os_ = ((V, 1) if planar else (1, 3)), ((1, 3) if planar else (V, 1))

                def call(t):
                    ua = (p(t["u"]), 0) + us if with_u else (None, 0, 0, 0)
                    return L.cvx_affine_field_f64(p(t["theta"]), *shape, *ua, p(t["out"]), 1, *os_, stream())

                def verify(t):
                    o = t["out"].cpu().numpy()
                    got = o if planar else np.moveaxis(o, 0, -1)
                    assert same_bits(got, R.field(R.THETA, shape, u if with_u else None)), "differs from the restatement"
                return ops, call, verify
            row("cvx_affine_field_f64", "%s-%s-%s" % ("x".join(map(str, shape)), "planar" if planar else "interleaved", "u" if with_u else "null"))(build_field)


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
    if entry not in SYNCHRONISES:
        if not armed:                                    # the host was held up while it enqueued: once more behind the longest delay
            _, armed = check_side_stream(operands, call, DEV, delay, reference=ref, delay_ms=delay.cap_ms)
        assert armed, "side-stream run: the call returned to the host only after the delay had drained"
    # at unaligned addresses: all operands at once, then each alone
    movable = [k for k, op in operands.items() if op.kind != "scratch"]
    assert check_unaligned(operands, call, DEV, movable, reference=ref)[1] == "ran"
    for k in movable:
        assert check_unaligned(operands, call, DEV, [k], reference=ref)[1] == "ran"


def test_every_affine_export_is_fenced():
    from convexadam_amd._affine import AFFINE_SIGNATURES
    rows = {r[0] for r in ROWS}
    assert rows | set(NOT_LAUNCHING) == set(AFFINE_SIGNATURES) and not rows & set(NOT_LAUNCHING), \
        "exported without a fence row or a written reason: %s" % sorted(set(AFFINE_SIGNATURES) - rows - set(NOT_LAUNCHING))
    assert all(isinstance(v, str) and len(v) > 20 for v in NOT_LAUNCHING.values())
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS), "duplicate row ids"
