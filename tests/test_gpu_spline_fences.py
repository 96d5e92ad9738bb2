"""The entry points of include/convexadam_spline.h between fences (run on the MI355X box with `-m gpu`), with the helpers of tests/fences.py as
they are:

  check_fences       each operand between two moats of at least 64 KiB; plain allocations, NaN (loud) input moats, zero (quiet) input moats;
                     moats intact, outputs byte-identical across the three runs, inputs unchanged.  The in-place prefilter's volume is an
                     in/out operand: its moats are guarded like an output's.
  check_side_stream  the same call on a fresh stream behind a bounded delay, inputs arriving late on that stream: the three passes of the
                     prefilter and both gathers must be enqueued behind the delay.
  check_unaligned    every operand one element behind the 256-byte boundary, all at once and each alone: the header grants no refusal for
                     that (elements stay aligned to their size), so the call runs with the same bits.

A read outside the samples would put a NaN into a line's recursion and from there into every coefficient of the line; a read outside the
coefficients reaches the 64 taps (the mirrored indices are what keeps them inside); a read outside the field moves the sampling point.  The
plain run is then compared with the restatement.  Shapes (3, 5, 131) -- contiguous lines of four staged chunks and a rest, 15 lines in a
tile of 64 -- and (5, 6, 7).  The last test reads SPLINE_SIGNATURES: every name is a row here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spline_restatement as R  # noqa: E402
from fences import IN, INOUT, OUT, Delay, check_fences, check_side_stream, check_unaligned, plain_run  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = []
SHAPES = [(3, 5, 131), (5, 6, 7)]


def row(entry, case):
    def deco(build):
        ROWS.append((entry, case, build))
        return build
    return deco


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _spline
    return _spline.lib()


@pytest.fixture(scope="module")
def delay(L):
    return Delay(DEV)


def p(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def same(t, want):
    return np.array_equal(t.cpu().numpy(), want)


for shape in SHAPES:
    tag = "x".join(map(str, shape))
    for dt in (np.float32, np.float64):
        def build_prefilter(L, shape=shape, dt=dt):
            vol = R.volume(shape, 31, dt)
            ops = dict(src=IN(dev(vol)), coef=OUT(shape, torch.float64))

            def call(t):
                return L.cvx_spline_prefilter_f64(p(t["src"]), int(dt == np.float64), *shape, p(t["coef"]), stream())

            def verify(t):
                assert same(t["coef"], R.prefilter(vol)), "differs from the restatement"
            return ops, call, verify
        row("cvx_spline_prefilter_f64", "%s-%s" % (tag, np.dtype(dt).name))(build_prefilter)

    def build_in_place(L, shape=shape):
        vol = R.volume(shape, 32)
        ops = dict(vol=INOUT(dev(vol)))

        def call(t):
            return L.cvx_spline_prefilter_f64(p(t["vol"]), 1, *shape, p(t["vol"]), stream())

        def verify(t):
            assert same(t["vol"], R.prefilter(vol)), "differs from the restatement"
        return ops, call, verify
    row("cvx_spline_prefilter_f64", "%s-in-place" % tag)(build_in_place)

    for layout, dt in (("interleaved", np.float32), ("planar", np.float64)):
        def build_map(L, shape=shape, layout=layout, dt=dt):
            coef = R.prefilter(R.volume(shape, 33))
            field = R.field_through(shape, R.coordinates(shape, 33), 0, dt)
            V = int(np.prod(shape))
            cs, vs = (1, 3) if layout == "interleaved" else (V, 1)
            ops = dict(coef=IN(dev(coef)), field=IN(dev(field if layout == "interleaved" else np.moveaxis(field, -1, 0))), out=OUT(shape, torch.float64))

            def call(t):
                return L.cvx_map_coordinates_cubic_f64(p(t["coef"]), p(t["field"]), int(dt == np.float64), cs, vs, *shape, p(t["out"]), stream())

            def verify(t):
                want = R.map_cubic(coef, R.warp_coordinates(shape, field)).reshape(shape)
                assert (want != 0.0).sum() > V // 2 and (want == 0.0).any()
                assert same(t["out"], want), "differs from the restatement"
            return ops, call, verify
        row("cvx_map_coordinates_cubic_f64", "%s-%s-%s" % (tag, layout, np.dtype(dt).name))(build_map)

    for out_dt in (torch.float32, torch.float64):
        def build_resample(L, shape=shape, out_dt=out_dt):
            coef = R.prefilter(R.volume(shape, 34))
            out_shape = (shape[0] + 2, shape[1] + 1, shape[2] + 3)
            M = np.array([[0.9, 0.05, 0.0], [-0.04, 0.95, 0.1], [0.0, 0.08, 0.85]])
            tr = np.array([-0.7, 0.2, -0.45])
            m12 = (C.c_double * 12)(*M.reshape(-1).tolist(), *tr.tolist())
            ops = dict(coef=IN(dev(coef)), out=OUT(out_shape, out_dt))

            def call(t):
                return L.cvx_resample_cubic_f64(p(t["coef"]), *shape, p(t["out"]), int(out_dt == torch.float64), *out_shape, m12, -1.5, stream())

            def verify(t):
                want = R.itk_cubic(coef, R.index_grid(out_shape, M, tr), -1.5).reshape(out_shape)
                assert (want != -1.5).sum() > want.size // 4 and (want == -1.5).any()
                assert same(t["out"], want.astype(np.float64 if out_dt == torch.float64 else np.float32)), "differs from the restatement"
            return ops, call, verify
        row("cvx_resample_cubic_f64", "%s-%s" % (tag, str(out_dt).split(".")[-1]))(build_resample)


ENTRIES = sorted({r[0] for r in ROWS})


@pytest.mark.parametrize("entry", ENTRIES, ids=[e[4:] for e in ENTRIES])
def test_fenced(L, delay, entry):
    """every row of one entry point (shape, element types, layouts, in place); a failing row is named in the assertion"""
    for r in ROWS:
        if r[0] == entry:
            try:
                _fenced_row(L, delay, r)
            except AssertionError as e:
                raise AssertionError("row %s-%s: %s" % (r[0], r[1], e)) from e


def _fenced_row(L, delay, r):
    entry, _, build = r
    operands_, call, verify = build(L)
    plain = check_fences(operands_, call, DEV)
    verify(plain)
    ref = plain_run(operands_, call, DEV)
    for k, op in operands_.items():
        if op.kind in ("out", "inout"):
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


def test_every_spline_export_is_fenced():
    from convexadam_amd._spline import SPLINE_SIGNATURES
    rows = {r[0] for r in ROWS}
    assert rows == set(SPLINE_SIGNATURES), "exported without a fence row: %s" % sorted(set(SPLINE_SIGNATURES) - rows)
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS) == 14, "duplicate row ids"
