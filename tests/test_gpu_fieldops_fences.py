"""Both entry points of include/convexadam_field.h between fences (run on the MI355X box with `-m gpu`).

tests/fences.py: each operand sits between two moats of at least 64 KiB; the call runs on plain allocations, fenced with NaN (loud) input
moats and fenced with zero (quiet) input moats; moats stay intact, outputs are byte-identical across the three runs, inputs unchanged.
The fields push most coordinates through the border clamp (tests/fieldops_restatement.py), so a tap that left the volume would read a moat.
Shapes 5 x 4 x 131 (a row length that is a multiple of nothing) and 7 x 9 x 11, both layouts, the optional outputs present and NULL.  The
plain run is then compared with the restatement.  The last test reads FIELD_SIGNATURES: every name is a row here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldops_restatement as R  # noqa: E402
from fences import IN, OUT, check_fences  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [("5x4x131", 2), ("7x9x11", 1)]           # index into the smooth set
ROWS = []


def row(entry, case):
    def deco(build):
        ROWS.append((entry, case, build))
        return build
    return deco


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _field
    return _field.lib()


def p(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def hwd3(t, planar):
    a = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.moveaxis(a, 0, -1)) if planar else a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def strides(shape, planar):
    return (shape[0] * shape[1] * shape[2], 1) if planar else (1, 3)


def fshape(shape, planar):
    return (3,) + tuple(shape) if planar else tuple(shape) + (3,)


for case, k in CASES:
    for planar in (0, 1):
        for optional in (True, False):
            def build_invert(L, k=k, planar=planar, optional=optional):
                u = R.smooth_set()[k].astype(np.float32)
                shape = u.shape[:3]
                # float in, double out in the other layout: the two strides and the two element sizes differ
                ops = {"u": IN(torch.from_numpy(R.layouts(u, np.float32, planar)).to(DEV)), "v": OUT(fshape(shape, 1 - planar), torch.float64)}
                if optional:
                    ops.update(residual=OUT(shape, torch.float64), iters=OUT(shape, torch.uint8), stats=OUT((3,), torch.int64))

                def call(t):
                    opt = [p(t[n]) if optional else None for n in ("residual", "iters", "stats")]
                    return L.cvx_field_invert_f64(p(t["u"]), 0, *strides(shape, planar), *shape, 12, 1e-9, p(t["v"]), 1, *strides(shape, 1 - planar),
                                                  *opt, stream())

                def verify(a):
                    want = R.invert(u, 12, 1e-9)
                    assert same_bits(hwd3(a["v"], 1 - planar), want["v"])
                    if optional:
                        assert same_bits(a["residual"].cpu().numpy(), want["residual"]) and same_bits(a["iters"].cpu().numpy(), want["iters"])
                        assert same_bits(a["stats"].cpu().numpy(), want["stats"]) and int(want["stats"][0]) > 0
                return ops, call, verify
            row("cvx_field_invert_f64", "%s-%s-%s" % (case, "planar" if planar else "interleaved", "all" if optional else "null"))(build_invert)

        def build_compose(L, k=k, planar=planar):
            a = R.smooth_set()[k]
            b = R.invert(a, 2, 0.0)["v"].astype(np.float32)
            shape = a.shape[:3]
            ops = {"a": IN(torch.from_numpy(R.layouts(a, np.float64, planar)).to(DEV)),
                   "b": IN(torch.from_numpy(R.layouts(b, np.float32, 1 - planar)).to(DEV)), "out": OUT(fshape(shape, planar), torch.float32)}

            def call(t):
                return L.cvx_field_compose_f64(p(t["a"]), 1, *strides(shape, planar), p(t["b"]), 0, *strides(shape, 1 - planar), *shape, p(t["out"]), 0,
                                               *strides(shape, planar), stream())
            return ops, call, lambda t: same_bits(hwd3(t["out"], planar), R.compose(a, b).astype(np.float32)) or pytest.fail("differs from the restatement")
        row("cvx_field_compose_f64", "%s-%s" % (case, "planar" if planar else "interleaved"))(build_compose)


@pytest.mark.parametrize("r", ROWS, ids=["%s-%s" % (r[0][4:], r[1]) for r in ROWS])
def test_fenced(L, r):
    operands, call, verify = r[2](L)
    plain = check_fences(operands, call, DEV)
    for k, op in operands.items():                       # the plain run holds no NaN: one in the loud run would come from a moat
        if op.kind == "out" and op.dtype.is_floating_point:
            assert not bool(torch.isnan(plain[k]).any()), "the plain run's %r holds a NaN: the inputs of this row are badly chosen" % k
    verify(plain)


def test_every_field_export_is_fenced():
    from convexadam_amd._field import FIELD_SIGNATURES
    rows = {r[0] for r in ROWS}
    assert rows == set(FIELD_SIGNATURES), "exported without a fence row: %s" % sorted(set(FIELD_SIGNATURES) - rows)
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS), "duplicate row ids"
