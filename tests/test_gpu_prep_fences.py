"""Every kernel-launching entry point of include/convexadam_prep.h between fences (run on the MI355X box with `-m gpu`).

tests/fences.py: each operand sits between two moats of at least 64 KiB; the call runs on plain allocations, fenced with NaN (loud) input
moats and fenced with zero (quiet) input moats; moats stay intact, outputs are byte-identical across the three runs, inputs unchanged.
The workspace is fenced at exactly the queried size.  Each entry point runs at two shapes, one of them 5 x 4 x 131 (a row length that is
a multiple of nothing); the other is one element past a span of 4096 for the flat operators and 7 x 9 x 11 for the volumes, which also
run at rows of 16 and 12 bytes, where the hole filling's sweep along D works in 8- and 4-byte words.  The plain
run is then compared with the restatement.  The last test reads PREP_SIGNATURES: every name is a row here or excused in writing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_restatement as R  # noqa: E402
from fences import IN, OUT, SCRATCH, check_fences  # noqa: E402
from test_gpu_prep import make, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLAT = [("5x4x131", 5 * 4 * 131), ("span+1", 4097)]
VOLUMES = [("5x4x131", (5, 4, 131)), ("7x9x11", (7, 9, 11)), ("6x5x16", (6, 5, 16)), ("3x5x12", (3, 5, 12))]     # the last two: the D sweep in 8- / 4-byte words
ROWS = []


def row(entry, case):
    def deco(build):
        ROWS.append((entry, case, build))
        return build
    return deco


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _prep
    return _prep.lib()


def p(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def npy(t):
    return t.detach().cpu().numpy()


for case, n in FLAT:
    for variant, kw in (("ct", dict(clamp_to=(-1000.0, 1500.0), qs=(0.005, 0.995))), ("positive", dict(positive=True))):
        def build_stats(L, n=n, kw=kw):
            x = make("background", n, 31)
            flags = (1 if "clamp_to" in kw else 0) | (2 if kw.get("positive") else 0)
            lo, hi = kw.get("clamp_to", (0.0, 0.0))
            q = kw.get("qs")
            ops = {"x": IN(torch.from_numpy(x).to(DEV)), "params": OUT((4,)), "moments": OUT((3,), torch.float64),
                   "ws": SCRATCH(L.cvx_prep_stats_workspace_bytes(n))}

            def call(t):
                return L.cvx_prep_stats_f32(p(t["x"]), n, flags, lo, hi, 2 if q else 0, q[0] if q else 0.0, q[1] if q else 0.0, p(t["params"]),
                                            p(t["moments"]), p(t["ws"]), t["ws"].numel(), stream())

            def verify(a):
                want, (count, mean, ss) = R.stats(x, **kw)
                assert same_bits(npy(a["params"]), want) and same_bits(npy(a["moments"]), np.array([count, mean, ss], np.float64))
            return ops, call, verify
        row("cvx_prep_stats_f32", "%s-%s" % (variant, case))(build_stats)

    for mode in (0, 1):
        for host in (False, True):
            def build_norm(L, n=n, mode=mode, host=host):
                x = make("random", n, 32)
                params = np.array([12.5, 300.25, -700.0, 900.0], np.float32)
                ops = {"x": IN(torch.from_numpy(x).to(DEV)), "out": OUT((n,))}
                if not host:
                    ops["params"] = IN(torch.from_numpy(params).to(DEV))
                hp = (C.c_float * 4)(*params.tolist())

                def call(t):
                    return L.cvx_prep_normalise_f32(p(t["x"]), n, None if host else p(t["params"]), hp if host else None, mode, p(t["out"]), stream())
                return ops, call, lambda a: same_bits(npy(a["out"]), R.normalise(x, params, mode)) or pytest.fail("differs from the restatement")
            row("cvx_prep_normalise_f32", "mode%d-%s-%s" % (mode, "host" if host else "device", case))(build_norm)

for case, shape in VOLUMES:
    def build_mask(L, shape=shape):
        g = np.random.default_rng(33)
        data = ((g.random((2,) + shape) < 0.4) * g.normal(size=(2,) + shape)).astype(np.float32)
        H, W, D = shape
        ops = {"data": IN(torch.from_numpy(data).to(DEV)), "mask": OUT(shape, torch.uint8), "box": OUT((6,), torch.int32),
               "count": OUT((1,), torch.int64), "ws": SCRATCH(L.cvx_prep_nonzero_mask_workspace_bytes(H, W, D))}

        def call(t):
            return L.cvx_prep_nonzero_mask_u8(p(t["data"]), 2, H, W, D, 3, p(t["mask"]), p(t["box"]), p(t["count"]), None, p(t["ws"]), t["ws"].numel(),
                                              stream())

        def verify(a):
            want = R.nonzero_mask(data)[0]
            assert np.array_equal(npy(a["mask"]), want.astype(np.uint8)) and int(a["count"].cpu()[0]) == int(want.sum())
            assert npy(a["box"]).tolist() == [v for ax in R.bbox(want) for v in ax]
        return ops, call, verify
    row("cvx_prep_nonzero_mask_u8", case)(build_mask)

    def build_bbox(L, shape=shape):
        g = np.random.default_rng(34)
        m = np.zeros(shape, np.uint8)
        m[1:-1, 1:-1, 2:-3] = g.random((shape[0] - 2, shape[1] - 2, shape[2] - 5)) < 0.2
        H, W, D = shape
        # the loud moat of the byte mask is 1, a valid value: a read outside the mask would count it and move the box
        ops = {"mask": IN(torch.from_numpy(m).to(DEV), loud=1), "box": OUT((6,), torch.int32), "count": OUT((1,), torch.int64)}

        def verify(a):
            assert npy(a["box"]).tolist() == [v for ax in R.bbox(m) for v in ax] and int(a["count"].cpu()[0]) == int(m.sum())
        return ops, lambda t: L.cvx_prep_mask_bbox_i32(p(t["mask"]), H, W, D, p(t["box"]), p(t["count"]), stream()), verify
    row("cvx_prep_mask_bbox_i32", case)(build_bbox)


HOST = "a size query: host arithmetic over the workspace layout, nothing is launched"
EXCLUDED = {"cvx_prep_stats_workspace_bytes": HOST, "cvx_prep_nonzero_mask_workspace_bytes": HOST}


@pytest.mark.parametrize("r", ROWS, ids=["%s-%s" % (r[0][4:], r[1]) for r in ROWS])
def test_fenced(L, r):
    operands, call, verify = r[2](L)
    plain = check_fences(operands, call, DEV)
    for k, op in operands.items():                       # the plain run holds no NaN: one in the loud run would come from a moat
        if op.kind == "out" and op.dtype.is_floating_point:
            assert not bool(torch.isnan(plain[k]).any()), "the plain run's %r holds a NaN: the inputs of this row are badly chosen" % k
    verify(plain)


def test_every_prep_export_is_fenced_or_excused():
    from convexadam_amd._prep import PREP_SIGNATURES
    rows = {r[0] for r in ROWS}
    names = set(PREP_SIGNATURES)
    assert not rows - names and not set(EXCLUDED) - names and not rows & set(EXCLUDED)
    missing = names - rows - set(EXCLUDED)
    assert not missing, "exported without a fence row or a written reason: %s" % sorted(missing)
    assert all(isinstance(v, str) and len(v) > 20 for v in EXCLUDED.values())
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS), "duplicate row ids"
