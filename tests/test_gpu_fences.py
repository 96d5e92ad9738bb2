"""Every kernel-launching entry point of the C ABI between fences (run on the MI355X box with `-m gpu`).

tests/fences.py: each operand of a call sits between two moats of at least 64 KiB; the call runs on plain allocations, fenced with NaN
(loud) input moats and fenced with zero (quiet) input moats.  A store outside an output changes a moat; a read outside an input that
reaches arithmetic turns up as a difference between the loud run and the other two (0 * NaN is NaN); an element the call leaves
unwritten differs between the plain run (outputs start as 0x3C bytes) and the fenced ones (0xA5).  Every assertion is equality of bytes.
Workspaces and scratch buffers are fenced as well (their moats only), at exactly the queried size.

One table, ROWS, drives the file: (entry point, case, options) -> a builder that returns the operands, the raw ctypes call and, where
the shape is new to the suite and the oracle has the operator, a comparison of the plain run with the oracle.  Shapes are the
smallest at which an overhang exists: one past every tile edge, below one tile, and row lengths around the vector / word width.  The
16-byte kernels take rows of whole quads only (every other length goes to a scalar kernel), so each operator that has one also gets
shapes with D % 4 == 0 that are ragged against that kernel's own tiles, and the options that select a kernel are set at those.  The
last test reads the exported names from _lib.SIGNATURES: each is a row here or listed in EXCLUDED with its reason."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fences import IN, INOUT, OUT, SCRATCH, check_fences  # noqa: E402
from test_gpu_workspace import PAIR_SHAPES, _bases, _pair, _volume, option, p, rnd, stream  # noqa: E402

DEV = "cuda:0"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "convexadam_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _lib
    return _lib.lib()


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def kconst(fname, name):
    """A tile constant as the kernel source states it (`NAME = 123`)."""
    return int(re.search(r"\b%s\s*=\s*(\d+)" % name, _src(fname)).group(1))


# ---- tile constants, from the kernels ----------------------------------------------------------------------------------------------
MIND_TZ, MIND_TY = kconst("mind.hip", "TZ"), kconst("mind.hip", "TY")
MIND_TX = sorted(set(int(x) for x in re.findall(r"k_mind<R, (\d+)>", _src("mind.hip"))))       # [32, 64]: 32 for radius 3 with dilation 4
MP_TX = kconst("mind.hip", "MP_TX")
MARCH_TILES = sorted(set((int(a), int(b)) for a, b in re.findall(r"launch_mind_march_g<MMGeo<(\d+), (\d+)>>", _src("mindmarch.hip"))))     # (TY, TX) of k_mind_march
BOX_TILE = tuple(int(x) for x in re.search(r"kind 2 = (\d+) x (\d+) x (\d+)", _src("boxtile.hip")).groups())       # the large tiles of k_box3_tile (z, y, x)
BT = (kconst("adam.hip", "BT_Z"), kconst("adam.hip", "BT_Y"), kconst("adam.hip", "BT_X"))                             # the z-marching boxes
WARP_TILE = tuple(int(x) for x in re.search(r"(\d+) x (\d+) x (\d+) voxel tile per workgroup", _src("warp.hip")).groups())     # k_warp_grad
WORD = int(re.search(r"\(D \+ \d+\) / (\d+)", _src("surfdist.hip")).group(1))                                      # bits of a plane word
assert len(MIND_TX) == 2 and len(MARCH_TILES) == 2 and BOX_TILE[2] % 4 == 0, (MIND_TX, MARCH_TILES, BOX_TILE)


def quads(d):
    """the next row length that is a whole number of 16-byte quads: what the vector kernels take"""
    return -(-d // 4) * 4


def ragged(tile):
    """one element past every tile edge"""
    return tuple(t + 1 for t in tile)


ROWS = []


class Row:
    def __init__(self, entry, case, opts, build):
        self.entry, self.case, self.opts, self.build = entry, case, opts, build
        self.id = "%s-%s%s" % (entry[4:], case, "".join("-%s%d" % kv for kv in sorted(opts.items())))


def row(entry, case, opts_list=({},)):
    def deco(build):
        for o in opts_list:
            ROWS.append(Row(entry, case, dict(o), build))
        return build
    return deco


def morc():
    from oracle import metrics_oracle
    return metrics_oracle


def vp(arr):
    return C.cast(arr, C.c_void_p)


def npy(t):
    return t.detach().cpu().numpy()


def same(t, ref):
    a, b = npy(t), np.asarray(ref)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), "the plain run differs from the oracle"


def ws_of(t, name="ws"):
    return (p(t[name]), t[name].numel()) if name in t else (None, 0)


def labels(shape, nl, seed):
    """a label phantom: blocks of a few voxels, values 0..nl"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, nl + 1, tuple(-(-s // 3) for s in shape), generator=g).float()
    full = coarse.repeat_interleave(3, 0).repeat_interleave(3, 1).repeat_interleave(3, 2)
    return full[:shape[0], :shape[1], :shape[2]].contiguous().to(DEV)


# ---- descriptors ---------------------------------------------------------------------------------------------------------------------
def mind_rows():
    cases = [("ragged64", ragged((MIND_TZ, MIND_TY, MIND_TX[1])), 1, 2), ("below", (2, 3, 5), 1, 2), ("row63", (3, 4, 63), 1, 2),
             ("row64", (3, 4, 64), 1, 2), ("tiny", (1, 2, 3), 2, 2),
             # rows of whole quads: r = 1, d = 2 then runs the z-marching stencil (mindmarch.hip) unless mind_tiled = 1 -- the smallest members of
             # test_mindssc_marching_kernel_shapes, and one past both of its tiles in y and x
             ("march-2x3x4", (2, 3, 4), 1, 2), ("march-3x9x8", (3, 9, 8), 1, 2), ("march-7x17x68", (7, 17, 68), 1, 2)] + \
            [("march-ragged%dx%d" % t, (3, t[0] + 1, t[1] + 4), 1, 2) for t in MARCH_TILES]
    for case, shape, r, d in cases:
        def build(L, orc, shape=shape, r=r, d=d):
            H, W, D = shape
            img = rnd(shape, 1, 0.0, 100.0)
            ops = {"img": IN(img), "out": OUT((12,) + shape), "ws": SCRATCH(L.cvx_mindssc_workspace_bytes(H, W, D, r, d))}
            return ops, lambda t: L.cvx_mindssc_f32(p(t["img"]), H, W, D, r, d, p(t["out"]), *ws_of(t), stream()), \
                lambda a: same(a["out"], orc.mindssc(npy(img), r, d))
        row("cvx_mindssc_f32", case, [{}, {"mind_tiled": 1}])(build)

    def build32(L, orc):                          # radius 3 with dilation 4: the 32-column tile
        shape = ragged((MIND_TZ, MIND_TY, MIND_TX[0]))
        H, W, D = shape
        img = rnd(shape, 2, 0.0, 100.0)
        ops = {"img": IN(img), "out": OUT((12,) + shape), "ws": SCRATCH(L.cvx_mindssc_workspace_bytes(H, W, D, 3, 4))}
        return ops, lambda t: L.cvx_mindssc_f32(p(t["img"]), H, W, D, 3, 4, p(t["out"]), *ws_of(t), stream()), \
            lambda a: same(a["out"], orc.mindssc(npy(img), 3, 4))
    row("cvx_mindssc_f32", "r3d4-ragged32")(build32)


mind_rows()


def mind_pooled_rows():
    # windows (g1, g2); D even (8-byte row segments); one past the pooling tile (T = the larger window, MP_TX columns); rows of a multiple
    # of 4 voxels are what the single pass takes
    for g1, g2 in [(6, 2), (4, 2), (6, 3), (6, 0)]:
        T = max(g1, g2)
        for case, shape in [("ragged", (T + 1, 2 * T + 1, MP_TX + 2)), ("ragged4", (T + 1, 2 * T + 1, MP_TX + 4)), ("rows4", (T, T + 1, MP_TX + 4)),
                            ("onetile", (T, T, T)), ("onetile4", (T, T, quads(T + 1)))]:
            def build(L, orc, g1=g1, g2=g2, shape=shape):
                H, W, D = shape
                img = rnd(shape, 3, 0.0, 100.0)
                nscr = L.cvx_mindssc_pooled_scratch_bytes(H, W, D, 1, 2, g1, g2)
                ops = {"img": IN(img), "o1": OUT((12, H // g1, W // g1, D // g1)), "ws": SCRATCH(L.cvx_mindssc_workspace_bytes(H, W, D, 1, 2))}
                if g2:
                    ops["o2"] = OUT((12, H // g2, W // g2, D // g2))
                if nscr:
                    ops["scr"] = SCRATCH(nscr)

                def call(t):
                    return L.cvx_mindssc_pooled_f32(p(t["img"]), H, W, D, 1, 2, g1, p(t["o1"]), g2, p(t.get("o2")), *ws_of(t, "scr"), *ws_of(t), None, stream())

                def verify(a):
                    full = orc.mindssc(npy(img), 1, 2)
                    same(a["o1"], orc.avgpool_stride(full, g1))
                    if g2:
                        same(a["o2"], orc.avgpool_stride(full, g2))
                return ops, call, verify
            row("cvx_mindssc_pooled_f32", "g%d_%d-%s" % (g1, g2, case), [{}, {"mind_single": 1}, {"mind_single": 2}])(build)


mind_pooled_rows()

# (even rows take k_avgpool_even for g = 2, 4, 6, 8; odd rows and other windows the generic kernel)
for _g, _shape in [(2, (3, 5, 7, 9)), (3, (2, 7, 9, 10)), (2, (1, 2, 2, 2)), (3, (1, 3, 4, 5)), (2, (3, 5, 7, 10)), (4, (2, 9, 10, 14)), (6, (2, 13, 7, 20)),
                   (8, (1, 9, 8, 18)), (4, (1, 4, 4, 4)), (6, (1, 6, 6, 6))]:
    def _build_avgpool(L, orc, g=_g, shape=_shape):
        c, H, W, D = shape
        x = rnd(shape, 4, -1.0, 1.0)
        ops = {"x": IN(x), "out": OUT((c, H // g, W // g, D // g))}
        return ops, lambda t: L.cvx_avgpool_f32(p(t["x"]), c, H, W, D, g, p(t["out"]), stream()), lambda a: same(a["out"], orc.avgpool_stride(npy(x), g))
    row("cvx_avgpool_f32", "g%d-%s" % (_g, "x".join(map(str, _shape))))(_build_avgpool)


def _present(nl):
    return torch.arange(1, nl + 1, dtype=torch.int32, device=DEV), rnd((nl,), 5, 0.5, 2.0)


for _V in [1, 255, 256, 257]:
    def _build_label_features(L, orc, V=_V):
        lab = labels((1, 1, V), 4, V).reshape(-1)
        present, weights = _present(4)
        ops = {"lab": IN(lab), "present": IN(present, loud=1), "weights": IN(weights), "feat": OUT((4, V))}
        return ops, lambda t: L.cvx_label_features_f32(p(t["lab"]), V, 4, p(t["present"]), p(t["weights"]), 10.0, p(t["feat"]), stream()), \
            lambda a: same(a["feat"], np.stack([(np.float32(10.0) * npy(weights)[c]) * (npy(lab) == c + 1).astype(np.float32) for c in range(4)]))
    row("cvx_label_features_f32", "V%d" % _V)(_build_label_features)

for _shape, _g1, _g2 in [((7, 9, 11), 2, 3), ((5, 6, 65), 4, 2), ((2, 2, 2), 2, 0), ((3, 3, 3), 1, 0)]:
    def _build_label_pooled(L, orc, shape=_shape, g1=_g1, g2=_g2):
        H, W, D = shape
        lab = labels(shape, 4, 6)
        present, weights = _present(4)
        ops = {"lab": IN(lab), "present": IN(present, loud=1), "weights": IN(weights), "o1": OUT((4, H // g1, W // g1, D // g1))}
        if g2:
            ops["o2"] = OUT((4, H // g2, W // g2, D // g2))
        return ops, lambda t: L.cvx_label_features_pooled_f32(p(t["lab"]), H, W, D, 4, p(t["present"]), p(t["weights"]), 10.0, g1, p(t["o1"]), g2,
                                                             p(t.get("o2")), stream()), None
    row("cvx_label_features_pooled_f32", "%s-g%d_%d" % ("x".join(map(str, _shape)), _g1, _g2))(_build_label_pooled)

SMALL3 = [(7, 9, 11), (1, 1, 1), (2, 1, 3), (3, 4, 65)]

for _shape in SMALL3:
    def _build_erode(L, orc, shape=_shape):
        H, W, D = shape
        mask = (rnd(shape, 7) > 0.3).float()
        ops = {"mask": IN(mask), "out": OUT(shape)}
        return ops, lambda t: L.cvx_mask_erode_f32(p(t["mask"]), H, W, D, 0.9, p(t["out"]), stream()), \
            lambda a: same(a["out"], (orc.box3_replicate(npy(mask)) > np.float32(0.9)).astype(np.float32))
    row("cvx_mask_erode_f32", "x".join(map(str, _shape)))(_build_erode)

    def _build_ft(L, orc, shape=_shape):
        H, W, D = shape
        obj = (rnd(shape, 8) > 0.4).float()
        obj.view(-1)[0] = 0.0                                  # at least one zero voxel to be found
        ops = {"obj": IN(obj), "feat": OUT((3,) + shape, torch.int32), "ws": SCRATCH(L.cvx_feature_transform_workspace_bytes(H, W, D))}
        return ops, lambda t: L.cvx_feature_transform_i32(p(t["obj"]), H, W, D, p(t["feat"]), *ws_of(t), stream()), \
            lambda a: same(a["feat"], orc.feature_transform(npy(obj)))
    row("cvx_feature_transform_i32", "x".join(map(str, _shape)))(_build_ft)


# ---- convex stage --------------------------------------------------------------------------------------------------------------------
CORR_SHAPES = [(5, 6, 7), (1, 2, 3), (3, 2, 9), (2, 3, 8)]  # rows of 7, 3, 9 and 8 voxels: 2 quads - 1, below one quad, 2 quads + 1, 2 quads


def corr_rows():
    from convexadam_amd._lib import CorrOpts
    for C_ in (5, 12, 20):
        for fast in (0, 1, 2):
            for f16 in (0, 2):
                if f16 and fast == 2:
                    continue
                for shape in CORR_SHAPES:
                    def build(L, orc, C_=C_, fast=fast, f16=f16, shape=shape):
                        h, w, d = shape
                        hw = 2
                        K, v = (2 * hw + 1) ** 3, h * w * d
                        fix, mov = rnd((C_,) + shape, 9), rnd((C_,) + shape, 10)
                        co = CorrOpts(0, 2, fast, f16)
                        ops = {"fix": IN(fix), "mov": IN(mov), "ssd": OUT((K,) + shape, torch.float16 if f16 == 2 else torch.float32),
                               "argmin": OUT(shape, torch.int64), "ws": SCRATCH(L.cvx_correlate_workspace_bytes(C_, h, w, d, hw))}

                        def call(t):
                            return L.cvx_correlate_ex_f32(p(t["fix"]), p(t["mov"]), C_, h, w, d, hw, C.byref(co), p(t["ssd"]), p(t["argmin"]), *ws_of(t), stream())

                        def verify(a):
                            ssd, am = orc.correlate(npy(fix), npy(mov), hw)
                            same(a["argmin"], am)          # (fast = 2: the certified argmin is the exact volume's)
                            if fast == 0:
                                same(a["ssd"], ssd)
                        return ops, call, verify if (f16 == 0 and fast != 1) else None
                    opts = [{}, {"corr_fused_all": 1}, {"cert_unfused": 2}] + ([{"corr_unfused": 1}] if fast != 1 and not f16 else [])
                    row("cvx_correlate_ex_f32", "C%d-fast%d-f16_%d-%s" % (C_, fast, f16, "x".join(map(str, shape))), opts)(build)


corr_rows()


def coupled_rows():
    for entry in ("cvx_coupled_convex_f32", "cvx_coupled_convex_f16", "cvx_coupled_convex_masked_f32"):
        for shape in CORR_SHAPES:
            def build(L, orc, entry=entry, shape=shape):
                h, w, d = shape
                hw = 2
                K = (2 * hw + 1) ** 3
                ssd, am, mesh = _volume(L, 12, shape, hw, 11)
                torch.cuda.synchronize()
                f16, masked = entry.endswith("f16"), "masked" in entry
                ssd = (ssd.half() if f16 else ssd).reshape((K,) + shape)
                ops = {"ssd": IN(ssd), "argmin": IN(am.reshape(shape), loud=K - 1), "mesh": IN(mesh.reshape(3, K)), "out": OUT((3,) + shape),
                       "ws": SCRATCH(L.cvx_coupled_convex_workspace_bytes(h, w, d, hw))}
                if masked:
                    mask = (rnd(shape, 12) > 0.3).to(torch.uint8)
                    ops["mask"] = IN(mask, loud=1)

                def call(t):
                    head = (p(t["ssd"]), p(t["argmin"]), p(t["mesh"])) + ((p(t["mask"]),) if masked else ())
                    return getattr(L, entry)(*head, h, w, d, hw, p(t["out"]), *ws_of(t), stream())
                verify = None if (f16 or masked) else (lambda a: same(a["out"], orc.coupled_convex(npy(ssd), npy(am).reshape(shape), npy(mesh).reshape(3, K), hw)))
                return ops, call, verify
            row(entry, "x".join(map(str, shape)), [{}, {"no_prune": 1}])(build)


coupled_rows()

for _iters in (1, 2):
    for _shape in CORR_SHAPES + [(12, 10, 14)]:
        def _build_ic(L, orc, iters=_iters, shape=_shape):
            h, w, d = shape
            f1, f2 = rnd((3,) + shape, 13, -0.05, 0.05), rnd((3,) + shape, 14, -0.05, 0.05)
            bh, bw, bd = _bases(L, shape)
            torch.cuda.synchronize()
            ops = {"f1": IN(f1), "f2": IN(f2), "bh": IN(bh), "bw": IN(bw), "bd": IN(bd), "o1": OUT((3,) + shape), "o2": OUT((3,) + shape),
                   "ws": SCRATCH(L.cvx_inverse_consistency_workspace_bytes(h, w, d))}

            def call(t):
                return L.cvx_inverse_consistency_f32(p(t["f1"]), p(t["f2"]), h, w, d, iters, p(t["bh"]), p(t["bw"]), p(t["bd"]), p(t["o1"]), p(t["o2"]),
                                                     *ws_of(t), stream())

            def verify(a):
                o1, o2 = orc.inverse_consistency(npy(f1), npy(f2), iters)
                same(a["o1"], o1)
                same(a["o2"], o2)
            return ops, call, verify
        row("cvx_inverse_consistency_f32", "it%d-%s" % (_iters, "x".join(map(str, _shape))))(_build_ic)

for _ic, _shape in [(0, (5, 6, 7)), (2, (5, 6, 7)), (2, (3, 2, 9))]:
    def _build_stage(L, orc, ic=_ic, shape=_shape):
        from convexadam_amd._lib import StageParams
        h, w, d = shape
        gs, hw, C_ = 2, 2, 12
        H, W, D = h * gs + 1, w * gs, d * gs + 1
        sp = StageParams(C_, h, w, d, hw, gs, ic, H, W, D, None, (C.c_int * 4)(0, 0, 0, 0))
        ff, fm = rnd((C_,) + shape, 15), rnd((C_,) + shape, 16)
        mf, mm = (rnd(shape, 17) > 0.2).to(torch.uint8), (rnd(shape, 18) > 0.2).to(torch.uint8)
        ops = {"ff": IN(ff), "fm": IN(fm), "mf": IN(mf, loud=1), "mm": IN(mm, loud=1), "coarse": OUT((3,) + shape), "hr": OUT((3, H, W, D)),
               "ws": SCRATCH(L.cvx_convex_stage_workspace_bytes(C.byref(sp)))}
        return ops, lambda t: L.cvx_convex_stage_f32(p(t["ff"]), p(t["fm"]), p(t["mf"]), p(t["mm"]), C.byref(sp), p(t["coarse"]), p(t["hr"]), *ws_of(t),
                                                     stream()), None
    row("cvx_convex_stage_f32", "ic%d-%s" % (_ic, "x".join(map(str, _shape))), [{}, {"no_prune": 1}])(_build_stage)

for _shape in [(5, 6, 7), (1, 1, 1), (3, 2, 9)]:
    def _build_samples(L, orc, shape=_shape):
        h, w, d = shape
        H, W, D = 2 * h + 1, 2 * w, 2 * d + 1
        field = rnd((3,) + shape, 19, -2.0, 2.0)
        mask = (rnd(shape, 20) > 0.3).to(torch.uint8)
        mask.view(-1)[0] = 1
        v = h * w * d
        cnt = C.c_int64(0)
        ops = {"field": IN(field), "mask": IN(mask, loud=1), "T1": OUT((v, 4)), "T2": OUT((v, 4)),
               "ws": SCRATCH(L.cvx_rigid_samples_workspace_bytes(h, w, d, H, W, D))}
        M = int(mask.sum())

        def call(t):
            rc = L.cvx_rigid_samples_f32(p(t["field"]), p(t["mask"]), h, w, d, H, W, D, p(t["T1"]), p(t["T2"]), C.byref(cnt), *ws_of(t), stream())
            assert cnt.value == M, "kept cells: %d, the mask holds %d" % (cnt.value, M)
            torch.cuda.synchronize()
            for k in ("T1", "T2"):                          # the contract writes M rows; the rest keeps the buffer's bytes, which differ by run
                t[k][M:].zero_()
            return rc
        return ops, call, None
    row("cvx_rigid_samples_f32", "x".join(map(str, _shape)))(_build_samples)


# ---- resampling and smoothing --------------------------------------------------------------------------------------------------------
for _entry in ("cvx_resize_trilinear_f32", "cvx_resize_trilinear_ac_f32"):
    for _C in (1, 3, 5):
        for _case, _in, _out in [("up2", (3, 4, 5), (6, 8, 10)), ("up2-one", (1, 1, 1), (2, 2, 2)), ("generic", (3, 4, 5), (7, 5, 9)),
                                 ("down", (5, 6, 9), (2, 3, 4)), ("row65", (2, 2, 33), (3, 3, 65))]:
            def _build_resize(L, orc, entry=_entry, C_=_C, i=_in, o=_out):
                x = rnd((C_,) + i, 21, -1.0, 1.0)
                ops = {"x": IN(x), "out": OUT((C_,) + o)}
                verify = (lambda a: same(a["out"], orc.resize_trilinear(npy(x), o))) if entry == "cvx_resize_trilinear_f32" else None
                return ops, lambda t: getattr(L, entry)(p(t["x"]), C_, *i, p(t["out"]), *o, stream()), verify
            row(_entry, "C%d-%s" % (_C, _case))(_build_resize)

for _C, _in, _out in [(1, (3, 4, 5), (2, 3, 7)), (3, (1, 1, 1), (2, 2, 2)), (2, (5, 3, 9), (4, 4, 65))]:
    def _build_gs(L, orc, C_=_C, i=_in, o=_out):
        vol = rnd((C_,) + i, 22, -1.0, 1.0)
        grid = rnd(o + (3,), 23, -1.3, 1.3)                  # some samples outside: zero padding
        ops = {"vol": IN(vol), "grid": IN(grid), "out": OUT((C_,) + o)}
        return ops, lambda t: L.cvx_grid_sample_f32(p(t["vol"]), C_, *i, p(t["grid"]), *o, p(t["out"]), stream()), \
            lambda a: same(a["out"], orc.grid_sample(npy(vol), npy(grid)))
    row("cvx_grid_sample_f32", "C%d-%s" % (_C, "x".join(map(str, _out))))(_build_gs)

# rows of whole quads take the 16-byte kernels (k_box_walk of launch_box_zero), the others the scalar ones: both at every kind of shape
SMOOTH_SHAPES = [(3, 7, 9, 11), (3, 7, 9, 12), (3, 1, 1, 1), (3, 2, 3, 4), (3, 2, 3, 63), (3, 2, 3, 64), (3, 2, 3, 65), (3,) + ragged(BOX_TILE),
                 (3,) + ragged(BOX_TILE)[:2] + (BOX_TILE[2] + 4,)]

for _shape in SMOOTH_SHAPES:
    _sid = "x".join(map(str, _shape))
    for _k in (2, 4):
        if min(_shape[1:]) < _k // 2:                   # refused: avg_pool3d needs input >= pad
            continue

        def _build_grow(L, orc, shape=_shape, k=_k):
            c, H, W, D = shape
            x = rnd(shape, 24, -1.0, 1.0)
            ops = {"x": IN(x), "out": OUT((c, H + 1, W + 1, D + 1))}
            return ops, lambda t: L.cvx_box_grow_f32(p(t["x"]), c, H, W, D, k, p(t["out"]), stream()), lambda a: same(a["out"], orc.box_grow(npy(x), k))
        row("cvx_box_grow_f32", "k%d-%s" % (_k, _sid))(_build_grow)

    for _passes in (1, 3):
        def _build_bs(L, orc, shape=_shape, passes=_passes):
            c, H, W, D = shape
            x = rnd(shape, 25, -1.0, 1.0)
            need = L.cvx_box_smooth_workspace_bytes(c, H, W, D, passes)
            ops = {"x": IN(x), "out": OUT(shape)}
            if need:
                ops["ws"] = SCRATCH(need)
            return ops, lambda t: L.cvx_box_smooth_f32(p(t["x"]), c, H, W, D, 3, passes, p(t["out"]), *ws_of(t), stream()), None
        row("cvx_box_smooth_f32", "p%d-%s" % (_passes, _sid))(_build_bs)

    for _kind, _bw in [("box35", 0), ("box35", 1), ("gauss", 0), ("gauss", 1)]:
        def _build_smooth(L, orc, shape=_shape, kind=_kind, bw=_bw):
            from convexadam_amd._lib import Smoother
            c, H, W, D = shape
            x = rnd(shape, 26, -1.0, 1.0)
            sm = Smoother(0, 2, (C.c_int * 4)(3, 5, 0, 0), (C.c_float * 5)(0, 0, 0, 0, 0)) if kind == "box35" else \
                Smoother(1, 0, (C.c_int * 4)(0, 0, 0, 0), (C.c_float * 5)(0.0625, 0.25, 0.375, 0.25, 0.0625))
            osm = orc.make_smoother(boxes=[3, 5]) if kind == "box35" else orc.make_smoother(gauss_w=[0.0625, 0.25, 0.375, 0.25, 0.0625])
            ops = {"x": IN(x), "out": OUT(shape), "ws": SCRATCH(L.cvx_smooth_workspace_bytes(c, H, W, D))}
            return ops, lambda t: L.cvx_smooth_f32(p(t["x"]), c, H, W, D, C.byref(sm), bw, p(t["out"]), *ws_of(t), stream()), \
                lambda a: same(a["out"], orc.smooth(npy(x), osm, bool(bw)))
        row("cvx_smooth_f32", "%s-bw%d-%s" % (_kind, _bw, _sid))(_build_smooth)

    for _bw in (0, 1):
        def _build_sf(L, orc, shape=_shape, bw=_bw):
            from convexadam_amd._lib import Smoother
            c, H, W, D = shape
            x = rnd(shape, 27, -1.0, 1.0)
            sm = Smoother(0, 2, (C.c_int * 4)(3, 5, 0, 0), (C.c_float * 5)(0, 0, 0, 0, 0))
            ops = {"x": IN(x), "out": OUT(shape)}
            return ops, lambda t: L.cvx_smooth_fast_f32(p(t["x"]), H, W, D, C.byref(sm), bw, p(t["out"]), stream()), \
                lambda a: same(a["out"], orc.fast_boxchain(npy(x), [3, 5], bool(bw)))
        row("cvx_smooth_fast_f32", "bw%d-%s" % (_bw, _sid))(_build_sf)

    def _build_b3(L, orc, shape=_shape):
        c, H, W, D = shape
        x = rnd(shape, 28, -1.0, 1.0)
        ops = {"x": IN(x), "out": OUT(shape)}
        return ops, lambda t: L.cvx_box3_fast_f32(p(t["x"]), H, W, D, p(t["out"]), stream()), lambda a: same(a["out"], orc.fast_box3x3(npy(x)))
    row("cvx_box3_fast_f32", _sid)(_build_b3)

for _mode in (0, 1):
    for _C, _in, _out in [(1, (3, 4, 5), (2, 3, 7)), (3, (1, 1, 1), (2, 2, 2)), (2, (5, 3, 9), (4, 4, 65))]:
        def _build_aw(L, orc, mode=_mode, C_=_C, i=_in, o=_out):
            vol = rnd((C_,) + i, 29, -1.0, 1.0)
            theta = torch.tensor([[0.9, 0.1, 0.0, 0.05], [-0.1, 1.1, 0.05, -0.1], [0.0, 0.05, 1.2, 0.2]], device=DEV)      # part of the output samples outside
            ops = {"vol": IN(vol), "theta": IN(theta), "out": OUT((C_,) + o)}
            return ops, lambda t: L.cvx_affine_warp_f32(p(t["vol"]), C_, *i, p(t["theta"]), *o, mode, p(t["out"]), stream()), None
        row("cvx_affine_warp_f32", "mode%d-C%d-%s" % (_mode, _C, "x".join(map(str, _out))))(_build_aw)

for _q in (0, 1):
    for _shape in SMALL3:
        def _build_pack(L, orc, q=_q, shape=_shape):
            H, W, D = shape
            f = rnd((3,) + shape, 30, -20.0, 20.0)
            ops = {"f": IN(f), "out": OUT(shape + (3,), torch.float64)}
            want = npy(f.half().float() if q else f).astype(np.float64).transpose(1, 2, 3, 0)
            return ops, lambda t: L.cvx_pack_field_f64(p(t["f"]), H, W, D, q, p(t["out"]), stream()), lambda a: same(a["out"], np.ascontiguousarray(want))
        row("cvx_pack_field_f64", "q%d-%s" % (_q, "x".join(map(str, _shape))))(_build_pack)


def doubles(vals):
    return (C.c_double * len(vals))(*vals)


MAP12 = [0.9, 0.05, 0.0, -0.05, 1.1, 0.0, 0.0, 0.05, 0.8, 0.3, -0.6, 0.4]          # M (3 x 3, x y z order), t: part of the output falls outside

for _s64, _o64 in [(1, 1), (0, 0), (0, 1)]:
    for _src_shape, _out_shape in [((5, 6, 7), (6, 5, 9)), ((1, 1, 1), (2, 2, 2)), ((3, 2, 65), (2, 3, 66))]:
        def _build_rs(L, orc, s64=_s64, o64=_o64, s=_src_shape, o=_out_shape):
            src = rnd(s, 31, -1.0, 1.0, torch.float64 if s64 else torch.float32)
            m = doubles(MAP12)
            ops = {"src": IN(src), "out": OUT(o, torch.float64 if o64 else torch.float32)}
            return ops, lambda t: L.cvx_resample_linear_f64(p(t["src"]), s64, *s, p(t["out"]), o64, *o, vp(m), -1.5, stream()), None
        row("cvx_resample_linear_f64", "s%d-o%d-%s" % (_s64, _o64, "x".join(map(str, _out_shape))))(_build_rs)

for _planar in (1, 0):
    for _f, _m in [((5, 6, 7), (6, 5, 9)), ((1, 1, 1), (2, 2, 2)), ((3, 2, 65), (2, 3, 66))]:
        def _build_ftg(L, orc, planar=_planar, f=_f, mext=_m):
            V = f[0] * f[1] * f[2]
            field = rnd((3,) + f if planar else f + (3,), 32, -1.5, 1.5, torch.float32 if planar else torch.float64)
            moving = rnd(mext, 33, 0.0, 1.0, torch.float64)
            cs, vs = (V, 1) if planar else (1, 3)
            m, rot, ratio = doubles(MAP12), doubles([1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0]), doubles([1.0, 0.5, 2.0])
            ops = {"field": IN(field), "moving": IN(moving), "carried": OUT(mext + (3,), torch.float64), "warped": OUT(mext, torch.float64)}

            def call(t):
                return L.cvx_field_to_grid_f64(p(t["field"]), 0 if planar else 1, cs, vs, *f, vp(m), vp(rot), vp(ratio), p(t["moving"]), 1, *mext,
                                               p(t["carried"]), p(t["warped"]), 1, stream())
            return ops, call, None
        row("cvx_field_to_grid_f64", "%s-%s" % ("planar" if _planar else "interleaved", "x".join(map(str, _m))))(_build_ftg)

FM_SPAN = kconst("fieldmean.hip", "FM_THREADS") * kconst("fieldmean.hip", "FM_K")

for _case, _shape in [("oneblock-1", (1, 1, FM_SPAN - 1)), ("oneblock+1", (1, 1, FM_SPAN + 1)), ("small", (2, 3, 5)), ("voxel", (1, 1, 1))]:
    for _sel in ("all", "mask", "seg"):
        def _build_fm(L, orc, shape=_shape, sel=_sel):
            H, W, D = shape
            field = rnd((3,) + shape, 34, -2.0, 2.0)
            ops = {"field": IN(field), "sums": OUT((3,), torch.float64), "count": OUT((1,), torch.int64), "ws": SCRATCH(L.cvx_field_mean_workspace_bytes(H, W, D))}
            m, sext = None, (0, 0, 0)
            if sel == "mask":
                ops["mask"] = IN((rnd(shape, 35) > 0.5).to(torch.uint8), loud=1)
            if sel == "seg":
                sext = (3, 4, 5)
                ops["seg"] = IN((rnd(sext, 36, 0.0, 1.0, torch.float64) > 0.5).double())
                m = doubles([0.5 * sext[2] / D, 0.0, 0.0, 0.0, 0.9 * sext[1] / W, 0.0, 0.0, 0.0, 1.2 * sext[0] / H, 0.1, 0.0, -0.2])

            def call(t):
                return L.cvx_field_mean_f64(p(t["field"]), 0, H * W * D, 1, H, W, D, 0, p(t.get("mask")), p(t.get("seg")), 0, *sext, vp(m) if m else None,
                                            p(t["sums"]), p(t["count"]), *ws_of(t), stream())
            return ops, call, None
        row("cvx_field_mean_f64", "%s-%s" % (_sel, _case))(_build_fm)

for _shape in SMALL3:
    def _build_mc(L, orc, shape=_shape):
        H, W, D = shape
        moving = rnd(shape, 37, 0.0, 1.0, torch.float64)
        disp = rnd(shape + (3,), 38, -2.0, 2.0, torch.float64)
        ops = {"moving": IN(moving), "disp": IN(disp), "out": OUT(shape, torch.float64)}
        return ops, lambda t: L.cvx_map_coordinates_linear_f64(p(t["moving"]), p(t["disp"]), H, W, D, p(t["out"]), stream()), \
            lambda a: same(a["out"], np.asarray(morc().apply_convex(npy(disp), npy(moving)), np.float64).reshape(shape))
    row("cvx_map_coordinates_linear_f64", "x".join(map(str, _shape)))(_build_mc)

for _flags, _name in [(4 | 2, "f32"), (4, "f16")]:
    for _shape in [(7, 9, 11), (2, 2, 2), (3, 4, 9), (2, 3, 65)]:
        def _build_crop(L, orc, flags=_flags, shape=_shape):
            H, W, D = shape
            field = rnd((3,) + shape, 39, -5.0, 5.0)
            ops = {"field": IN(field), "out": OUT((3, H // 2, W // 2, D // 2), torch.float32 if flags & 2 else torch.float16)}
            return ops, lambda t: L.cvx_crop_field_half_f32(p(t["field"]), H * W * D, 1, H, W, D, None, H, W, D, 0, flags, p(t["out"]), stream()), None
        row("cvx_crop_field_half_f32", "identity-%s-%s" % (_name, "x".join(map(str, _shape))))(_build_crop)


# ---- Adam loop -----------------------------------------------------------------------------------------------------------------------
# k_box3_tile (boxtile.hip) takes rows of whole quads only: one voxel past its tile in z and y and one quad past it in x -- (13, 17, 60), every
# tile ragged -- and (5, 3, 8), smaller than one tile, run it when box_fwd_tile / box_bwd_tile select it (2000 the large tiles, 1000 the small
# ones; the automatic choice takes tiles only where they fill the chip, so at these sizes the default is the z-marching kernels, as with 0).
# The marching boxes and k_warp_grad get one past their own tiles, with rows of whole quads (the 16-byte staging path) and without.
ADAM_TILE_SHAPES = [ragged(BOX_TILE)[:2] + (BOX_TILE[2] + 4,), (5, 3, 8), ragged(BT)[:2] + (quads(BT[2] + 1),)]
ADAM_SHAPES = ADAM_TILE_SHAPES + [ragged(BOX_TILE), (3, 3, 5), (6, 9, 30), ragged(BT), ragged(WARP_TILE), ragged(WARP_TILE)[:2] + (quads(WARP_TILE[2] + 1),)]
TILE_OPTS = [{"box_fwd_tile": 2000, "box_bwd_tile": 2000}, {"box_fwd_tile": 1000, "box_bwd_tile": 1000}]


def adam_rows():
    from convexadam_amd._lib import Smoother
    variants = [("cvx_adam_run_ex_f32", "exact-f32", lambda sm: (None, 0)), ("cvx_adam_run_ex_f32", "exact-f16", lambda sm: (None, 1)),
                ("cvx_adam_run_ex_f32", "chain35-f32", lambda sm: (sm, 0)), ("cvx_adam_run_mode_f32", "fast", lambda sm: (None, 1)),
                ("cvx_adam_run_mode_f32", "fast_all", lambda sm: (None, 2)), ("cvx_adam_run_mode_f32", "fast_all-f16", lambda sm: (None, 2 | 16)),
                ("cvx_adam_run_mode_f32", "fast-chain35", lambda sm: (sm, 1))]
    for entry, name, tail in variants:
        for C_ in (12, 5):
            for shape in ADAM_SHAPES:
                def build(L, orc, entry=entry, name=name, tail=tail, C_=C_, shape=shape):
                    h, w, d = shape
                    F2, M2 = rnd((C_,) + shape, 40), rnd((C_,) + shape, 41)
                    P0 = rnd((3,) + shape, 42, -0.5, 0.5)
                    bh, bw, bd = _bases(L, shape)
                    torch.cuda.synchronize()
                    sm = Smoother(0, 2, (C.c_int * 4)(3, 5, 0, 0), (C.c_float * 5)(0, 0, 0, 0, 0))
                    smo, last = tail(sm)
                    its = (C.c_int * 2)(1, 3)
                    zero = torch.zeros_like(P0)
                    ops = {"F2": IN(F2), "M2": IN(M2), "bh": IN(bh), "bw": IN(bw), "bd": IN(bd), "P": INOUT(P0), "m": INOUT(zero), "v": INOUT(zero),
                           "U": OUT((3,) + shape), "G": OUT((3,) + shape), "snap": OUT((2, 3) + shape), "ws": SCRATCH(L.cvx_adam_workspace_bytes(C_, h, w, d))}

                    def call(t):
                        return getattr(L, entry)(p(t["F2"]), p(t["M2"]), C_, h, w, d, p(t["P"]), p(t["m"]), p(t["v"]), 1.25, 3, 0, 1.0, p(t["bh"]), p(t["bw"]),
                                                 p(t["bd"]), p(t["U"]), p(t["G"]), vp(its), 2, p(t["snap"]), C.byref(sm) if smo is not None else None, last,
                                                 *ws_of(t), stream())

                    def verify(a):
                        r = orc.adam_run(npy(F2), npy(M2), npy(P0), 1.25, 3, cost_scale=1.0, want_grad=True)
                        for k in ("P", "m", "v", "U", "G"):
                            same(a[k], r[k])
                        same(a["snap"][1], r["U"])
                    return ops, call, verify if name == "exact-f32" else None
                opts = [{}]
                if name.startswith("exact") and "chain" not in name:
                    opts = [{}, {"box_fwd_tile": 0, "box_bwd_tile": 0}] + (TILE_OPTS if shape in ADAM_TILE_SHAPES else [])
                row(entry, "%s-C%d-%s" % (name, C_, "x".join(map(str, shape))), opts)(build)


adam_rows()


# ---- whole pair ----------------------------------------------------------------------------------------------------------------------
for _shape in PAIR_SHAPES:
    for _ic in (0, 1):
        for _lam in (0.0, 1.25):
            def _build_pair(L, orc, shape=_shape, ic=_ic, lam=_lam):
                H, W, D = shape
                pp = _pair(H, W, D, ic, lam, 0)
                a, b = rnd(shape, 43, 0.0, 100.0), rnd(shape, 44, 0.0, 100.0)
                oshape = (3,) + (shape if (ic or lam > 0) else tuple(s // 2 for s in shape))
                ops = {"a": IN(a), "b": IN(b), "out": OUT(oshape), "ws": SCRATCH(L.cvx_register_pair_workspace_bytes(C.byref(pp)))}
                return ops, lambda t: L.cvx_register_pair_f32(p(t["a"]), p(t["b"]), None, None, C.byref(pp), p(t["out"]), None, *ws_of(t), stream()), None
            row("cvx_register_pair_f32", "ic%d-lam%g-%s" % (_ic, _lam, "x".join(map(str, _shape))))(_build_pair)

    def _build_snap(L, orc, shape=_shape):
        H, W, D = shape
        pp = _pair(H, W, D, 1, 1.25, 0)
        its, sms = (C.c_int * 2)(1, 3), (C.c_int * 2)(0, 3)
        a, b = rnd(shape, 45, 0.0, 100.0), rnd(shape, 46, 0.0, 100.0)
        ops = {"a": IN(a), "b": IN(b), "out": OUT((2, 2, 3) + shape), "ws": SCRATCH(L.cvx_register_pair_snapshots_workspace_bytes(C.byref(pp), 2, vp(sms), 2))}
        return ops, lambda t: L.cvx_register_pair_snapshots_f32(p(t["a"]), p(t["b"]), None, None, C.byref(pp), vp(its), 2, vp(sms), 2, p(t["out"]), *ws_of(t),
                                                                stream()), None
    row("cvx_register_pair_snapshots_f32", "x".join(map(str, _shape)))(_build_snap)

    def _build_label_pair(L, orc, shape=_shape):
        H, W, D = shape
        nl = 4
        pp = _pair(H, W, D, 1, 1.25, nl)
        la, lb = labels(shape, nl, 47), torch.roll(labels(shape, nl, 47), (1, -1, 2), (0, 1, 2)).contiguous()
        present, weights = _present(nl)
        ops = {"la": IN(la), "lb": IN(lb), "present": IN(present, loud=1), "weights": IN(weights), "out": OUT((3,) + shape),
               "ws": SCRATCH(L.cvx_register_label_pair_workspace_bytes(C.byref(pp)))}
        return ops, lambda t: L.cvx_register_label_pair_f32(p(t["la"]), p(t["lb"]), p(t["present"]), p(t["weights"]), 10.0, C.byref(pp), p(t["out"]), None,
                                                            *ws_of(t), stream()), None
    row("cvx_register_label_pair_f32", "x".join(map(str, _shape)))(_build_label_pair)


# ---- evaluation ----------------------------------------------------------------------------------------------------------------------
for _c1 in (0, 1):
    for _shape in [(5, 5, 5), (7, 9, 11), (5, 6, 69)]:
        def _build_jac(L, orc, c1=_c1, shape=_shape):
            H, W, D = shape
            flow = rnd((3,) + shape, 48, -1.0, 1.0)
            ops = {"flow": IN(flow), "out": OUT((H - 4, W - 4, D - 4))}
            return ops, lambda t: L.cvx_jacobian_det_f32(p(t["flow"]), H, W, D, c1, p(t["out"]), stream()), \
                lambda a: same(a["out"], morc().jacobian_determinant_3d(npy(flow), bool(c1)).reshape(H - 4, W - 4, D - 4))
        row("cvx_jacobian_det_f32", "c%d-%s" % (_c1, "x".join(map(str, _shape))))(_build_jac)

WORD_SHAPES = [(3, 4, WORD - 1), (3, 4, WORD), (3, 4, WORD + 1), (9, 7, 12), (1, 1, 1)]

for _shape in SMALL3 + [s for s in WORD_SHAPES[:3] if s not in SMALL3]:
    _sid = "x".join(map(str, _shape))

    _wshape = tuple(max(s, 2) for s in _shape)                   # (the operator takes extents of 2 and more)

    def _build_wl(L, orc, shape=_wshape):
        H, W, D = shape
        seg = labels(shape, 5, 49)
        disp = rnd((3,) + shape, 50, -3.0, 3.0)
        bh, bw, bd = _bases(L, shape)
        torch.cuda.synchronize()
        ops = {"seg": IN(seg), "disp": IN(disp), "bh": IN(bh), "bw": IN(bw), "bd": IN(bd), "out": OUT(shape)}
        return ops, lambda t: L.cvx_warp_labels_nearest_f32(p(t["seg"]), p(t["disp"]), H, W, D, p(t["bh"]), p(t["bw"]), p(t["bd"]), p(t["out"]), stream()), \
            lambda a: same(a["out"], morc().warp_labels_nearest(npy(seg), npy(disp)).reshape(shape))
    row("cvx_warp_labels_nearest_f32", "x".join(map(str, _wshape)))(_build_wl)

    def _build_lo(L, orc, shape=_shape):
        n, nl = shape[0] * shape[1] * shape[2], 5
        a, b = labels(shape, nl, 51).reshape(-1), labels(shape, nl, 52).reshape(-1)
        ops = {"a": IN(a), "b": IN(b), "counts": OUT((3, nl), torch.int64)}
        return ops, lambda t: L.cvx_label_overlap_i64(p(t["a"]), p(t["b"]), n, nl, p(t["counts"]), stream()), None
    row("cvx_label_overlap_i64", _sid)(_build_lo)

    for _seq in ({}, {"edt_sequential": 1}):
        def _build_edt(L, orc, shape=_shape):
            H, W, D = shape
            objs = (rnd((2,) + shape, 53) > 0.4).float()
            ops = {"objs": IN(objs), "d2": OUT((2,) + shape, torch.int32), "ws": SCRATCH(L.cvx_edt_squared_workspace_bytes(2, H, W, D))}
            return ops, lambda t: L.cvx_edt_squared_i32(p(t["objs"]), 2, H, W, D, p(t["d2"]), *ws_of(t), stream()), None
        row("cvx_edt_squared_i32", _sid, [_seq])(_build_edt)

        def _build_edtl(L, orc, shape=_shape):
            H, W, D = shape
            seg = labels(shape, 3, 54)
            labs = (C.c_int * 3)(1, 2, 3)
            ops = {"seg": IN(seg), "d2": OUT((6,) + shape, torch.int32), "ws": SCRATCH(L.cvx_edt_squared_workspace_bytes(6, H, W, D))}
            return ops, lambda t: L.cvx_edt_squared_labels_i32(p(t["seg"]), H, W, D, vp(labs), 3, p(t["d2"]), *ws_of(t), stream()), None
        row("cvx_edt_squared_labels_i32", _sid, [_seq])(_build_edtl)

        def _build_sq(L, orc, shape=_shape):
            H, W, D = shape
            obj = (rnd(shape, 55) > 0.4).float()
            obj.view(-1)[0] = 0.0
            feat = torch.from_numpy(orc.feature_transform(npy(obj))).to(DEV)
            ops = {"obj": IN(obj), "feat": IN(feat, loud=min(1, min(shape) - 1)), "d2": OUT(shape, torch.int32)}
            return ops, lambda t: L.cvx_edt_sqdist_i32(p(t["obj"]), p(t["feat"]), H, W, D, p(t["d2"]), stream()), None
        row("cvx_edt_sqdist_i32", _sid, [_seq])(_build_sq)

def _bits(L, seg, nl):
    H, W, D = seg.shape
    b = torch.empty(int(L.cvx_label_bits_bytes(H, W, D, nl)) // 8, dtype=torch.int64, device=DEV)
    assert L.cvx_label_bits_u64(p(seg), H, W, D, nl, p(b), stream()) == 0
    torch.cuda.synchronize()
    return b


for _shape in WORD_SHAPES:
    _sid = "x".join(map(str, _shape))

    def _build_bits(L, orc, shape=_shape):
        H, W, D = shape
        nl = 5
        seg = labels(shape, nl, 56)
        ops = {"seg": IN(seg), "bits": OUT((int(L.cvx_label_bits_bytes(H, W, D, nl)) // 8,), torch.int64)}
        def verify(a):
            nseg = (D + WORD - 1) // WORD
            want = np.zeros((nl, H * W, nseg * WORD), np.uint8)
            for lab in range(1, nl + 1):
                want[lab - 1, :, :D] = (npy(seg) == lab).reshape(H * W, D)
            same(a["bits"], np.packbits(want.reshape(nl, H * W, nseg, WORD), axis=-1, bitorder="little").view(np.int64).reshape(-1))
        return ops, lambda t: L.cvx_label_bits_u64(p(t["seg"]), H, W, D, nl, p(t["bits"]), stream()), verify
    row("cvx_label_bits_u64", _sid)(_build_bits)

    for _entry in ("cvx_surface_distance_hist_i64", "cvx_surface_distance_hist_bits_i64"):
        def _build_sd(L, orc, shape=_shape, entry=_entry):
            H, W, D = shape
            nl = 5
            sa, sb = labels(shape, nl, 57), labels(shape, nl, 58)
            ba, bb = _bits(L, sa, nl), _bits(L, sb, nl)
            nbins = (H - 1) ** 2 + (W - 1) ** 2 + (D - 1) ** 2 + 2
            act4 = (C.c_uint64 * 4)(*[(1 << 64) - 1] * 4)
            ops = {"ba": IN(ba, loud=-1), "hist": INOUT(torch.zeros((nl, nbins), dtype=torch.int64)), "over": INOUT(torch.zeros(nl, dtype=torch.int32))}
            if entry.endswith("bits_i64"):
                ops["bb"] = IN(bb, loud=-1)
                ops["ws"] = SCRATCH(L.cvx_surface_distance_hist_bits_workspace_bytes(H, W, D, nl))
                return ops, lambda t: L.cvx_surface_distance_hist_bits_i64(p(t["bb"]), p(t["ba"]), H, W, D, nl, vp(act4), nbins, p(t["hist"]), nbins, p(t["over"]),
                                                                           1, 0, *ws_of(t), stream()), None
            ops["sb"] = IN(sb)
            return ops, lambda t: L.cvx_surface_distance_hist_i64(p(t["sb"]), p(t["ba"]), H, W, D, nl, vp(act4), nbins, p(t["hist"]), nbins, p(t["over"]), 1, 0,
                                                                  stream()), None
        row(_entry, _sid)(_build_sd)


def ssim_rows():
    from convexadam_amd.ssim import TILE
    for ws_ in (11, 3):
        for case, shape in [("ragged", ragged(TILE)), ("below", (2, 3, 5)), ("voxel", (1, 1, 1))]:
            def build(L, orc, ws_=ws_, shape=shape):
                n, c = 1, 2
                h, w, d = shape
                x, y = rnd((n, c) + shape, 59), rnd((n, c) + shape, 60)
                ops = {"x": IN(x), "y": IN(y), "map": OUT((n, c) + shape), "mean": OUT((1,)), "slice": OUT((n, d)),
                       "ws": SCRATCH(L.cvx_ssim3d_workspace_bytes(n, c, h, w, d, ws_))}
                return ops, lambda t: L.cvx_ssim3d_f32(p(t["x"]), p(t["y"]), n, c, h, w, d, ws_, p(t["map"]), p(t["mean"]), p(t["slice"]), *ws_of(t), stream()), None
            row("cvx_ssim3d_f32", "ws%d-%s" % (ws_, case))(build)


ssim_rows()

for _n, _nrhs in [(5, 1), (37, 3), (65, 4)]:
    def _tps(L, n, nrhs):
        c = rnd((n, 3), 61, -1.0, 1.0)
        f = rnd((n, nrhs), 62, -2.0, 2.0)
        return c, f

    def _build_fit(L, orc, n=_n, nrhs=_nrhs):
        c, f = _tps(L, n, nrhs)
        ops = {"c": IN(c), "f": IN(f), "theta": OUT((n + 4, nrhs)), "ws": SCRATCH(L.cvx_tps_fit_workspace_bytes(n, nrhs))}
        return ops, lambda t: L.cvx_tps_fit_f32(p(t["c"]), p(t["f"]), n, nrhs, 0.0, p(t["theta"]), *ws_of(t), stream()), None
    row("cvx_tps_fit_f32", "n%d-r%d" % (_n, _nrhs))(_build_fit)

    def _theta(L, n, nrhs):
        c, f = _tps(L, n, nrhs)
        theta = torch.empty((n + 4, nrhs), device=DEV)
        need = L.cvx_tps_fit_workspace_bytes(n, nrhs)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        assert L.cvx_tps_fit_f32(p(c), p(f), n, nrhs, 0.0, p(theta), p(ws), need, stream()) == 0
        return c, theta

    for _m in (1, 63, 257):
        def _build_eval(L, orc, n=_n, nrhs=_nrhs, m=_m):
            c, theta = _theta(L, n, nrhs)
            pts = rnd((m, 3), 63, -1.0, 1.0)
            ops = {"pts": IN(pts), "c": IN(c), "theta": IN(theta), "out": OUT((m, nrhs))}
            return ops, lambda t: L.cvx_tps_eval_f32(p(t["pts"]), m, p(t["c"]), p(t["theta"]), n, nrhs, p(t["out"]), stream()), None
        row("cvx_tps_eval_f32", "n%d-r%d-m%d" % (_n, _nrhs, _m))(_build_eval)

    for _s in [(3, 4, 5), (1, 1, 2), (2, 3, 65)]:
        def _build_dense(L, orc, n=_n, nrhs=_nrhs, s=_s):
            c, theta = _theta(L, n, nrhs)
            ops = {"c": IN(c), "theta": IN(theta), "out": OUT((nrhs,) + s)}
            return ops, lambda t: L.cvx_tps_dense_f32(*s, p(t["c"]), p(t["theta"]), n, nrhs, p(t["out"]), stream()), None
        row("cvx_tps_dense_f32", "n%d-r%d-%s" % (_n, _nrhs, "x".join(map(str, _s))))(_build_dense)

for _n, _iters in [(2, 1), (7, 5), (301, 5), (1025, 3)]:
    def _build_lts(L, orc, n=_n, iters=_iters):
        f = rnd((n, 4), 64, -20.0, 20.0)
        f[:, 3] = 1.0
        m = (f + rnd((n, 4), 65, -0.1, 0.1)).contiguous()
        m[:, 3] = 1.0
        ops = {"f": IN(f), "m": IN(m), "T": OUT((4, 4)), "inl": OUT((n,), torch.uint8), "ws": SCRATCH(L.cvx_rigid_lts_workspace_bytes(n))}
        return ops, lambda t: L.cvx_rigid_lts_f32(p(t["f"]), 4, p(t["m"]), 4, n, iters, p(t["T"]), p(t["inl"]), *ws_of(t), stream()), None
    row("cvx_rigid_lts_f32", "n%d-it%d" % (_n, _iters))(_build_lts)

for _R, _N, _S in [(1, 1, 1), (2, 5, 7), (1, 9, 65)]:
    def _build_rank(L, orc, R=_R, N=_N, S=_S):
        samples = rnd((R, N, S), 66, -1.0, 1.0, torch.float64)
        ops = {"samples": IN(samples), "scores": OUT((R, N), torch.int32), "u2": OUT((R, N, N), torch.int32)}
        return ops, lambda t: L.cvx_ranksum_better_f64(p(t["samples"]), None, 1.0, 1.0, R, N, S, S * S + 1, p(t["scores"]), p(t["u2"]), stream()), None
    row("cvx_ranksum_better_f64", "%dx%dx%d" % (_R, _N, _S))(_build_rank)


# ---- the one-thread-per-element entry points that the table makes cheap ----------------------------------------------------------------
for _n in (1, 255, 257):
    def _build_gather(L, orc, n=_n):
        src = rnd((40,), 67)
        idx = torch.randint(0, 40, (n,), generator=torch.Generator().manual_seed(68), dtype=torch.int64).to(DEV)
        ops = {"src": IN(src), "idx": IN(idx, loud=39), "out": OUT((n,))}
        return ops, lambda t: L.cvx_gather_f32(p(t["src"]), p(t["idx"]), n, p(t["out"]), stream()), lambda a: same(a["out"], npy(src)[npy(idx)])
    row("cvx_gather_f32", "n%d" % _n)(_build_gather)

    def _build_select(L, orc, n=_n):
        mask, a, b = (rnd((n,), 69) > 0.5).float(), rnd((n,), 70), rnd((n,), 71)
        ops = {"mask": IN(mask), "a": IN(a), "b": IN(b), "out": OUT((n,))}
        return ops, lambda t: L.cvx_select_f32(p(t["mask"]), p(t["a"]), p(t["b"]), n, p(t["out"]), stream()), \
            lambda r: same(r["out"], np.where(npy(mask) != 0, npy(a), npy(b)))
    row("cvx_select_f32", "n%d" % _n)(_build_select)

    def _build_round(L, orc, n=_n):
        x = rnd((n,), 72, -70000.0, 70000.0)
        return {"x": INOUT(x)}, lambda t: L.cvx_round_f16_f32(p(t["x"]), n, stream()), lambda a: same(a["x"], npy(x.half().float()))
    row("cvx_round_f16_f32", "n%d" % _n)(_build_round)

    def _build_hist(L, orc, n=_n):
        lab = labels((1, 1, n), 6, 73).reshape(-1)
        ops = {"lab": IN(lab), "hist": OUT((7,), torch.int64)}
        return ops, lambda t: L.cvx_label_histogram_i64(p(t["lab"]), n, 6, p(t["hist"]), stream()), \
            lambda a: same(a["hist"], np.bincount(npy(lab).astype(np.int64), minlength=7).astype(np.int64))
    row("cvx_label_histogram_i64", "n%d" % _n)(_build_hist)

    def _build_js(L, orc, n=_n):
        jac = rnd((n,), 74, -0.5, 2.0)
        ops = {"jac": IN(jac), "acc": OUT((3,), torch.float64)}
        return ops, lambda t: L.cvx_jacobian_stats_f64(p(t["jac"]), n, p(t["acc"]), stream()), None
    row("cvx_jacobian_stats_f64", "n%d" % _n)(_build_js)


    def _build_expf(L, orc, n=_n):
        x = rnd((n,), 75, -80.0, 0.0)
        ops = {"x": IN(x), "out": OUT((n,))}
        return ops, lambda t: L.cvx_expf_f32(p(t["x"]), p(t["out"]), n, stream()), lambda a: same(a["out"], orc.expf(npy(x)))
    row("cvx_expf_f32", "n%d" % _n)(_build_expf)

    def _build_base(L, orc, n=_n):
        return {"out": OUT((n,))}, lambda t: L.cvx_affine_base_f32(n, p(t["out"]), stream()), lambda a: same(a["out"], orc.affine_base(n))
    row("cvx_affine_base_f32", "n%d" % _n)(_build_base)

    def _build_shist(L, orc, n=_n):
        g = torch.Generator().manual_seed(76)
        a_in, a_out = (torch.randint(0, 6, (n,), generator=g, dtype=torch.int32).to(DEV) for _ in range(2))
        b_in = torch.randint(0, 3, (n,), generator=g, dtype=torch.int32).to(DEV)
        nbins = 9                                              # values 10 do not fit: the overflow flag is part of the output
        ops = {"a_in": IN(a_in, loud=1), "a_out": IN(a_out, loud=1), "b_in": IN(b_in, loud=1), "hist": OUT((nbins,), torch.int64), "over": OUT((1,), torch.int32)}
        return ops, lambda t: L.cvx_surface_hist_i64(p(t["a_in"]), p(t["a_out"]), p(t["b_in"]), n, nbins, p(t["hist"]), p(t["over"]), stream()), None
    row("cvx_surface_hist_i64", "n%d" % _n)(_build_shist)

    def _build_shist_batch(L, orc, n=_n):
        g = torch.Generator().manual_seed(77)
        vols = {"v%d" % i: IN(torch.randint(0, 3, (n,), generator=g, dtype=torch.int32).to(DEV), loud=1) for i in range(6)}
        nbins = 9
        ops = dict(vols, hist=OUT((2, nbins), torch.int64), over=OUT((2,), torch.int32))

        def call(t):
            table = torch.tensor([t["v%d" % i].data_ptr() for i in range(6)], dtype=torch.int64, device=DEV)      # (a_in2, a_out2, b_in2) per histogram
            rc = L.cvx_surface_hist_batch_i64(p(table), 2, n, nbins, p(t["hist"]), p(t["over"]), stream())
            torch.cuda.synchronize()
            return rc
        return ops, call, None
    row("cvx_surface_hist_batch_i64", "n%d" % _n)(_build_shist_batch)

    def _build_hstats(L, orc, n=_n):
        hist = torch.randint(0, 5, (n,), generator=torch.Generator().manual_seed(78), dtype=torch.int64).to(DEV)
        hist[0] = 3
        total = int(hist.sum())
        ops = {"hist": IN(hist, loud=1), "out": OUT((3,), torch.int64)}
        return ops, lambda t: L.cvx_hist_order_stats_i64(p(t["hist"]), n, 0, total - 1, p(t["out"]), stream()), None
    row("cvx_hist_order_stats_i64", "n%d" % _n)(_build_hstats)

    def _build_hperc(L, orc, n=_n):
        hist = torch.randint(0, 5, (n,), generator=torch.Generator().manual_seed(79), dtype=torch.int64).to(DEV)
        hist[0] = 3
        ops = {"hist": IN(hist, loud=1), "out": OUT((3,), torch.int64)}
        return ops, lambda t: L.cvx_hist_percentile_neighbours_i64(p(t["hist"]), n, 0.95, p(t["out"]), stream()), None
    row("cvx_hist_percentile_neighbours_i64", "n%d" % _n)(_build_hperc)

    def _build_hperc_batch(L, orc, n=_n):
        hist = torch.randint(0, 5, (3, n), generator=torch.Generator().manual_seed(80), dtype=torch.int64).to(DEV)
        hist[:, 0] = 3
        ops = {"hist": IN(hist, loud=1), "out": OUT((3, 3), torch.int64)}
        return ops, lambda t: L.cvx_hist_percentile_neighbours_batch_i64(p(t["hist"]), n, 3, 0.95, p(t["out"]), stream()), None
    row("cvx_hist_percentile_neighbours_batch_i64", "n%d" % _n)(_build_hperc_batch)

for _hw in (0, 1, 3):
    def _build_mesh(L, orc, hw=_hw):
        K = (2 * hw + 1) ** 3
        return {"out": OUT((3, K))}, lambda t: L.cvx_disp_mesh_f32(hw, p(t["out"]), stream()), lambda a: same(a["out"], orc.disp_mesh(hw))
    row("cvx_disp_mesh_f32", "hw%d" % _hw)(_build_mesh)

for _shape in SMALL3:
    _sid = "x".join(map(str, _shape))

    def _build_flat(L, orc, shape=_shape):
        H, W, D = shape
        obj = (rnd(shape, 81) > 0.4).float()
        obj.view(-1)[0] = 0.0
        feat = torch.from_numpy(orc.feature_transform(npy(obj))).to(DEV)
        ops = {"feat": IN(feat, loud=min(1, min(shape) - 1)), "out": OUT(shape, torch.int64)}
        return ops, lambda t: L.cvx_feature_flat_index_i64(p(t["feat"]), H, W, D, 2 * W, 2 * D, p(t["out"]), stream()), None
    row("cvx_feature_flat_index_i64", _sid)(_build_flat)

    for _prec in (1, 2):
        def _build_lmask(L, orc, shape=_shape, prec=_prec):
            H, W, D = shape
            seg = labels(shape, 3, 82)
            big = tuple(s * prec for s in shape)
            ops = {"seg": IN(seg), "inside": OUT(big), "outside": OUT(big), "count": OUT((1,), torch.int64)}
            return ops, lambda t: L.cvx_label_mask_f32(p(t["seg"]), H, W, D, 2, prec, p(t["inside"]), p(t["outside"]), p(t["count"]), stream()), None
        row("cvx_label_mask_f32", "p%d-%s" % (_prec, _sid))(_build_lmask)

    def _build_lmask_scaled(L, orc, shape=_shape):
        H, W, D = shape
        s_ = 1.5
        seg = labels(shape, 3, 83)
        big = tuple(int(e * s_) for e in shape)
        ops = {"seg": IN(seg), "inside": OUT(big), "outside": OUT(big), "count": OUT((1,), torch.int64)}
        return ops, lambda t: L.cvx_label_mask_scaled_f32(p(t["seg"]), H, W, D, 2, *big, float(np.float32(1.0 / s_)), p(t["inside"]), p(t["outside"]), p(t["count"]),
                                                          stream()), None
    row("cvx_label_mask_scaled_f32", _sid)(_build_lmask_scaled)

    def _build_cent(L, orc, shape=_shape):
        H, W, D = shape
        seg = labels(shape, 4, 84)
        ops = {"seg": IN(seg), "acc": OUT((5, 4), torch.int64)}
        def verify(a):
            sg = npy(seg).astype(np.int64)
            z, y, x = np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing="ij")
            same(a["acc"], np.array([[(sg == l).sum(), z[sg == l].sum(), y[sg == l].sum(), x[sg == l].sum()] for l in range(5)], np.int64))
        return ops, lambda t: L.cvx_label_centroids_i64(p(t["seg"]), H, W, D, 4, p(t["acc"]), stream()), verify
    row("cvx_label_centroids_i64", _sid)(_build_cent)

for _g, _shape in [(2, (7, 9, 11)), (3, (3, 3, 3)), (2, (5, 4, 131)), (1, (1, 1, 1))]:
    def _build_tpm(L, orc, g=_g, shape=_shape):
        H, W, D = shape
        img = rnd(shape, 85)
        ops = {"img": IN(img), "mask": OUT((H // g, W // g, D // g), torch.uint8)}
        def verify(a):
            h, w, d = H // g, W // g, D // g
            cnt = (npy(img)[:h * g, :w * g, :d * g] > np.float32(0.5)).reshape(h, g, w, g, d, g).sum((1, 3, 5))
            same(a["mask"], (2 * cnt > g ** 3).astype(np.uint8))
        return ops, lambda t: L.cvx_threshold_pool_mask_u8(p(t["img"]), H, W, D, 0.5, g, p(t["mask"]), stream()), verify
    row("cvx_threshold_pool_mask_u8", "g%d-%s" % (_g, "x".join(map(str, _shape))))(_build_tpm)


# ---- what is not a row, and why --------------------------------------------------------------------------------------------------------
HOST = "host only: no kernel is launched"
QUERY = "size query: no kernel is launched"
CONTROL = "option, context, table or profiling call: launches nothing that reads or writes an operand of the caller's"
EXCLUDED = {
    "cvx_version": HOST, "cvx_last_error": HOST, "cvx_device_count": HOST, "cvx_affine_base_host": HOST, "cvx_disp_mesh_host": HOST,
    "cvx_label_weights_host": HOST, "cvx_const_div_make": HOST, "cvx_const_div_enumerate": HOST, "cvx_const_div_mismatches": HOST,
    "cvx_ranksum_critical_u2": HOST, "cvx_box_tile_sync_errors": HOST,
    "cvx_context_create": CONTROL, "cvx_context_destroy": CONTROL, "cvx_context_bind": CONTROL, "cvx_context_set_option": CONTROL,
    "cvx_context_get_option": CONTROL, "cvx_set_option": CONTROL, "cvx_get_option": CONTROL, "cvx_last_pair_profile": CONTROL, "cvx_set_profiling": CONTROL,
    "cvx_context_set_adam_sqrt_table": "copies a 6 MiB table into memory the context owns (hipMemcpy, no kernel); pinned by the reference-bits tests",
    "cvx_set_adam_sqrt_table": "as cvx_context_set_adam_sqrt_table", "cvx_context_set_mind_exp_table": "as cvx_context_set_adam_sqrt_table",
    "cvx_set_mind_exp_table": "as cvx_context_set_adam_sqrt_table",
    "cvx_mindssc_workspace_bytes": QUERY, "cvx_mindssc_pooled_scratch_bytes": QUERY, "cvx_box_smooth_workspace_bytes": QUERY, "cvx_correlate_workspace_bytes": QUERY,
    "cvx_coupled_convex_workspace_bytes": QUERY, "cvx_inverse_consistency_workspace_bytes": QUERY, "cvx_adam_workspace_bytes": QUERY,
    "cvx_smooth_workspace_bytes": QUERY, "cvx_register_pair_workspace_bytes": QUERY, "cvx_register_label_pair_workspace_bytes": QUERY,
    "cvx_register_pair_snapshots_workspace_bytes": QUERY, "cvx_feature_transform_workspace_bytes": QUERY, "cvx_edt_squared_workspace_bytes": QUERY,
    "cvx_label_bits_bytes": QUERY, "cvx_surface_distance_hist_bits_workspace_bytes": QUERY, "cvx_tps_fit_workspace_bytes": QUERY,
    "cvx_rigid_lts_workspace_bytes": QUERY, "cvx_rigid_samples_workspace_bytes": QUERY, "cvx_convex_stage_workspace_bytes": QUERY,
    "cvx_ssim3d_workspace_bytes": QUERY, "cvx_field_mean_workspace_bytes": QUERY,
    "cvx_correlate_f32": "cvx_correlate_ex_f32 with opts == NULL (one line in correlate.hip); the ex rows with fast 0, f16 0 run the same kernels",
    "cvx_adam_run_f32": "cvx_adam_run_ex_f32 with no smoother and float32 records: the exact-f32 rows",
    "cvx_adam_run_smoother_f32": "cvx_adam_run_ex_f32 with float32 records: the chain35-f32 rows",
    "cvx_adam_run_fast_f32": "cvx_adam_run_mode_f32 with mode 1 and no smoother: the fast rows",
    "cvx_adam_run_fast_all_f32": "cvx_adam_run_mode_f32 with mode 2 and no smoother: the fast_all rows",
    "cvx_register_pairs_f32": "cvx_register_pair_f32 per pair on internal streams, operands passed through host pointer tables; its workspace contract is in "
                              "tests/test_gpu_workspace.py",
}


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.id for r in ROWS])
def test_fenced(L, orc, r):
    with option(L, **r.opts):
        operands, call, verify = r.build(L, orc)
        plain = check_fences(operands, call, DEV)
        for k, op in operands.items():                       # (a) holds no NaN: one in the loud run comes from a moat
            if op.kind in ("out", "inout") and op.dtype.is_floating_point:
                assert not bool(torch.isnan(plain[k]).any()), "the plain run's %r holds a NaN: the inputs of this row are badly chosen" % k
        if verify is not None:
            verify(plain)


def test_every_export_is_fenced_or_excused():
    from convexadam_amd._lib import SIGNATURES
    rows = {r.entry for r in ROWS}
    names = set(SIGNATURES)
    assert all(n.startswith("cvx_") for n in names)
    assert not rows - names, "rows for names the library does not export: %s" % sorted(rows - names)
    assert not set(EXCLUDED) - names, "exclusions for names the library does not export: %s" % sorted(set(EXCLUDED) - names)
    assert not rows & set(EXCLUDED), "both a row and excluded: %s" % sorted(rows & set(EXCLUDED))
    missing = names - rows - set(EXCLUDED)
    assert not missing, "exported without a fence row or a written reason: %s" % sorted(missing)
    assert all(isinstance(v, str) and len(v) > 20 for v in EXCLUDED.values())
    assert len({r.id for r in ROWS}) == len(ROWS), "duplicate row ids"
