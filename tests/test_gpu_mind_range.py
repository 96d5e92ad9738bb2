"""MIND-SSC on the device over float32's range and at non-finite voxels: every input of tests/mind_range_cases.py through every kernel path
that takes its shape, bit-equal to the CPU oracle with NaNs in the same places.  The oracle equals the reference on these
inputs (tests/test_mind_range_reference.py); tests/test_gpu_mind_single.py feeds the same kernels mid-range, finite values.

Full descriptor (cvx_mindssc_f32): the default plan, option mind_tiled = 1 (k_mind instead of the marching stencil), an output that is not
16-byte aligned (k_mind + the scalar k_mind_finish<1>), option mind_mean_threads = 8 against the oracle's set_mean_threads(8) (torch's own
mean: all ones where the sum of the variances overflows).
Pooled (cvx_mindssc_pooled_f32): windows (6,2), (4,2), (2,0) under mind_single 0, 1, 2 and mind_blocked = 0.  A non-finite voxel under
mind_single = 1: k_mind_repair recomputes EVERY block (NaN clamp bounds).
Exact-mean paths: the outputs for base 2^-40 and base 2^40 are byte-equal to the output for base.
One test per path runs every case of the table (a failure names its cases).  No case is skipped: the last test holds every path to every
input class of the table."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mind_range_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# name -> (options, the oracle's mean threads, output offset in floats)
FULL_PATHS = {"default": ({}, 0, 0), "tiled": ({"mind_tiled": 1}, 0, 0), "unaligned_out": ({}, 0, 1), "mean8": ({"mind_mean_threads": 8}, 8, 0)}
WINDOWS = ((6, 2), (4, 2), (2, 0))
POOLED_PATHS = {"two_pass": {"mind_single": 0}, "single": {"mind_single": 1}, "repair_all": {"mind_single": 2}, "planar": {"mind_single": 0, "mind_blocked": 0}}
RAN = {}                        # path -> set of (class, shape tag) it compared


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def same(a, b):
    """equal values, NaNs in the same places (the payload of a NaN is not compared), as in test_gpu_mind_single.py"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _lib
    return _lib.lib()


@contextlib.contextmanager
def options(L, values):
    """Sets library options for the duration of a with-block and restores the previous values."""
    old = {k: L.cvx_get_option(k.encode()) for k in values}
    try:
        for k, v in values.items():
            assert L.cvx_set_option(k.encode(), v) == 0, k
        yield
    finally:
        for k, v in old.items():
            L.cvx_set_option(k.encode(), v)


_oracle = {}


def oracle_descriptor(orc, c, threads=0):
    """the oracle's descriptor of a case, computed once per mean mode and left unchanged"""
    if (c.name, threads) not in _oracle:
        orc.set_mean_threads(threads)
        try:
            m = orc.mindssc(c.img, c.radius, c.dilation)
        finally:
            orc.set_mean_threads(0)
        m.setflags(write=False)
        _oracle[c.name, threads] = m
    return _oracle[c.name, threads]


_pooled = {}


def oracle_pooled(orc, c, g):
    if (c.name, g) not in _pooled:
        _pooled[c.name, g] = orc.avgpool_stride(oracle_descriptor(orc, c), g)
    return _pooled[c.name, g]


def full_descriptor(L, c, out_offset):
    """cvx_mindssc_f32 into a view `out_offset` floats into a buffer filled with 7.0 (NaN is a legitimate result here): nothing around the view changes"""
    from convexadam_amd import _lib
    H, W, D = c.shape
    V = H * W * D
    nws = L.cvx_mindssc_workspace_bytes(H, W, D, c.radius, c.dilation)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    buf = torch.full((12 * V + 8,), 7.0, dtype=torch.float32, device=DEV)
    out = buf[out_offset:out_offset + 12 * V]
    assert out.data_ptr() % 16 == 4 * out_offset
    x = dev(c.img)
    rc = L.cvx_mindssc_f32(_lib.ptr(x), H, W, D, c.radius, c.dilation, _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0, L.cvx_last_error()
    assert bool((buf[:out_offset] == 7.0).all()) and bool((buf[out_offset + 12 * V:] == 7.0).all()), "written around the output"
    return host(out).reshape(12, H, W, D)


def describe(got, ref):
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    i = tuple(int(v[0]) for v in np.nonzero(bad))
    return "%d of %d values differ (NaNs: %d vs the oracle's %d), the first at %r: %r vs %r" % (
        int(bad.sum()), ref.size, int(np.isnan(got).sum()), int(np.isnan(ref).sum()), i, got[i], ref[i])


def report(errors, ncases):
    assert not errors, "%d failures over %d cases, the first:\n%s" % (len(errors), ncases, "\n".join(errors[:12]))


# One test per PATH, every case of the table inside it (the case is named in each message): the table has 106 cases and the suite's
# report one line per test.
@pytest.mark.parametrize("path", list(FULL_PATHS))
def test_full_descriptor(L, orc, path):
    opts, threads, off = FULL_PATHS[path]
    errors, base_bytes = [], {}
    for c in MC.CASES:
        ref = oracle_descriptor(orc, c, threads)
        with options(L, opts):
            got = full_descriptor(L, c, off)
        if not same(got, ref):
            errors.append("%s, %s: %s" % (c.name, path, describe(got, ref)))
        if c.cls == "nonfinite" and not np.isnan(got).all():
            errors.append("%s, %s: %d values are not NaN" % (c.name, path, int((~np.isnan(got)).sum())))
        # exact mean: the descriptors of base 2^-40 and base 2^40 are byte-equal to that of base (the table lists base first)
        if c.cls == "control":
            base_bytes[MC.tag(c.shape)] = got.tobytes()
        if c.cls == "pow2" and threads == 0 and got.tobytes() != base_bytes[MC.tag(c.shape)]:
            errors.append("%s, %s: not the bytes of base" % (c.name, path))
        RAN.setdefault("full/" + path, set()).add((c.cls, MC.tag(c.shape)))
    assert threads != 0 or len(base_bytes) == len(MC.SHAPES)
    report(errors, len(MC.CASES))


def poolable(c):
    return c.shape[2] % 2 == 0          # the pooled kernels read 8-byte row segments: 7x9x15 and 9x9x33 have no pooled path


POOLED_CASES = [c for c in MC.CASES if poolable(c)]


@pytest.mark.parametrize("path", list(POOLED_PATHS))
def test_pooled(L, orc, path):
    from convexadam_amd import convex_adam_utils as U
    errors, base_bytes = [], {}
    for c in POOLED_CASES:
        x = dev(c.img)[None, None]
        for g1, g2 in WINDOWS:
            with options(L, POOLED_PATHS[path]):
                single = L.cvx_mindssc_pooled_scratch_bytes(*c.shape, c.radius, c.dilation, g1, g2) == 0
                out = U.mind_pooled(x, c.radius, c.dilation, g1, g2, device=DEV, return_repairs=True)
            where = "%s, %s, windows (%d, %d)" % (c.name, path, g1, g2)
            for o, g in zip(out[:-1], (g1, g2)):
                got, ref = host(o)[0], oracle_pooled(orc, c, g)
                if not same(got, ref):
                    errors.append("%s, window %d: %s" % (where, g, describe(got, ref)))
                if c.cls == "nonfinite" and not np.isnan(got).all():
                    errors.append("%s, window %d: %d values are not NaN" % (where, g, int((~np.isnan(got)).sum())))
            # the single pass runs at radius 1, dilation 2, rows of a multiple of 4 voxels, and only where the option asks for it
            if single != (path in ("single", "repair_all") and (c.radius, c.dilation) == (1, 2) and c.shape[2] % 4 == 0):
                errors.append("%s: single pass %r" % (where, single))
            nblk = int(np.prod([-(-s // g1) for s in c.shape]))
            if not single and out[-1] != 0:
                errors.append("%s: %d blocks repaired without the single pass" % (where, out[-1]))
            if single and (path == "repair_all" or c.cls == "nonfinite") and out[-1] != nblk:
                errors.append("%s: %d of %d blocks repaired" % (where, out[-1], nblk))
            # every pooled path has the exact mean: base 2^-40 and base 2^40 give the bytes of base
            b = b"".join(host(o).tobytes() for o in out[:-1])
            if c.cls == "control":
                base_bytes[MC.tag(c.shape), g1, g2] = b
            if c.cls == "pow2" and b != base_bytes[MC.tag(c.shape), g1, g2]:
                errors.append("%s: not the bytes of base" % where)
        RAN.setdefault("pooled/" + path, set()).add((c.cls, MC.tag(c.shape)))
    assert len(base_bytes) == 4 * len(WINDOWS)
    report(errors, len(POOLED_CASES))


def test_every_path_ran_every_class_its_plan_admits():
    """(last in the file: the tests above record what they compared)  A class is admitted at a shape if the table has a case of it there --
    the sum-overflow case needs voxels, 36x32x32 carries nothing else -- and a pooled path admits the shapes with an even D."""
    table = {(c.cls, MC.tag(c.shape)) for c in MC.CASES}
    assert {cls for cls, _ in table} == set(MC.CLASSES)
    for path in FULL_PATHS:
        assert RAN.get("full/" + path) == table, (path, sorted(table - RAN.get("full/" + path, set())))
    pooled = {(c.cls, MC.tag(c.shape)) for c in MC.CASES if poolable(c)}
    assert {cls for cls, _ in pooled} == set(MC.CLASSES) and {t for _, t in pooled} == {"12x14x64", "13x19x92", "6x6x6", "9x10x12", "36x32x32"}
    for path in POOLED_PATHS:
        assert RAN.get("pooled/" + path) == pooled, (path, sorted(pooled - RAN.get("pooled/" + path, set())))
