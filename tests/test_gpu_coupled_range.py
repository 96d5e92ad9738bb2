"""The coupled-convex stage on the device over float32's range, at costs of either sign, at -Inf and at bounds that overflow: every cost
volume of tests/coupled_range_cases.py, with its true first-minimum seed and with a foreign one, through every path of csrc/convex.hip
that takes it, each result equal byte for byte to the CPU oracle's coupled_convex on the values the kernel sees.  The oracle equals the
upstream function on these inputs (tests/test_coupled_range_reference.py); test_gpu_parity.py, test_gpu_coupled_plan.py and
test_gpu_fp16_edges.py feed the same kernels costs in [0, 1), +Inf and NaN.

  cvx_coupled_convex_f32         defaults; no_prune = 1 (k_argmin / k_argmin4 stream every pass); prune_stream_above = 2^30 (cand_box decides
                                 every voxel: k_argmin_voxel, k_argmin_wave); prune_stream_above = 0 (argmin4_stream in every pass);
                                 prune_refine = 0 (no second bound)
  cvx_coupled_convex_masked_f32  the masked cases under the defaults, no_prune = 1 and prune_stream_above = 2^30: the columns of dropped cells hold NaN, -Inf and 3e38
                                 and must not be read
  cvx_coupled_convex_f16         the cases built from half values (-Inf, zeros of both signs, signed noise at scale 1), in all five option sets
  the library's minimum pass     through convex_adam_utils.coupled_convex with both seeds: smin and the first-NaN winners come from the
                                 library's own plain argmin (k_argmin<false> / k_argmin4<false>, keys, k_keys_to_min), never from the seed --
                                 the two results agree wherever the oracle's two results agree.  (No entry point exposes the plain argmin of
                                 a caller's volume, so it is reached through the stage.)
  the large geometry             16x20x16: slices of two displacements in the plain and the streamed argmin, under the defaults, no_prune = 1
                                 and prune_stream_above = 2^30
Every operator call runs twice into an output pre-filled with 0xA5 bytes and must give the same bytes both times.  One test per path runs
every case of the table that applies (a failure names its cases); the last test holds every path to every class of the table it admits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coupled_range_cases as CC  # noqa: E402
from test_gpu_fp16_edges import dev, host, option  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPTION_SETS = {"defaults": ("no_prune", 0), "no_prune": ("no_prune", 1), "boxes_decide": ("prune_stream_above", 1 << 30),
               "every_pass_streams": ("prune_stream_above", 0), "no_refine": ("prune_refine", 0)}
SMALL = [c for c in CC.CASES if not c.large and not c.masked]
MASKED = [c for c in CC.CASES if c.masked]
HALF = [c for c in SMALL if c.half_ok()]
LARGE = [c for c in CC.CASES if c.large]
RAN = {}                        # path -> set of classes it compared


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _lib
    return _lib.lib()


_want, _dev = {}, {}


def oracle_field(orc, c, which):
    """the oracle's field of a case and seed on the values the kernel sees: computed once, read-only"""
    if (c.name, which) not in _want:
        f = orc.coupled_convex(np.array(c.seen()), np.array(c.seed(which)), orc.disp_mesh(c.hw), c.hw)
        f.setflags(write=False)
        _want[c.name, which] = f
    return _want[c.name, which]


def on_device(key, make):
    if key not in _dev:
        _dev[key] = make()
    return _dev[key]


def operands(orc, L, c, half):
    """(volume, mesh, mask or None, workspace, its size) on the device: uploaded once per case, the workspace filled with 0xA5 once"""
    if half:
        assert c.half_ok()
        vol = on_device((c.name, "half"), lambda: dev(c.ssd().astype(np.float16)))
        assert vol.dtype == torch.float16 and np.array_equal(host(vol).astype(np.float32), c.ssd(), equal_nan=True)
    else:
        vol = on_device((c.name, "f32"), lambda: dev(c.ssd()))
        assert vol.dtype == torch.float32
    mesh = on_device(("mesh", c.hw), lambda: dev(orc.disp_mesh(c.hw)))
    mask = on_device((c.name, "mask"), lambda: dev(c.mask)) if c.masked else None
    n = L.cvx_coupled_convex_workspace_bytes(*c.shape, c.hw)
    ws = on_device(("ws", c.shape, c.hw), lambda: torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV))
    return vol, mesh, mask, ws, n


def run_twice(orc, L, c, which, half=False):
    """the entry point of the case's kind, twice, each time into an output of 0xA5 bytes -> (field, None) or (None, what differed)"""
    from convexadam_amd import _lib
    vol, mesh, mask, ws, n = operands(orc, L, c, half)
    am = on_device((c.name, "seed", which), lambda: dev(c.seed(which)))
    got = []
    for _ in range(2):
        out = torch.empty((3,) + c.shape, dtype=torch.float32, device=DEV)
        out.view(torch.uint8).fill_(0xA5)
        tail = (*c.shape, c.hw, _lib.ptr(out), _lib.ptr(ws), n, _lib.stream_ptr(DEV))
        if c.masked:
            rc = L.cvx_coupled_convex_masked_f32(_lib.ptr(vol), _lib.ptr(am), _lib.ptr(mesh), _lib.ptr(mask), *tail)
        else:
            rc = (L.cvx_coupled_convex_f16 if half else L.cvx_coupled_convex_f32)(_lib.ptr(vol), _lib.ptr(am), _lib.ptr(mesh), *tail)
        if rc != 0:
            return None, "status %d: %s" % (rc, L.cvx_last_error())
        got.append(host(out))
    if got[0].tobytes() != got[1].tobytes():
        return None, "two runs differ in %d of %d values" % (int((got[0].view(np.uint32) != got[1].view(np.uint32)).sum()), got[0].size)
    return got[0], None


def describe(got, want):
    bad = got.view(np.uint32) != want.view(np.uint32)
    i = tuple(int(v[0]) for v in np.nonzero(bad))
    return "%d of %d values differ (%d voxels), the first at %r: %r vs the oracle's %r" % (
        int(bad.sum()), want.size, int(bad.any(0).sum()), i, got[i], want[i])


def compare(orc, L, cases, path, opt, half=False):
    errors = []
    for c in cases:
        for which in CC.SEEDS:
            want = oracle_field(orc, c, which)
            with option(L, *opt):
                got, err = run_twice(orc, L, c, which, half)
            if err is None and got.tobytes() != want.tobytes():
                err = describe(got, np.array(want))
            if err is not None:
                errors.append("%s, %s seed, %s: %s" % (c.name, which, path, err))
        RAN.setdefault(path, set()).add(c.cls)
    assert not errors, "%d failures over %d cases x 2 seeds, the first:\n%s" % (len(errors), len(cases), "\n".join(errors[:16]))


@pytest.mark.parametrize("opts", list(OPTION_SETS))
def test_float32_operator(L, orc, opts):
    compare(orc, L, SMALL, "f32/" + opts, OPTION_SETS[opts])


@pytest.mark.parametrize("opts", ["defaults", "no_prune", "boxes_decide"])
def test_masked_operator(L, orc, opts):
    """the result is the oracle's on ssd * mask with clean zeros: nothing of a dropped cell's column (NaN, -Inf, 3e38) reaches it"""
    for c in MASKED:
        assert not np.isfinite(c.ssd().reshape(c.K, -1)[:, c.mask.reshape(-1) == 0]).all() and np.isfinite(c.seen()).all() == ("neginf" not in c.kind)
    compare(orc, L, MASKED, "masked/" + opts, OPTION_SETS[opts])


@pytest.mark.parametrize("opts", list(OPTION_SETS))
def test_half_operator(L, orc, opts):
    """-Inf (beside +Inf and NaN in one column), zeros of both signs and signed noise as half storage: the values are half values already"""
    assert any(np.isneginf(c.ssd()).any() and np.isposinf(c.ssd()).any() for c in HALF)
    compare(orc, L, HALF, "f16/" + opts, OPTION_SETS[opts], half=True)


def test_the_minimum_pass_does_not_depend_on_the_seed(L, orc):
    """Through the Python operator, defaults: the lower bound smin and the first NaN of a column come from the library's own plain argmin of
    the volume.  Both seeds give the oracle's field, and the two fields agree wherever the oracle's two fields agree."""
    from convexadam_amd import convex_adam_utils as U
    errors = []
    for c in SMALL:
        vol, mesh, _, _, _ = operands(orc, L, c, False)
        got = {}
        for which in CC.SEEDS:
            got[which] = host(U.coupled_convex(vol, dev(c.seed(which)), mesh[:, :, None], 1, c.shape))[0]
            want = np.array(oracle_field(orc, c, which))
            if got[which].tobytes() != want.tobytes():
                errors.append("%s, %s seed: %s" % (c.name, which, describe(got[which], want)))
        must = oracle_field(orc, c, "true").view(np.uint32) == oracle_field(orc, c, "foreign").view(np.uint32)
        differ = (got["true"].view(np.uint32) != got["foreign"].view(np.uint32)) & must
        if differ.any():
            errors.append("%s: the seeds' fields differ at %d values where the oracle's agree" % (c.name, int(differ.sum())))
        RAN.setdefault("minimum_pass", set()).add(c.cls)
    assert not errors, "%d failures over %d cases, the first:\n%s" % (len(errors), len(SMALL), "\n".join(errors[:16]))


@pytest.mark.parametrize("opts", ["defaults", "no_prune", "boxes_decide"])
def test_large_geometry(L, orc, opts):
    """(boxes_decide beyond the defaults: at a few thousand voxels of noise the default budget still sends most passes to the stream)"""
    assert all(CC.k_slices(int(np.prod(c.shape)), c.K)[0] >= 2 for c in LARGE) and len(LARGE) == 5
    compare(orc, L, LARGE, "large/" + opts, OPTION_SETS[opts])


def test_every_path_ran_every_class_it_admits():
    """(last in the file: the tests above record what they compared)"""
    every = set(CC.CLASSES) - {"masked"}
    assert {c.cls for c in SMALL} == every and {c.cls for c in MASKED} == {"masked"}
    for opts in OPTION_SETS:
        assert RAN.get("f32/" + opts) == every, (opts, sorted(every - RAN.get("f32/" + opts, set())))
        assert RAN.get("f16/" + opts) == {"neg_inf", "signed_zeros", "signed"}, opts
    assert RAN.get("minimum_pass") == every
    for opts in ("defaults", "no_prune", "boxes_decide"):
        assert RAN.get("masked/" + opts) == {"masked"}, opts
        assert RAN.get("large/" + opts) == {"scaled_noise", "real_minimum", "offset_spread", "signed"}, opts
    assert len(RAN) == 5 + 5 + 1 + 3 + 3
