"""The Python layer off torch's default stream (run on the MI355X box with `-m gpu`).

Every wrapper takes its stream from torch.cuda.current_stream() and its scratch from _lib.workspace(), which keys the buffers by (thread,
device, stream); until now no test called the layer anywhere but on the default stream.  One call per public module -- the one its own GPU
test makes first, on the smallest inputs that test uses -- runs inside `with torch.cuda.stream(s)` behind the delay of tests/fences.py.
Its tensor inputs start as NaN (integers: zeros) and receive their data on `s`; the result, read on `s`, must be byte-identical to the same
call on the default stream.  A wrapper that passed another stream to the library, allocated its outputs on one stream and filled them on
another, or shared scratch between streams, would differ.

Where a module's first call is not reproducible bit for bit by design, the next one of the same test stands in (convexAdam_hyper_util:
the standard deviation of jacobian_log_std_and_folding sums with atomics in free order; its folding fraction is compared, and the bytes of
jacobian_determinant_3d).  Where the first call takes host arrays the device-tensor form of the same function is used, since late inputs
are the point (fieldops.invert_field)."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fences import Delay  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def delay():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return Delay(DEV)


def to_host(r):
    """a result -> nested tuples of numpy arrays and plain values (device tensors are read on the current stream)"""
    if isinstance(r, torch.Tensor):
        return r.detach().cpu().numpy()
    if isinstance(r, np.ndarray):
        return r
    if isinstance(r, dict):
        return tuple((k, to_host(r[k])) for k in sorted(r))
    if isinstance(r, (tuple, list)):
        return tuple(to_host(v) for v in r)
    if hasattr(r, "array") and hasattr(r, "GetOrigin"):                    # an imageio.Image
        return (np.asarray(r.array), tuple(r.GetOrigin()), tuple(r.GetSpacing()))
    return r


def same(a, b, where="result"):
    if isinstance(a, tuple):
        assert isinstance(b, tuple) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (where, a.dtype, b.dtype, a.shape, b.shape)
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), "%s: the side-stream call differs from the default-stream call" % where
    elif isinstance(a, float) and np.isnan(a):
        assert isinstance(b, float) and np.isnan(b), where
    else:
        assert a == b, (where, a, b)


def stale_like(v):
    return torch.full_like(v, float("nan")) if v.is_floating_point() else torch.zeros_like(v)


def on_both_streams(delay, tensors, fn):
    """tensors: {name: device tensor}; fn(tensors) -> result.  The default-stream result, then the same call on a fresh stream behind the
    delay with inputs that are filled on that stream; both as host values."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = to_host(fn({k: v.clone() for k, v in tensors.items()}))
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    late = {k: stale_like(v) for k, v in tensors.items()}
    torch.cuda.synchronize()
    s = delay.side_stream(DEV)                           # (on another hardware queue than the default stream)
    with torch.cuda.stream(s):
        delay.enqueue(delay.ms_for(host))
        for k, v in tensors.items():
            late[k].copy_(v)
        got = to_host(fn(late))
        s.synchronize()
    torch.cuda.synchronize()
    for k, v in tensors.items():
        assert torch.equal(late[k].view(torch.uint8), v.view(torch.uint8)), "input %r was modified" % k
    same(got, want)
    return got


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


PIPELINE = dict(mind_r=1, mind_d=2, grid_sp=4, disp_hw=3, grid_sp_adam=2)


def test_convex_adam_MIND(delay, golden):
    """convex_adam_pt on the golden pipeline pair (tests/test_gpu_parity.py::test_pipeline_vs_oracle_bit_exact, first case): host arrays in,
    host field out; then register_pair_device, whose image tensors arrive late"""
    from convexadam_amd import convex_adam_MIND as M
    g = golden("pipeline")
    on_both_streams(delay, {}, lambda t: M.convex_adam_pt(g["fix"], g["mov"], dtype=torch.float32, device=torch.device(DEV), lambda_weight=0, ic=True, **PIPELINE))
    kw = dict(PIPELINE, lambda_weight=1.25, selected_niter=4, ic=True)
    on_both_streams(delay, {"fix": dev(g["fix"]), "mov": dev(g["mov"])}, lambda t: M.register_pair_device(t["fix"], t["mov"], **kw).clone())


def test_convex_adam_nnUNet(delay):
    from convexadam_amd import convex_adam_nnUNet as N
    from test_gpu_label_pooled import label_sets
    _, lf, lm = next(iter(label_sets((4, 4, 4), 2, 0)))

    def fn(t):
        lf_d, lm_d, present_d, weights_d, Cn = N._label_channels(t["lf"], t["lm"], DEV)
        return (present_d, weights_d, Cn) + tuple(N.extract_features(lf_d, lm_d, mult=10.0, device=DEV))
    on_both_streams(delay, {"lf": dev(lf.astype(np.float32)), "lm": dev(lm.astype(np.float32))}, fn)


def test_convex_adam_translation(delay):
    from convexadam_amd.convex_adam_translation import convex_adam_translation
    import translation_cases as TC
    fixed, moving, seg, _ = TC.make(TC.NAMES[0])

    def fn(t):
        tr, moved, co = convex_adam_translation(fixed, moving, segmentation=seg, co_moving_images=[moving.copy()], device=DEV)
        return tuple(float(v) for v in tr), moved, co[0]
    on_both_streams(delay, {}, fn)


def test_convex_adam_utils(delay):
    from convexadam_amd import convex_adam_utils as U
    from convexadam_amd.phantom import phantom
    img = phantom((20, 18, 23), 3, 30)
    on_both_streams(delay, {"img": img[None, None].to(DEV)}, lambda t: U.MINDSSC(t["img"], 1, 2, device=DEV))


def test_convexAdam_hyper_util(delay):
    from convexadam_amd import convexAdam_hyper_util as HU
    import test_oracle_metrics as cases
    j = cases.JAC_CASES[next(iter(cases.JAC_CASES))]()
    on_both_streams(delay, {"j": dev(j)}, lambda t: HU.jacobian_log_std_and_folding(t["j"])[1])          # (the folding fraction: an integer count)
    flow = (np.random.default_rng(15).standard_normal((3, 5, 5, 5)) * 0.1).astype(np.float32)
    on_both_streams(delay, {"flow": dev(flow)[None]}, lambda t: HU.jacobian_determinant_3d(t["flow"], False))


def test_apply_convex(delay):
    from convexadam_amd.apply_convex import apply_convex
    import test_oracle_metrics as cases
    disp, _, mov = cases.convex_trials(next(iter(cases.CONVEX_CASES)))[0]
    got = on_both_streams(delay, {}, lambda t: apply_convex(disp, mov))
    assert got.dtype == np.float64
    on_both_streams(delay, {"disp": dev(disp), "mov": dev(mov)}, lambda t: apply_convex(t["disp"], t["mov"]))


def test_rigid(delay):
    from convexadam_amd.rigid import least_trimmed_rigid
    from test_gpu_rigid import GOLDEN, TAGS
    z = np.load(GOLDEN)
    f, m = z[TAGS[0] + "_fixed"], z[TAGS[0] + "_moving"]
    on_both_streams(delay, {"f": dev(f), "m": dev(m)}, lambda t: least_trimmed_rigid(t["f"], t["m"], 1, return_inliers=True))


def test_tps(delay):
    from convexadam_amd.tps import TPS
    n = 1
    g = torch.Generator().manual_seed(n)
    c = torch.rand(n, 3, generator=g) * 2 - 1
    x = torch.rand(3000, 3, generator=g) * 2.2 - 1.1
    theta = torch.randn(n + 4, 3, generator=g) * 0.1
    on_both_streams(delay, {"x": x.to(DEV), "c": c.to(DEV), "theta": theta.to(DEV)}, lambda t: TPS.z(t["x"], t["c"], t["theta"]))


def test_ssim(delay):
    from convexadam_amd import ssim as S
    import ssim_golden
    name, wss = ssim_golden.CASES[0]
    x, y = ssim_golden.inputs(name)
    on_both_streams(delay, {"x": x.to(DEV), "y": y.to(DEV)}, lambda t: S.ssim3D_map(t["x"], t["y"], wss[0]))


def test_prep(delay):
    from convexadam_amd import prep as P
    from convexadam_amd._prep import CVX_PREP_CLAMP
    from test_gpu_prep import CT, SIZES, make
    x = make("random", SIZES[0], 1)
    on_both_streams(delay, {"x": dev(x)}, lambda t: P._stats(t["x"], CVX_PREP_CLAMP, CT["clamp_to"], CT["qs"], moments=True))


def test_fieldops(delay):
    from convexadam_amd.fieldops import invert_field
    import fieldops_restatement as R
    u = R.smooth_set()[0]
    on_both_streams(delay, {"u": dev(np.array(u))}, lambda t: invert_field(t["u"], return_info=True))


def test_geometry(delay):
    from convexadam_amd import geometry
    import geometry_restatement as G
    fixed, _, gr, _ = G.make_case(1)
    on_both_streams(delay, {"src": dev(fixed.array.astype(np.float32))}, lambda t: geometry.resample_device(t["src"], fixed, gr))


def test_cropfield(delay):
    from convexadam_amd import cropfield
    x = torch.randn((1, 3, 2, 3, 5), generator=torch.Generator().manual_seed(3))
    on_both_streams(delay, {"x": x.to(DEV)}, lambda t: cropfield.half_resolution_field(t["x"]))


def test_l2r3(delay):
    from convexadam_amd import l2r3
    samples = np.random.default_rng(1).standard_normal((1, 1, 1))
    on_both_streams(delay, {"s": dev(samples)}, lambda t: l2r3.ranksum_better(t["s"], return_u2=True))
    samples = np.random.default_rng(2).standard_normal((2, 5, 63))
    on_both_streams(delay, {"s": dev(samples)}, lambda t: l2r3.ranksum_better(t["s"], return_u2=True))


# ---- the scratch buffers -------------------------------------------------------------------------------------------------------------
def test_workspaces_are_per_stream_and_back_to_back_calls_do_not_share_them(delay):
    """A call on stream A followed at once by one on stream B, nothing synchronised in between: both results equal the serial ones, and the
    calling thread then holds a distinct _lib.workspace buffer for each of the two streams."""
    from convexadam_amd import _lib
    from convexadam_amd import convex_adam_MIND as M
    from convexadam_amd.phantom import phantom
    shape = (24, 28, 20)
    kw = dict(mind_r=1, mind_d=2, grid_sp=2, disp_hw=2, grid_sp_adam=2, lambda_weight=1.25, selected_niter=3, ic=True)
    pairs = [(phantom(shape, 1, 10 + i).to(DEV), torch.roll(phantom(shape, 1, 20 + i), (1, -1, 2), (0, 1, 2)).to(DEV)) for i in range(2)]
    serial = [M.register_pair_device(f, m, **kw).clone() for f, m in pairs]
    torch.cuda.synchronize()
    assert not torch.equal(serial[0], serial[1])
    late = [(stale_like(f), stale_like(m)) for f, m in pairs]
    a = delay.side_stream(DEV)
    b = delay.side_stream(DEV, apart_from=[a])           # (on another hardware queue than A: B's kernels can run while A is held back)
    assert a.cuda_stream != b.cuda_stream
    torch.cuda.synchronize()
    outs = []
    for s, (f, m), (lf, lm) in zip((a, b), pairs, late):
        with torch.cuda.stream(s):
            delay.enqueue(delay.floor_ms)
            lf.copy_(f)
            lm.copy_(m)
            outs.append(M.register_pair_device(lf, lm, **kw))
    with torch.cuda.stream(a):
        got_a = outs[0].cpu()
    with torch.cuda.stream(b):
        got_b = outs[1].cpu()
    torch.cuda.synchronize()
    assert torch.equal(got_a.view(torch.int32), serial[0].cpu().view(torch.int32)), "the call on stream A differs from the serial one"
    assert torch.equal(got_b.view(torch.int32), serial[1].cpu().view(torch.int32)), "the call on stream B differs from the serial one"
    held = _lib._tls.workspaces
    keys = {k: v for k, v in held.items() if k[1] in (a.cuda_stream, b.cuda_stream)}
    assert len(keys) == 2, "expected one scratch buffer per stream, found keys %s" % sorted(held)
    bufs = list(keys.values())
    assert bufs[0].data_ptr() != bufs[1].data_ptr() and bufs[0].untyped_storage().data_ptr() != bufs[1].untyped_storage().data_ptr()
    lo = [(t.data_ptr(), t.data_ptr() + t.numel()) for t in bufs]
    assert lo[0][1] <= lo[1][0] or lo[1][1] <= lo[0][0], "the two streams' scratch buffers overlap"
