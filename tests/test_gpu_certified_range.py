"""The certified correlation path (the three fast kernels and certify.hip's decisions) over float32's range and at NaNs:
every input of tests/certified_cases.py -- inside the input contract of INTEGRATION.md -- through the certified operator with each kernel
that takes its shape, and the pair cases through the whole-pair entry point.  tests/test_gpu_certified.py feeds the path values in [0, 1).

Per plain case and kernel, against the CPU oracle (which equals the reference's captures on these inputs, test_certified_cases_reference.py):
  * argmin        array_equal with the oracle's -- where ATen's denormal roundings create and break ties only the exact evaluator's
                  restatement of those roundings gets it right;
  * enclosure     cert_lower(ssdu) <= ssd <= cert_upper(ssdu) for every entry that is no NaN: the invariant every certified decision
                  rests on, with certify.hip's own constants (restated in certified_cases.py, held against the file's text on the CPU);
  * distance      |ssdu / 729 - ssd| <= 2^-17 ssd, the proven bound, where the whole volume is at or above 2^-100;
  * zero pattern  ssdu == 0 => ssd == 0 everywhere, <=> where the positive entries are at or above 2^-100;
  * NaN pattern   isnan(ssdu) == isnan(ssd) entry by entry.
Pair cases: register_pair_device with corr_cert 1, 2 and 0 gives the oracle's field bit for bit, three times the same."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import certified_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_REL = 2.0 ** -17
NORMAL_FROM = 2.0 ** -100
# (name, {option: value}, smallest C): the role kernel of corrfused.hip, the staged kernel of corrcert.hip, the round-1 pair k_corr_raw<fast> + corrbox.hip FAST
KERNELS = (("role", {"corr_cert": 1}, 1), ("staged", {"corr_cert": 2}, 1), ("round1", {"corr_cert": 1, "cert_unfused": 2}, 16))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def U():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import convex_adam_utils
    return convex_adam_utils


@pytest.fixture(scope="module")
def L():
    from convexadam_amd import _lib
    return _lib.lib()


@contextlib.contextmanager
def option(L, name, value):
    """Sets a library option for the duration of a with-block and restores the previous value."""
    old = L.cvx_get_option(name.encode())
    assert L.cvx_set_option(name.encode(), value) == 0
    try:
        yield
    finally:
        L.cvx_set_option(name.encode(), old)


@contextlib.contextmanager
def options(L, values):
    with contextlib.ExitStack() as st:
        for k, v in values.items():
            st.enter_context(option(L, k, v))
        yield


def certified(U, L, f, m, hw, opts):
    """(ssdu, argmin) on the host, or None where no certified kernel takes the shape under these options"""
    from convexadam_amd._lib import CvxError, CVX_ERR_UNSUPPORTED
    C, shape = f.shape[0], f.shape[1:]
    with options(L, opts):
        try:
            ssdu, am = U.correlate(dev(f)[None], dev(m)[None], hw, 1, shape, C, mode="certified")
        except CvxError as e:
            assert e.code == CVX_ERR_UNSUPPORTED, e
            return None
    return host(ssdu), host(am)


def check_volume(tag, ssdu, am, rs, ra):
    assert ssdu.dtype == np.float32 and ssdu.shape == rs.shape
    wrong = int((am != ra).sum())
    assert wrong == 0, "%s: %d of %d argmins differ from the oracle's" % (tag, wrong, ra.size)
    nan = np.isnan(rs)
    assert np.array_equal(np.isnan(ssdu), nan), "%s: NaN pattern differs in %d entries" % (tag, int((np.isnan(ssdu) != nan).sum()))
    ok = ~nan
    lo, hi = CC.cert_lower(ssdu), CC.cert_upper(ssdu)
    out = ok & ~((lo <= rs) & (rs <= hi))
    assert not out.any(), "%s: %d entries outside their interval, the first: ssdu %r ssd %r in [%r, %r]" % (
        (tag, int(out.sum())) + tuple(a[out][0] for a in (ssdu, rs, lo, hi)))
    assert not (ok & (ssdu == 0) & (rs != 0)).any(), "%s: a zero of the fast volume where the oracle is positive" % tag
    ref = rs[ok].astype(np.float64)
    got = ssdu[ok].astype(np.float64) / CC.BOXES
    pos = ref[ref > 0]
    if pos.size and float(pos.min()) >= NORMAL_FROM:
        assert np.array_equal(got == 0, ref == 0), "%s: exact zeros differ" % tag
    rel = float((np.abs(got - ref)[ref > 0] / pos).max()) if pos.size else 0.0
    print("CERT_RANGE %s max_rel %.4g min_pos %.4g" % (tag, rel, float(pos.min()) if pos.size else 0.0))
    if ref.size and float(ref.min()) >= NORMAL_FROM:
        assert bool((np.abs(got - ref) <= E_REL * ref).all()), "%s: distance %g of the proven 2^-17" % (tag, rel)


_oracle_cache = {}


def oracle_volume(orc, name):
    if name not in _oracle_cache:
        _, C, shape, hw, f, m = CC.case(name)
        rs, ra = orc.correlate(f, m, hw)
        rs.setflags(write=False); ra.setflags(write=False)
        _oracle_cache[name] = (rs, ra)
    return _oracle_cache[name]


@pytest.mark.parametrize("name", CC.NAMES)
def test_certified_volume_and_argmin(U, L, orc, name):
    _, C, shape, hw, f, m = CC.case(name)
    rs, ra = oracle_volume(orc, name)
    ran = []
    for kernel, opts, c_min in KERNELS:
        if C < c_min:
            continue
        got = certified(U, L, f, m, hw, opts)
        if got is None:
            continue
        ran.append(kernel)
        check_volume("%s %s" % (name, kernel), got[0], got[1], rs, ra)
    assert ran, "no certified kernel took this shape"
    if C >= 16:
        assert "round1" in ran, "the round-1 pair must take every C >= 16 shape of the list"


def pair_field(L, f, m, cert):
    from convexadam_amd.convex_adam_MIND import register_pair_device
    with option(L, "corr_cert", cert):
        return np.moveaxis(host(register_pair_device(feat_fixed=f, feat_moving=m, **CC.PAIR_KW)), 0, -1).astype(np.float64)


@pytest.mark.parametrize("name", CC.PAIR_NAMES)
def test_certified_coupled_passes(L, orc, name):
    """The plain argmin and the six coupled passes of both directions: the share of decisions the intervals leave to the exact evaluator, and
    whether the admissible box is the whole search range, depend on the volume's scale against the penalties' -- the field must not."""
    _, f, m = CC.pair(name)
    ref = orc.convex_adam_pipeline(None, None, features=(f, m), **CC.PAIR_KW)
    fd, md = dev(f), dev(m)
    outs = []
    for cert in (1, 2, 0):
        outs.append(pair_field(L, fd, md, cert))
        assert np.array_equal(outs[-1], ref), "%s, corr_cert = %d: %d field values differ from the oracle's (max %g)" % (
            name, cert, int((outs[-1] != ref).sum()), np.nanmax(np.abs(outs[-1] - ref)))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize("name", ["pair_textured@e-66"])
def test_certified_pair_on_a_side_stream_at_an_odd_address(L, orc, name):
    """The same pair with the features one element behind the 256-byte boundary (no 16-byte loads from them), arriving late on a side stream
    behind the delay of tests/fences.py: the certified passes' launches all follow the caller's stream."""
    from fences import Delay, fenced
    _, f, m = CC.pair(name)
    ref = orc.convex_adam_pipeline(None, None, features=(f, m), **CC.PAIR_KW)
    delay = Delay(DEV)
    late = {k: fenced(a.shape, torch.float32, DEV, float("nan"), shift=4) for k, a in (("f", f), ("m", m))}
    for t in late.values():
        assert t.data_ptr() % 256 == 4
        t.fence.snapshot()
    staged = {"f": dev(f), "m": dev(m)}
    torch.cuda.synchronize()
    s = delay.side_stream(DEV)
    with torch.cuda.stream(s):
        delay.enqueue(delay.floor_ms)
        for k in late:
            late[k].copy_(staged[k])
        out = pair_field(L, late["f"], late["m"], 1)            # (reads the result on `s`)
        s.synchronize()
    torch.cuda.synchronize()
    for k, t in late.items():
        assert t.fence.moats_intact() is None, "the moats of %r changed" % k
        assert torch.equal(t.view(torch.uint8), staged[k].view(torch.uint8)), "input %r was modified" % k
    assert np.array_equal(out, ref), "%d field values differ from the oracle's" % int((out != ref).sum())
