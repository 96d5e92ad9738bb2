"""CPU checks of the soft cost-volume statistics, no device needed: the header the kernels compile
(csrc/softstats_core.h) run on the host under AddressSanitizer and UndefinedBehaviorSanitizer -- a stand-alone program,
tools/softstats_host.cpp, with the sanitizer runtimes linked in and started as a child process, so that no library has to be preloaded
anywhere -- against the numpy restatement bit for bit; the restatement against known answers and against an independent float64
evaluation, inside the bound that softstats_restatement.reference_bound derives."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softstats_restatement as R  # noqa: E402
from oracle import oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the host-arithmetic test needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("softstats_host") / "softstats_host")
    header = os.path.join(ROOT, "convexadam_amd", "csrc", "softstats_core.h")
    assert os.path.exists(header), "csrc/softstats_core.h: the per-column arithmetic as a plain-C++ header"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.dirname(header), os.path.join(ROOT, "tools", "softstats_host.cpp"), "-o", exe]
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run(cmd + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode == 0:
            return exe
    raise AssertionError("%s\n%s" % (" ".join(cmd), r.stdout))


def _run(exe, args, tmp, inputs, nbytes):
    paths = []
    for i, a in enumerate(inputs):
        paths.append(os.path.join(tmp, "in%d.bin" % i))
        np.ascontiguousarray(a).tofile(paths[-1])
    out = os.path.join(tmp, "out.bin")
    r = subprocess.run([exe] + [str(a) for a in args] + paths + [out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "", "softstats_host %s: exit %d\n%s" % (args, r.returncode, r.stderr[-4000:])
    raw = open(out, "rb").read()
    assert len(raw) == nbytes
    return raw


def host_stats(exe, tmp, ssd, hw, beta, field=None, coupling=0.0):
    grid = ssd.shape[1:]
    V = int(np.prod(grid))
    half = ssd.dtype == np.float16
    args = ["stats", *grid, hw, int(half), int(field is not None), repr(float(F(coupling))), repr(float(F(beta)))]
    raw = _run(exe, args, tmp, [ssd] + ([field] if field is not None else []), 48 * V + 8)
    return np.frombuffer(raw, F, 12 * V).reshape((12,) + tuple(grid)), int(np.frombuffer(raw, np.int64, 1, 48 * V)[0])


def expf_arguments():
    """float32 arguments in [-104, 0]: a dense sweep, the ends, both zeros, and the neighbours of every reduction boundary (q + 1/2) ln 2,
    where rint(d / ln 2) steps, and of every q ln 2"""
    parts = [np.linspace(-104.0, 0.0, 200001).astype(F), np.array([-104.0, -0.0, 0.0, -87.33655, -87.5, -1e-30, -1e-45], F)]
    for scale in (np.arange(0, 151) + 0.5, np.arange(0, 151)):
        b = (-(scale * np.log(2.0))).astype(F)
        parts += [b, np.nextafter(b, F(0.0)), np.nextafter(b, F(-200.0)), np.nextafter(np.nextafter(b, F(-200.0)), F(-200.0))]
    x = np.concatenate(parts)
    return x[(x >= F(-104.0)) & (x <= F(0.0))]


def test_soft_expf_equals_the_oracle_bit_for_bit(host_program, tmp_path):
    x = expf_arguments()
    assert x.size > 200000 and x.min() == F(-104.0) and x.max() == F(0.0)
    raw = _run(host_program, ["expf", x.size], str(tmp_path), [x], 4 * x.size)
    assert same_bits(np.frombuffer(raw, F), oracle.expf(x))


def test_host_arithmetic_under_sanitizers_equals_the_restatement(host_program, tmp_path):
    cases = R.bit_cases()
    assert len(cases) == 80
    for name, ssd, hw, beta, field, coupling in cases:
        want, bad = R.soft_stats(ssd, hw, beta, field, coupling)
        got, n = host_stats(host_program, str(tmp_path), ssd, hw, beta, field, coupling)
        assert bad == n == 0 and same_bits(got, want), name
    extra = [("flat", R.flat_column(3), 3, 2.0, None, 0.0), ("spike", R.spike_column(2, 2.0, 7), 2, 2.0, None, 0.0),
             ("half-inf", R.half_with_inf(), 2, 0.001, None, 0.0), ("half-inf-field", R.half_with_inf(), 2, 0.001, R.random_field(2, (3, 5, 7), 4), 1.0)]
    for half in (False, True):
        ssd, _ = R.poisoned(half=half)
        extra.append(("poisoned-%d" % half, ssd, 2, 3.0, None, 0.0))
        extra.append(("poisoned-field-%d" % half, ssd, 2, 3.0, R.random_field(2, (3, 5, 7), 5), 1.0))
    for name, ssd, hw, beta, field, coupling in extra:
        want, bad = R.soft_stats(ssd, hw, beta, field, coupling)
        got, n = host_stats(host_program, str(tmp_path), ssd, hw, beta, field, coupling)
        assert bad == n == (3 if name.startswith("poisoned") else 0) and same_bits(got, want), name


def test_an_all_equal_column():
    for hw in (0, 1, 3, 5):
        for value in (3.25, 0.0, -7.5):
            n = 2 * hw + 1
            out, bad = R.soft_stats(R.flat_column(hw, value=value), hw, 2.0)
            o = out.reshape(12)
            assert bad == 0 and (o[0:3] == 0).all() and not np.signbit(o[0:3]).any()
            # sum of d^2 over -hw .. hw is hw (hw + 1) (2 hw + 1) / 3, so E d^2 = hw (hw + 1) / 3: sums of integers, exact in float64
            exact = np.float64(hw * (hw + 1)) / 3.0
            assert o[3] == o[6] == o[8] == F(exact) and o[4] == o[5] == o[7] == 0
            assert o[9] == n ** 3 and o[10] == 0 and o[11] == F(value)


def test_a_column_with_one_entry_far_below_the_others():
    for hw, beta, k in ((1, 2.0, 0), (2, 2.0, 7), (2, 0.125, 124), (3, 40.0, 171), (5, 1.0, 1330)):
        ssd = R.spike_column(hw, beta, k)
        assert (np.delete(ssd.ravel(), k) >= F(105.0) / F(beta)).all()
        out, bad = R.soft_stats(ssd, hw, beta)
        o = out.reshape(12)
        assert bad == 0 and (o[0:3] == R.deltas(hw)[k]).all() and (o[3:9] == 0).all() and o[9] == 1 and o[10] == 0 and o[11] == 0


def _bowl(hw, grid, beta, seed):
    """the sampled quadratic bowl |delta - c|^2 / (2 s^2 beta): a discretised Gaussian of width s around c under beta"""
    rng = np.random.default_rng(seed)
    V = int(np.prod(grid))
    c = rng.uniform(-0.5 * hw, 0.5 * hw, (3, V))
    s = rng.uniform(0.4, 1.5, V)
    D = R.deltas(hw).astype(np.float64)
    e = ((D[:, :, None] - c[None]) ** 2).sum(1) / (2.0 * s * s * beta)
    return e.astype(F).reshape((-1,) + grid), c, s


def _check_against_float64(name, ssd, hw, beta, field=None, coupling=0.0):
    """|restatement - float64 evaluation| within the derived bound, nothing tuned.  Each kept weight carries a relative error of at most
    eps = 104 * 2^-23 + 2^-22 ~ 1.27e-5: t = -(beta * (e - m)) takes two float32 roundings, 2^-23 |t| <= 104 * 2^-23 in absolute terms,
    which is the relative change of exp(t), and the exponential is within one ulp.  A weighted average of f under weights that each move
    by a relative eps moves by at most eps (1 + eps) E|f - E f|, so: mean within 2 hw eps, cov within 4 hw^2 eps, Z within eps relative,
    excess within 2 eps * 104 / beta.  Every bound also carries 2^-24 of the value for the output cast, and the dropped entries (t < -104)
    and denormal weights K (e^-104 + 2^-149) against Z >= 1.  softstats_restatement.reference_bound has the steps in full."""
    out, bad = R.soft_stats(ssd, hw, beta, field, coupling)
    assert bad == 0
    o = out.reshape(12, -1).astype(np.float64)
    mean, cov, Z, excess = R.reference64(ssd, hw, beta, field, coupling)
    b = R.reference_bound(hw, beta, (2 * hw + 1) ** 3)
    worst = dict(mean=np.abs(o[0:3] - mean) - R.CAST * np.abs(mean), cov=np.abs(o[3:9] - cov) - R.CAST * np.abs(cov),
                 Z=np.abs(o[9] / Z - 1.0) - R.CAST, excess=np.abs(o[10] - excess) - R.CAST * np.abs(excess))
    print(name, {k: "%.3g of %.3g" % (float(v.max()) + (R.CAST if k == "Z" else 0.0), b[k]) for k, v in worst.items()})
    for k, v in worst.items():
        assert float(v.max()) <= b[k], (name, k, float(v.max()), b[k])
    return o, mean


def test_restatement_against_a_float64_evaluation():
    for name, ssd, hw, beta, field, coupling in R.bit_cases()[4::3]:
        _check_against_float64(name, ssd, hw, beta, field, coupling)
    for hw, beta in ((2, 1.0), (3, 0.01), (5, 30.0)):
        ssd, c, s = _bowl(hw, (3, 5, 7), beta, 60 + hw)
        o, mean = _check_against_float64("bowl-hw%d" % hw, ssd, hw, beta)
        # where the Gaussian sits well inside the window and is wide enough to be sampled, the soft mean is its centre
        ok = (s > 0.8) & (np.abs(c).max(0) + 3.5 * s < hw)
        if ok.any():
            assert float(np.abs(mean[:, ok] - c[:, ok]).max()) < 2e-3
    # costs as large as a float16 volume's, and a beta that keeps only a few entries
    ssd = R.half_with_inf()
    _check_against_float64("half-inf", ssd, 2, 0.001)
    _check_against_float64("sharp", R.random_volume(3, (3, 5, 7), 77), 3, 400.0)


def test_the_coupling_draws_the_mean_towards_the_field():
    hw, grid = 3, (3, 5, 7)
    ssd = R.random_volume(hw, grid, 11)
    u = R.random_field(hw, grid, 12)
    free = R.soft_stats(ssd, hw, 4.0, u, 0.0)[0].reshape(12, -1)
    assert same_bits(free, R.soft_stats(ssd, hw, 4.0)[0].reshape(12, -1))          # a zero coupling adds +0.0 to every energy
    tied = R.soft_stats(ssd, hw, 4.0, u, 1.0)[0].reshape(12, -1)
    d_free = np.sqrt(((free[0:3] - u.reshape(3, -1)) ** 2).sum(0))
    d_tied = np.sqrt(((tied[0:3] - u.reshape(3, -1)) ** 2).sum(0))
    assert (d_tied < d_free).all() and float((d_free - d_tied).mean()) > 0.1
