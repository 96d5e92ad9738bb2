"""CPU checks of the joint histogram and the mutual information built on it, no device needed: the header the kernels compile
(csrc/simhist_core.h) run on the host under AddressSanitizer and UndefinedBehaviorSanitizer -- a stand-alone program,
tools/simhist_host.cpp, with the sanitizer runtimes linked in and started as a child process, so that no library has to be preloaded
anywhere -- against the numpy restatement bit for bit on the whole case matrix; the restatement against numpy.histogram2d where float32
and float64 binning provably agree; known answers; the entropies of convexadam_amd.similarity (torch, here on the CPU) against a float64
numpy evaluation inside the bound that simhist_restatement.entropy_bound derives; and the issue's sketch as a regression."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simhist_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the host-arithmetic test needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("simhist_host") / "simhist_host")
    header = os.path.join(ROOT, "convexadam_amd", "csrc", "simhist_core.h")
    assert os.path.exists(header), "csrc/simhist_core.h: the per-voxel arithmetic as a plain-C++ header"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.dirname(header), os.path.join(ROOT, "tools", "simhist_host.cpp"), "-o", exe]
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run(cmd + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode == 0:
            return exe
    raise AssertionError("%s\n%s" % (" ".join(cmd), r.stdout))


def host_run(exe, tmp, c, bins_list, rng=None):
    """the host program on one case, all of bins_list in one process -> (range, range stats, [(hist, stats)])"""
    shape = c["fixed"].shape
    V = int(np.prod(shape))
    field, mask = c["field"], c["mask"]
    kind, cs, vs = 0, 1, 3
    if field is not None:
        kind = 2 if field.dtype == np.float64 else 1
        cs, vs = (V, 1) if field.shape[0] == 3 and field.shape != shape + (3,) else (1, 3)
    inputs = [c["fixed"], c["moving"]] + ([field] if field is not None else []) + ([mask] if mask is not None else [])
    paths = []
    for i, a in enumerate(inputs):
        paths.append(os.path.join(tmp, "in%d.bin" % i))
        np.ascontiguousarray(a).tofile(paths[-1])
    out = os.path.join(tmp, "out.bin")
    given = [repr(float(v)) for v in (rng if rng is not None else (0, 0, 0, 0))]
    args = [*shape, kind, cs, vs, int(mask is not None), int(c["drop_outside"]), int(rng is not None), *given, len(bins_list)]
    for b in bins_list:
        args += list(b)
    r = subprocess.run([exe] + [str(a) for a in args] + paths + [out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "", "simhist_host %s: exit %d\n%s" % (args, r.returncode, r.stderr[-4000:])
    raw = open(out, "rb").read()
    assert len(raw) == 16 + 40 + sum(8 * ba * bb + 40 for ba, bb in bins_list)
    got_range, got_rs = np.frombuffer(raw, F, 4), np.frombuffer(raw, np.int64, 5, 16)
    off, hists = 56, []
    for ba, bb in bins_list:
        h = np.frombuffer(raw, np.int64, ba * bb, off).reshape(ba, bb)
        hists.append((h, np.frombuffer(raw, np.int64, 5, off + 8 * ba * bb)))
        off += 8 * ba * bb + 40
    return got_range, got_rs, hists


def test_host_arithmetic_under_sanitizers_equals_the_restatement(host_program, tmp_path):
    n = 0
    for shape in R.SHAPES:
        for with_mask in (False, True):
            for fk in R.FIELDS:
                for drop in ((0, 1) if fk is not None else (0,)):
                    c = R.case(shape, None, with_mask, fk, drop, seed=len(shape) + n % 5)
                    got_range, got_rs, hists = host_run(host_program, str(tmp_path), c, R.BINS)
                    want_range, want_rs = R.value_range(c["fixed"], c["moving"], c["field"], c["mask"], c["drop_outside"])
                    name = (shape, with_mask, fk, drop)
                    assert same_bits(got_range, want_range) and same_bits(got_rs, want_rs), name
                    assert int(want_rs[:4].sum()) == int(np.prod(shape)) and want_rs[4] == 0
                    for b, (h, s) in zip(R.BINS, hists):
                        want_h, want_s = R.joint_hist(c["fixed"], c["moving"], b, want_range, c["field"], c["mask"], c["drop_outside"])
                        assert same_bits(h, want_h) and same_bits(s, want_s), (name, b)
                        assert int(h.sum()) == int(s[0]) and int(s[:4].sum()) == int(np.prod(shape))
                        n += 1
    assert n == len(R.matrix()) == 630


def test_host_arithmetic_on_non_finite_values_and_given_ranges(host_program, tmp_path):
    c = R.planted_non_finite()
    r, rs, hists = host_run(host_program, str(tmp_path), c, [(32, 32), (129, 128)])
    want_r, want_rs, _, _ = R.expected(c)
    assert same_bits(r, want_r) and same_bits(rs, want_rs) and rs[R.NON_FINITE] >= 9
    for b, (h, s) in zip([(32, 32), (129, 128)], hists):
        want_h, want_s = R.joint_hist(c["fixed"], c["moving"], b, want_r, c["field"], c["mask"], c["drop_outside"])
        assert same_bits(h, want_h) and same_bits(s, want_s)
    # ranges the values overrun (clamped counts), a reversed, a constant, an infinite and a NaN range: every kept voxel still lands in a bin
    c = R.case((5, 4, 130), None, True, ("planar", "f32"), 1, seed=3)
    for rng in ((-0.5, 0.5, 0.2, 0.9), (1.0, -1.0, 0.0, 1.0), (0.25, 0.25, 0.0, 3.0), (-np.inf, np.inf, 0.0, 1.0), (np.nan, 1.0, 0.0, np.nan),
                (-3e38, 3e38, 0.0, 1e-44)):
        _, _, hists = host_run(host_program, str(tmp_path), c, [(7, 130)], rng=np.array(rng, F))
        want_h, want_s = R.joint_hist(c["fixed"], c["moving"], (7, 130), np.array(rng, F), c["field"], c["mask"], c["drop_outside"])
        assert same_bits(hists[0][0], want_h) and same_bits(hists[0][1], want_s), rng
        assert int(want_h.sum()) == int(want_s[0]) > 0
    assert R.scale(0.0, 1e-44, 130) == 0   # (the last range: nb / (hi - lo) overflows, everything of b lands in its bin 0)


def test_restatement_equals_numpy_histogram2d_on_integer_images():
    """Integer values 0 .. nb - 1 with lo = 0, hi = nb: scale = nb / nb = 1 exactly, t = (x - 0) * 1 = x exactly in float32 as in float64,
    so both binnings agree on every voxel and every case must match.  histogram2d closes its last bin on the right, which no value
    reaches here."""
    for k, (ba, bb) in enumerate(R.BINS):
        for shape in R.SHAPES:
            rng = np.random.default_rng(40 + k)
            a = rng.integers(0, ba, shape).astype(F)
            b = rng.integers(0, bb, shape).astype(F)
            h, s = R.joint_hist(a, b, (ba, bb), np.array([0, ba, 0, bb], F))
            ref, _, _ = np.histogram2d(a.ravel().astype(np.float64), b.ravel().astype(np.float64), bins=(ba, bb), range=((0, ba), (0, bb)))
            assert np.array_equal(h, ref.astype(np.int64)), (ba, bb, shape)
            assert s.tolist() == [a.size, 0, 0, 0, 0]


def _tol(*hists):
    """three entropies enter MI and NMI: the sum of their bounds.  NMI = (H_a + H_b) / H_ab moves by at most (1 + NMI) / H_ab <= 3 / H_ab
    times that (NMI <= 2), and its own division rounds once more: the tests allow 4 / H_ab."""
    return sum(R.entropy_bound(h.sum(1)) + R.entropy_bound(h.sum(0)) + R.entropy_bound(h) for h in hists)


def test_known_answers():
    rng = np.random.default_rng(7)
    shape, nb = (24, 20, 33), 32
    a = rng.integers(0, nb, shape).astype(F)
    full = np.array([0, nb, 0, nb], F)
    # identical images: MI = H_a, NMI = 2
    h, _ = R.joint_hist(a, a, nb, full)
    ha, hb, hab = R.entropies(h)
    assert ha > 3.0 and abs(R.mutual_information(h) - ha) <= _tol(h) and abs(R.normalized_mutual_information(h) - 2.0) <= 4 * _tol(h) / hab
    # b = perm[a]: a one-to-one relation of the bin values, the same MI = H_a
    perm = rng.permutation(nb).astype(F)
    hp, _ = R.joint_hist(a, perm[a.astype(np.int64)], nb, full)
    assert not np.array_equal(hp, h) and abs(R.mutual_information(hp) - ha) <= _tol(hp, h)
    assert abs(R.normalized_mutual_information(hp) - 2.0) <= 4 * _tol(hp) / hab
    # a constant image: scale 0, everything in its bin 0, entropy 0, MI = 0, NMI = (H_a + 0) / H_a = 1
    const = np.full(shape, 0.75, F)
    r, _ = R.value_range(a, const)
    assert r.tolist() == [0.0, nb - 1.0, 0.75, 0.75]
    hc, sc = R.joint_hist(a, const, nb, r)
    assert (hc[:, 1:] == 0).all() and sc.tolist() == [a.size, 0, 0, 0, 0]
    assert R.entropies(hc)[1] == 0.0 and abs(R.mutual_information(hc)) <= _tol(hc)
    both, _ = R.joint_hist(const, const, nb, np.array([0.75, 0.75, 0.75, 0.75], F))
    assert both[0, 0] == a.size and R.mutual_information(both) == 0.0 and np.isnan(R.normalized_mutual_information(both))
    # nothing kept
    assert all(np.isnan(v) for v in R.entropies(np.zeros((4, 4), np.int64)))


def test_independent_uniform_images_stay_at_chance_level():
    for ba, bb, shape, seed in ((8, 8, (24, 20, 33), 1), (32, 32, (48, 48, 48), 2), (7, 13, (24, 20, 33), 3)):
        rng = np.random.default_rng(seed)
        n = int(np.prod(shape))
        assert n / (ba * bb) >= 50
        a, b = rng.integers(0, ba, shape).astype(F), rng.integers(0, bb, shape).astype(F)
        h, _ = R.joint_hist(a, b, (ba, bb), np.array([0, ba, 0, bb], F))
        dof = (ba - 1) * (bb - 1)
        mi, chance = R.mutual_information(h), dof / (2.0 * n)
        print("independent %dx%d n=%d: MI %.3e, chance level %.3e, bound %.3e" % (ba, bb, n, mi, chance, R.independence_factor(dof) * chance))
        assert 0.0 <= mi <= R.independence_factor(dof) * chance


def test_entropies_equal_a_float64_numpy_evaluation_within_the_derived_bound():
    from convexadam_amd.similarity import entropies, mutual_information, normalized_mutual_information
    worst = 0.0
    hists = []
    for k, (ba, bb) in enumerate(R.BINS):
        c = R.case((24, 20, 33), (ba, bb), False, None, 0, seed=k)
        r, _, h, _ = R.expected(c)
        hists.append(h)
    hists.append(np.diag(np.arange(1, 33)).astype(np.int64))
    hists.append(np.array([[10 ** 12, 1], [0, 3]], np.int64))                       # p next to 1 and next to 0
    for h in hists:
        got = [float(v) for v in entropies(torch.from_numpy(h))]
        want = R.entropies(h)
        for g, w, counts in zip(got, want, (h.sum(1), h.sum(0), h)):
            b = R.entropy_bound(counts)
            worst = max(worst, abs(g - w) / b if b else abs(g - w))
            assert abs(g - w) <= b, (h.shape, g, w, b)
        mi = float(mutual_information(torch.from_numpy(h)))
        assert abs(mi - R.mutual_information(h)) <= _tol(h)
        nmi = float(normalized_mutual_information(torch.from_numpy(h)))
        assert abs(nmi - R.normalized_mutual_information(h)) <= 4 * _tol(h) / want[2]
    print("entropies, torch against numpy: worst difference %.3g of the bound" % worst)
    empty = torch.zeros((5, 3), dtype=torch.int64)
    assert all(bool(torch.isnan(v)) and v.dtype == torch.float64 for v in entropies(empty))
    assert bool(torch.isnan(mutual_information(empty))) and bool(torch.isnan(normalized_mutual_information(empty)))
    one = torch.zeros((5, 3), dtype=torch.int64)
    one[2, 1] = 9
    assert float(mutual_information(one)) == 0.0 and bool(torch.isnan(normalized_mutual_information(one)))


def test_mutual_information_separates_aligned_from_deformed_under_a_non_monotone_remap():
    """the issue's sketch: deformed_pair((48, 48, 48)), the second image through exp(-1.3 x) + 0.1 x^2, 32 bins"""
    from convexadam_amd import phantom
    shape = (48, 48, 48)
    fix, mov = phantom.deformed_pair(shape)
    aligned = phantom.phantom(shape, 1, 110)                   # the moving image's phantom and noise draw, before its warp
    fix = fix.numpy()
    out = {}
    for name, second in (("deformed", mov.numpy()), ("aligned", aligned.numpy())):
        b = R.remap(second)
        r, _ = R.value_range(fix, b)
        h, s = R.joint_hist(fix, b, 32, r)
        assert s.tolist() == [fix.size, 0, 0, 0, 0]
        out[name] = (R.mutual_information(h), R.normalized_mutual_information(h))
    print("remapped 48^3 pair: MI / NMI deformed %.3f / %.3f, aligned %.3f / %.3f" % (out["deformed"] + out["aligned"]))
    assert out["aligned"][0] > out["deformed"][0] and out["aligned"][1] > out["deformed"][1]
