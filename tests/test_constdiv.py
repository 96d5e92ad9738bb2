"""Host side of div_const (csrc/constdiv.hip): which launch-constant divisors may take the three-operation division
    q = x * r ;  e = fma(-d, q, x) ;  q' = fma(e, r, q)          r = RN(1 / d)
of the exact Adam loop.  const_div_make proves a divisor by enumerating ONE binade of x and claims 2^-76 <= |x| <= 2^76 from it; here its
answer is set against a brute-force count (cvx_const_div_mismatches: one float at a time through libm's fmaf, both signs) over three whole
binades inside that range -- the lowest, the middle and the highest -- and, with the device's guard, over the two lowest and the two highest
exponents there are.  No GPU.

The failing divisor.  12 and 216, which tools/verify_div_exact.c lists with mismatches, QUALIFY: all their mismatches are dividends below
2^-122, whose quotients are denormal, and -0.0; the guard keeps both on the IEEE path -- checked below.  No divisor in [2^-48, 2^49) was
found to fail on a normal binade (12 000 random significands, the integers to 2000, every (n - 1) / 2 to n = 600).  The divisor used is
12 * 2^80: it brings 12's denormal quotients to dividends around 2^-65, inside the guard, where the sequence does fail (x = 1.125 * 2^-65),
and it must come back ok = 0: its exponent is outside the range for which one binade stands for the guard."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

GUARD = 76
BIAS = 127


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    return _lib.lib()


def make(L, d, cached=0):
    r, ok = C.c_float(), C.c_int(-1)
    assert L.cvx_const_div_make(C.c_float(d), cached, C.byref(r), C.byref(ok)) == 0
    return r.value, ok.value


def mismatches(L, d, lo, hi, guarded):
    first = C.c_uint(0)
    n = L.cvx_const_div_mismatches(C.c_float(d), lo, hi, guarded, C.byref(first))
    assert n >= 0
    return n, first.value


def bc2s(step):
    return float(np.float32(math.sqrt(1.0 - 0.999 ** step)))


def test_bc2s_is_the_loops_value():
    """the helper above restates adam_run_impl's (float)sqrt(1.0 - pow(0.999, step)) -- pow of a double, not a float"""
    assert bc2s(1) == float(np.float32(math.sqrt(1.0 - math.pow(0.999, 1.0)))) and 0.031 < bc2s(1) < 0.032 and 0.99 < bc2s(5000) < 1.0


DIVISORS = [27.0, 39.5, 47.5, 55.5, bc2s(1), bc2s(2), bc2s(80), bc2s(5000)]


@pytest.mark.parametrize("d", DIVISORS + [12.0, 216.0], ids=lambda d: "%.9g" % d)
def test_proof_agrees_with_brute_force(L, d):
    r, ok = make(L, d)
    assert ok == 1 and r == float(np.float32(1.0) / np.float32(d))
    for e in (BIAS - GUARD, BIAS, BIAS + GUARD - 1):                         # whole binades [2^-76, 2^-75), [1, 2), [2^75, 2^76)
        assert mismatches(L, d, e, e, 0) == (0, 0), e
    assert mismatches(L, d, BIAS + GUARD, BIAS + GUARD, 1)[0] == 0          # 2^76 itself is inside, the rest of its binade falls back
    # what the device computes at the edges of float32: denormals, zeros of both signs and the first normal binade; the last two
    assert mismatches(L, d, 0, 1, 1)[0] == 0
    assert mismatches(L, d, 253, 254, 1)[0] == 0


def test_the_guard_is_needed(L):
    """without it the sequence loses the sign of -0.0 for every divisor, and 12 misrounds denormal quotients"""
    n, first = mismatches(L, 27.0, 0, 0, 0)
    assert n == 1 and first == 0x80000000
    n, first = mismatches(L, 12.0, 0, 0, 0)
    assert n > 1


def test_a_divisor_that_fails_is_refused(L):
    d = 12.0 * 2.0 ** 80
    n, first = mismatches(L, d, BIAS - 65, BIAS - 65, 0)                     # x in [2^-65, 2^-64): inside the guard, quotients denormal
    assert n > 0 and 2.0 ** -65 <= np.array([first & 0x7fffffff], np.uint32).view(np.float32)[0] < 2.0 ** -64
    assert make(L, d)[1] == 0
    for bad in (0.0, -27.0, float("inf"), float("nan"), 2.0 ** -49, 2.0 ** 49):
        assert make(L, bad)[1] == 0, bad
    assert make(L, 2.0 ** -48)[1] == 1 and make(L, float(np.nextafter(np.float32(2.0 ** 49), np.float32(0))))[1] == 1


@pytest.mark.parametrize("d", [27.0, 39.5, bc2s(80)], ids=lambda d: "%.9g" % d)
def test_the_enumeration_rejects_a_wrong_reciprocal(L, d):
    """No divisor in range was found to fail with r = RN(1 / d), so the reject path of the enumeration itself is exercised with a wrong
    reciprocal.  The correction step squares the relative error of q = x r, so a reciprocal that is off by eps leaves about eps^2 in q':
    2^-8 leaves 2^-16, 256 ulps, and must be caught; the right reciprocal passes."""
    r = np.float32(1.0) / np.float32(d)
    assert L.cvx_const_div_enumerate(C.c_float(d), C.c_float(float(r))) == 1
    for wrong in (r * np.float32(1 + 2.0 ** -8), r * np.float32(1 - 2.0 ** -8)):
        assert L.cvx_const_div_enumerate(C.c_float(d), C.c_float(float(wrong))) == 0


def test_cache_gives_one_answer_to_two_threads(L):
    ds = [bc2s(s) for s in range(3000, 3006)] + [12.0 * 2.0 ** 80]
    got = [None, None]

    def work(i):
        got[i] = [make(L, d, cached=1) for d in ds]

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == got[1] == [make(L, d) for d in ds]
    assert [ok for _, ok in got[0]] == [1] * 6 + [0]
    assert got[0] == [make(L, d, cached=1) for d in ds]                       # and again, now from the table
