// constdiv.hip -- host side of div_const (cvx_common.h): which launch-constant divisors may take the three-operation division
//     q = x * r ;  e = fma(-d, q, x) ;  q' = fma(e, r, q)          r = RN(1 / d)
// in place of the IEEE sequence.  Nothing here runs on the device.
//
// THE PROOF of one divisor is an enumeration: for all 2^23 significands of x in [1, 2) the three operations must give the bits of x / d.
// One binade stands for every x with 2^-76 <= |x| <= 2^76 (kConstDivLo, kConstDivHi), by scaling:
//   * sign: RN is symmetric, so x -> -x negates q, e, q' and the IEEE quotient alike;
//   * powers of two: x -> x 2^k multiplies the exact value of every step by 2^k, and rounding commutes with that as long as each ROUNDED
//     value is zero or normal before and after.  Write d in [2^a, 2^(a+1)).  For x in [1, 2): q and the quotient lie in [2^(-a-2), 2^(1-a)],
//     and the residual E = x - d q is a multiple of ulp(d) ulp(q) >= 2^(a-23) 2^(-a-2-23) = 2^-48, so a non-zero e has |e| >= 2^-48 whatever
//     the divisor (e = 0 scales trivially; the products inside the two fma are exact and never rounded on their own).  With k in [-76, 75]:
//     |e| 2^k >= 2^-124 is normal, q 2^k >= 2^(-a-78) is normal for a <= 48, and q 2^k <= 2^(76-a) is finite for a >= -48.
//   So a divisor qualifies when it is finite, positive, 2^-48 <= d < 2^49, and the enumeration finds no mismatch; everything else -- and on the
//   device every x outside the guard, +-0, Inf and NaN included -- keeps the IEEE division.  (tools/verify_div_exact.c's mismatches for 12 and
//   216 are of that kind: dividends below 2^-122 with denormal quotients, and -0.0.  On the guarded range both qualify.)
#include <math.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <unordered_map>
#include <vector>

#include "cvx_common.h"

#if !defined(__HIP_DEVICE_COMPILE__)
namespace cvx {
namespace {

inline float bits_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// OR of (candidate xor IEEE quotient) over n significands from m0 of the binade [1, 2).  The build does not contract (-ffp-contract=off):
// the candidate is the two fmaf the kernels issue, the reference a plain division.  No branch in the body, so that it vectorises.
#define CVX_CONSTDIV_BLOCK                                                                                              \
    uint32_t diff = 0;                                                                                                  \
    for (uint32_t i = 0; i < n; ++i) {                                                                                  \
        const float x = bits_float(0x3f800000u | (m0 + i));                                                            \
        const float q = x * r;                                                                                          \
        const float e = __builtin_fmaf(-d, q, x);                                                                       \
        const float q2 = __builtin_fmaf(e, r, q);                                                                       \
        const float ref = x / d;                                                                                        \
        diff |= float_bits(q2) ^ float_bits(ref);                                                                       \
    }                                                                                                                   \
    return diff;
#if defined(__x86_64__)
__attribute__((target("avx2,fma"), noinline)) uint32_t block_fma(float d, float r, uint32_t m0, uint32_t n) { CVX_CONSTDIV_BLOCK }
#endif
__attribute__((noinline)) uint32_t block_generic(float d, float r, uint32_t m0, uint32_t n) { CVX_CONSTDIV_BLOCK }
#undef CVX_CONSTDIV_BLOCK

bool enumerate_binade(float d, float r) {
    constexpr uint32_t kBlock = 4096;           // a failing divisor stops at its first bad block
#if defined(__x86_64__)
    static const bool have_fma = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    if (have_fma) {
        for (uint32_t m0 = 0; m0 < (1u << 23); m0 += kBlock)
            if (block_fma(d, r, m0, kBlock)) return false;
        return true;
    }
#endif
    for (uint32_t m0 = 0; m0 < (1u << 23); m0 += kBlock)
        if (block_generic(d, r, m0, kBlock)) return false;
    return true;
}

// process-wide: proofs by the bit pattern of the divisor.  Two threads that miss on the same divisor both enumerate and store the same answer.
std::mutex g_mu;
std::unordered_map<uint32_t, ConstDiv> g_table;

bool cache_find(float d, ConstDiv& out) {
    std::lock_guard<std::mutex> lock(g_mu);
    const auto it = g_table.find(float_bits(d));
    if (it == g_table.end()) return false;
    out = it->second;
    return true;
}

}  // namespace

bool const_div_enumerate(float d, float r) { return enumerate_binade(d, r); }

ConstDiv const_div_ieee(float d) { return ConstDiv{d, 1.0f / d, 0}; }

// Uncached.  Measured on an 8-core x86 host: 2.4 ms on one core with AVX2 + FMA (8 lanes; about ten times that through libm without them).
ConstDiv const_div_make(float d) {
    ConstDiv cd = const_div_ieee(d);
    if (!(d >= 0x1p-48f && d < 0x1p49f)) return cd;       // (NaN, Inf, zero, negative and the exponents the scaling argument does not cover)
    cd.ok = const_div_enumerate(cd.d, cd.r) ? 1 : 0;
    return cd;
}

ConstDiv const_div(float d) {
    ConstDiv cd;
    if (cache_find(d, cd)) return cd;
    cd = const_div_make(d);
    std::lock_guard<std::mutex> lock(g_mu);
    g_table.emplace(float_bits(d), cd);
    return cd;
}

ConstDiv const_div_if_proven(float d) {
    ConstDiv cd;
    return cache_find(d, cd) ? cd : const_div_ieee(d);
}

// What a run of the Adam loop pays: the 83 divisors of the benchmark pair (80 bias corrections, three grid scales) take 202 ms on one core
// and 61 ms from this pool on the 8-core host (8 workers on 8 cores that also run the caller: short of linear) -- once per process, in the
// warm-up call; above the "few tens of milliseconds" one would like for a first call, which is why it is a pool and why it is capped.
// Afterwards a lookup is a mutex and a hash probe, under 3 us through ctypes, 80 per pair.
void const_div_prove(const float* ds, int n, int budget) {
    std::vector<float> todo;
    for (int i = 0; i < n && (int)todo.size() < budget; ++i) {
        ConstDiv cd;
        bool seen = cache_find(ds[i], cd);
        for (size_t j = 0; j < todo.size() && !seen; ++j) seen = float_bits(todo[j]) == float_bits(ds[i]);
        if (!seen) todo.push_back(ds[i]);
    }
    if (todo.empty()) return;
    std::atomic<size_t> next{0};
    auto work = [&]() { for (size_t i; (i = next.fetch_add(1)) < todo.size();) (void)const_div(todo[i]); };
    const size_t nthreads = todo.size() < 8 ? todo.size() : 8;
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nthreads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

}  // namespace cvx

extern "C" int cvx_const_div_make(float d, int cached, float* r, int* ok) {
    CVX_REQUIRE(r && ok, "cvx_const_div_make: null pointer");
    const cvx::ConstDiv cd = cached ? cvx::const_div(d) : cvx::const_div_make(d);
    *r = cd.r;
    *ok = cd.ok;
    return CVX_OK;
}

// tests only: the enumeration with a reciprocal of the caller's choice (one that is off by 2^-8 must be caught)
extern "C" int cvx_const_div_enumerate(float d, float r) { return cvx::const_div_enumerate(d, r) ? 1 : 0; }

// The independent count behind tests/test_constdiv.py: one float at a time through libm's fmaf, no cache, no guard rule of its own.
extern "C" long long cvx_const_div_mismatches(float d, int exp_lo, int exp_hi, int guarded, unsigned* first_bad) {
    if (exp_lo < 0 || exp_hi > 254 || exp_lo > exp_hi) return -1;
    const volatile float dv = d;
    const float r = 1.0f / dv;
    long long bad = 0;
    for (uint32_t u = (uint32_t)exp_lo << 23; u < ((uint32_t)exp_hi + 1) << 23; ++u) {
        for (uint32_t sign = 0; sign < 2; ++sign) {
            const float x = cvx::bits_float(u | (sign << 31));
            const float ax = fabsf(x);
            float got;
            if (guarded && !(ax >= cvx::kConstDivLo && ax <= cvx::kConstDivHi)) got = x / dv;          // div_const's fallback
            else { const float q = x * r; const float e = fmaf(-dv, q, x); got = fmaf(e, r, q); }
            if (cvx::float_bits(got) != cvx::float_bits(x / dv)) {
                if (!bad && first_bad) *first_bad = u | (sign << 31);
                ++bad;
            }
        }
    }
    return bad;
}
#endif
