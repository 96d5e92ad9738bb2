// softstats_core.h -- the arithmetic of softstats.hip that a host program can run as it stands: the soft (Boltzmann-weighted)
// reading of a cost volume, per coarse cell the mean displacement, its 3 x 3 covariance, the partition sum and the mean excess energy.
// The entry point is stated at cvx_soft_stats_f32 (include/convexadam_soft.h); this text IS the contract, tests/softstats_restatement.py
// restates it with numpy loops, and tools/softstats_host.cpp runs it on the host under sanitizers.  Compiled with -ffp-contract=off: a
// multiply-add is fused only where the text says fmaf (soft_expf, as cvx_expf).
//
// The volume is [K][V], K = n^3, n = 2 hw + 1; entry k = (dD + hw) n^2 + (dW + hw) n + (dH + hw) of cell x belongs to the displacement
// delta_k = (dH, dW, dD): component 0 runs fastest, the order of correlate and disp_mesh.
//
//   energy   e_k = (float)ssd[k][x]                                   a half is widened exactly
//            with a field u (3 planes of V floats, coarse voxels):    e_k = e_k + coupling * q,
//            q = ((d0 - u0)^2 + (d1 - u1)^2) + (d2 - u2)^2            float32, each operation rounded
//   pass A   m = min_k e_k with the NaN-keeping min  (e < m || e != e) ? e : m  started at +Inf: it does not depend on the order of its
//            operands beyond a NaN's payload, which nothing reads.  m not finite (a NaN, a -Inf, or all entries +Inf): the column is
//            non-finite, its twelve outputs are the quiet NaN 0x7fc00000 and it counts once.
//   pass B   r = e_k - m;  t = -(beta * r);  an entry with t >= -104 is KEPT and weighs w = soft_expf(t); every other entry (t < -104, among
//            them r = +Inf: the +Inf entries of a float16 volume) is DROPPED: it adds nothing to any sum, its r included.
//            Eleven float64 sums over the kept entries, w, r and delta widened first, so that every product is exact (24 + 4 + 4 bits, 24 +
//            24 bits) and a fused multiply-add rounds like the multiply and the add:
//              Z += w;   A_a += w d_a (a = 0, 1, 2);   B_ab += (w d_a) d_b (ab = 00, 01, 02, 11, 12, 22);   E += w r
//   order    a chunk is one D-shift plane, the n^2 consecutive k of one dD: inside it every sum runs in k order from 0.0 (soft_chunk_sums);
//            the n chunk sums are added in dD order from 0.0 (soft_merge).  Any split of the chunks over wavefronts, workgroups or launches
//            therefore gives the same bits.
//   outputs  float64, rounded once to float32 (soft_finish):  0..2 mean_a = A_a / Z;  3..8 cov_ab = B_ab / Z - mean_a * mean_b in the order
//            of B, the diagonal clamped below at 0.0;  9 Z (>= 1: the minimum weighs exactly 1);  10 E / Z;  11 m.
//            No logarithm: the entropy ln Z + beta E / Z is taken by the caller.
// Plain C++ apart from the function qualifiers.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "interp_f64.h"

namespace cvx {

enum { SOFT_SUMS = 11, SOFT_CHANNELS = 12 };          // Z, A0 A1 A2, B00 B01 B02 B11 B12 B22, E

// a float16 as its bits, for the host; the kernels read __half and widen it in hardware -- both conversions are exact and equal
struct soft_half { uint16_t bits; };
CVX_HD float soft_widen(float v) { return v; }
CVX_HD float soft_widen(soft_half h) {
    const uint32_t s = (uint32_t)(h.bits & 0x8000u) << 16, ex = (h.bits >> 10) & 31u, man = h.bits & 0x3ffu;
    uint32_t u;
    if (ex == 31u) u = s | 0x7f800000u | (man << 13);                    // Inf, NaN
    else if (ex != 0u) u = s | ((ex + 112u) << 23) | (man << 13);        // normal
    else if (man == 0u) u = s;                                           // zero
    else {                                                               // subnormal: man * 2^-24, exact in float
        float f = (float)man * 5.9604644775390625e-08f;
        memcpy(&u, &f, 4);
        u |= s;
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// cvx_expf (cvx_common.h), restated for host and device: SLEEF's expf, Cody-Waite reduction, degree-6 FMA polynomial, one ldexp.  Called
// for -104 <= d <= 0 only, where q lies in -150 .. 0.
CVX_HD float soft_expf(float d) {
    const float R_LN2f = 1.442695040888963407359924681001892137426645954152985934135449406931f;
    const float L2Uf = 0.693145751953125f, L2Lf = 1.428606765330187045e-06f;
    const float qf = rintf(d * R_LN2f);
    const int q = (int)qf;
    float s = fmaf(qf, -L2Uf, d);
    s = fmaf(qf, -L2Lf, s);
    float u = 0.000198527617612853646278381f;
    u = fmaf(u, s, 0.00139304355252534151077271f);
    u = fmaf(u, s, 0.00833336077630519866943359f);
    u = fmaf(u, s, 0.0416664853692054748535156f);
    u = fmaf(u, s, 0.166666671633720397949219f);
    u = fmaf(u, s, 0.5f);
    u = 1.0f + fmaf(s * s, u, s);
    return ldexpf(u, q);
}

CVX_HD float soft_min(float e, float m) { return (e < m || e != e) ? e : m; }
CVX_HD bool soft_finite(float m) { return fabsf(m) <= FLT_MAX; }

// the coupling term of displacement (d0, d1, d2) around the field value (u0, u1, u2)
CVX_HD float soft_coupled(float e, float coupling, int d0, int d1, int d2, float u0, float u1, float u2) {
    const float a = (float)d0 - u0, b = (float)d1 - u1, c = (float)d2 - u2;
    const float q = (a * a + b * b) + c * c;
    return e + coupling * q;
}

// One column's view of the volume: entry k at ssd[k * V], the field value of the cell (has_field) and the coupling.
template <typename T>
struct SoftColumn {
    const T* ssd;          // &volume[0][x]
    size_t V;
    int hw;
    bool has_field;
    float coupling, u0, u1, u2;
    // the energy of entry j = (dW + hw) n + (dH + hw) of chunk c = dD + hw, given its stored value
    CVX_HD float energy(T stored, int dH, int dW, int dD) const {
        const float e = soft_widen(stored);
        return has_field ? soft_coupled(e, coupling, dH, dW, dD, u0, u1, u2) : e;
    }
};

// pass A over chunk c: the NaN-keeping min of its n^2 energies, started at +Inf
template <typename T>
CVX_HD float soft_chunk_min(const SoftColumn<T>& col, int c) {
    const int hw = col.hw, n = 2 * hw + 1;
    const T* p = col.ssd + (size_t)c * n * n * col.V;
    float m = INFINITY;
    for (int dW = -hw; dW <= hw; ++dW)
        for (int dH = -hw; dH <= hw; ++dH, p += col.V) m = soft_min(col.energy(*p, dH, dW, c - hw), m);
    return m;
}

// one kept-or-dropped entry added to the eleven sums
CVX_HD void soft_add(double (&s)[SOFT_SUMS], float e, float m, float beta, int dH, int dW, int dD) {
    const float r = e - m;
    const float t = -(beta * r);
    if (!(t >= -104.0f)) return;                                        // dropped (also: a NaN t, which only a non-finite column has)
    const double w = (double)soft_expf(t), d0 = (double)dH, d1 = (double)dW, d2 = (double)dD;
    const double a0 = w * d0, a1 = w * d1, a2 = w * d2;                  // exact
    s[0] += w;
    s[1] += a0;
    s[2] += a1;
    s[3] += a2;
    s[4] = fma(a0, d0, s[4]);                                            // exact products: the fused form rounds once, like the plain add
    s[5] = fma(a0, d1, s[5]);
    s[6] = fma(a0, d2, s[6]);
    s[7] = fma(a1, d1, s[7]);
    s[8] = fma(a1, d2, s[8]);
    s[9] = fma(a2, d2, s[9]);
    s[10] = fma(w, (double)r, s[10]);
}

// pass B over chunk c: the eleven sums of its n^2 entries in k order from 0.0
template <typename T>
CVX_HD void soft_chunk_sums(const SoftColumn<T>& col, int c, float m, float beta, double (&s)[SOFT_SUMS]) {
    const int hw = col.hw, n = 2 * hw + 1;
    const T* p = col.ssd + (size_t)c * n * n * col.V;
    for (int i = 0; i < SOFT_SUMS; ++i) s[i] = 0.0;
    for (int dW = -hw; dW <= hw; ++dW)
        for (int dH = -hw; dH <= hw; ++dH, p += col.V) soft_add(s, col.energy(*p, dH, dW, c - hw), m, beta, dH, dW, c - hw);
}

// the next chunk's sums added to the running totals (which start at 0.0 and take the chunks in dD order)
CVX_HD void soft_merge(double (&total)[SOFT_SUMS], const double (&chunk)[SOFT_SUMS]) {
    for (int i = 0; i < SOFT_SUMS; ++i) total[i] += chunk[i];
}

// the twelve outputs of a column from its totals and its minimum; returns whether the column is non-finite
CVX_HD bool soft_finish(const double (&s)[SOFT_SUMS], float m, float (&out)[SOFT_CHANNELS]) {
    if (!soft_finite(m)) {
        uint32_t qnan = 0x7fc00000u;
        float f;
        memcpy(&f, &qnan, 4);
        for (int i = 0; i < SOFT_CHANNELS; ++i) out[i] = f;
        return true;
    }
    const double Z = s[0];
    const double mean[3] = {s[1] / Z, s[2] / Z, s[3] / Z};
    out[0] = (float)mean[0];
    out[1] = (float)mean[1];
    out[2] = (float)mean[2];
    int i = 4;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b, ++i) {
            double c = s[i] / Z - mean[a] * mean[b];
            if (a == b && c < 0.0) c = 0.0;
            out[i - 1] = (float)c;
        }
    out[9] = (float)Z;
    out[10] = (float)(s[10] / Z);
    out[11] = m;
    return false;
}

// a whole column, the way a single thread would take it (tools/softstats_host.cpp; the kernels split the chunks and merge in this order)
template <typename T>
CVX_HD bool soft_column(const SoftColumn<T>& col, float beta, float (&out)[SOFT_CHANNELS]) {
    const int n = 2 * col.hw + 1;
    float m = INFINITY;
    for (int c = 0; c < n; ++c) m = soft_min(soft_chunk_min(col, c), m);
    double total[SOFT_SUMS], chunk[SOFT_SUMS];
    for (int i = 0; i < SOFT_SUMS; ++i) total[i] = 0.0;
    for (int c = 0; c < n; ++c) {
        soft_chunk_sums(col, c, m, beta, chunk);
        soft_merge(total, chunk);
    }
    return soft_finish(total, m, out);
}

}  // namespace cvx
