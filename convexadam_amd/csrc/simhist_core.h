// simhist_core.h -- the arithmetic of simhist.hip that a host program can run as it stands: the joint histogram of a fixed
// image and a moving image, the latter optionally sampled through a displacement field, and the value range the bins are laid over.
// The entry points are stated at include/convexadam_sim.h; this text IS the contract, tests/simhist_restatement.py restates it with numpy
// and tools/simhist_host.cpp runs it on the host under sanitizers.  Compiled with -ffp-contract=off.
//
//   voxel    q = (i0 W + i1) D + i2 of an [H][W][D] grid; a = fixed[q]
//   sample   b = moving[q] without a field.  With a field u (a field operand of include/convexadam_field.h: component c of voxel q at
//            u[c * cs + q * vs], float or double, widened exactly to double):  c_k = (double)i_k + (double)u_k,  and
//            b = (float)map_linear_f64(moving, 1, H, W, D, c0, c1, c2)   (interp_f64.h): the arithmetic of cvx_map_coordinates_linear_f64
//            followed by warp_device's cast.  A coordinate outside 0 <= c <= n - 1 gives 0.0, or, with drop_outside, drops the voxel.
//   class    every voxel falls into exactly one class, decided in this order (sim_sample):
//              MASKED      the mask is given and mask[q] == 0 (nothing else of the voxel is looked at)
//              NON_FINITE  a is not finite, or a coordinate is not finite
//              OUTSIDE     drop_outside and a coordinate lies outside the volume
//              NON_FINITE  b is not finite (a NaN or Inf tap, or a float64 sum beyond float32's range)
//              KEPT        everything else
//   range    lo, hi = min, max of a and of b over the KEPT voxels, taken on the order-preserving key of the float's bits (sim_key: -0.0
//            sorts below +0.0), so that the result does not depend on the order; (+Inf, -Inf) when nothing is kept
//   scale    sim_scale(lo, hi, nb) = (float)nb / (hi - lo), float32; 0 when !(hi > lo) or when the quotient is not finite: a constant image
//            lands in bin 0
//   bin      t = (x - lo) * scale, each operation rounded;  0 if t < 0 (or t is a NaN, which only a non-finite range produces),
//            nb - 1 if t >= nb, else (int)t: the comparisons come BEFORE the conversion, as in interp_f64.h
//   counts   stats[0..3] = voxels per class (KEPT, MASKED, NON_FINITE, OUTSIDE): they sum to H W D.  stats[4] = KEPT voxels with
//            a < lo_a, a > hi_a, b < lo_b or b > hi_b: the values that were clamped into an end bin (always 0 from the range pass).
//            hist[ia * bins_b + ib] += 1 for every KEPT voxel: integers, exact whatever the split of the work.
// No logarithm here: the entropies are taken by the caller.  Plain C++ apart from the function qualifiers.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "interp_f64.h"

namespace cvx {

enum { SIM_KEPT = 0, SIM_MASKED = 1, SIM_NON_FINITE = 2, SIM_OUTSIDE = 3, SIM_CLAMPED = 4, SIM_STATS = 5 };
enum { SIM_MIN_BINS = 2, SIM_MAX_BINS = 256 };

CVX_HD bool sim_finite(float v) { return fabsf(v) <= FLT_MAX; }
CVX_HD bool sim_finite(double v) { return fabs(v) <= DBL_MAX; }

// order-preserving key of a float's bits: a < b as floats (or a = -0.0, b = +0.0)  <=>  sim_key(a) < sim_key(b) as unsigned integers
CVX_HD uint32_t sim_key(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
CVX_HD float sim_unkey(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float v;
    memcpy(&v, &b, 4);
    return v;
}
// The range is gathered in four unsigned slots that all take a MINIMUM and all start as 0xffffffff: slots 0, 2 hold sim_key of the smallest
// a, b, slots 1, 3 the complement of sim_key of the largest.  No finite value has the key 0xffffffff or 0, so an untouched slot is empty.
static constexpr uint32_t SIM_SLOT_EMPTY = 0xffffffffu;
CVX_HD float sim_slot_lo(uint32_t slot) { return slot == SIM_SLOT_EMPTY ? INFINITY : sim_unkey(slot); }
CVX_HD float sim_slot_hi(uint32_t slot) { return slot == SIM_SLOT_EMPTY ? -INFINITY : sim_unkey(~slot); }

CVX_HD float sim_scale(float lo, float hi, int nb) {
    if (!(hi > lo)) return 0.0f;
    const float s = (float)nb / (hi - lo);
    return sim_finite(s) ? s : 0.0f;
}
CVX_HD int sim_bin(float x, float lo, float scale, int nb) {
    const float t = (x - lo) * scale;
    if (t < 0.0f || t != t) return 0;
    if (t >= (float)nb) return nb - 1;
    return (int)t;
}
CVX_HD bool sim_clamped(float x, float lo, float hi) { return x < lo || x > hi; }

// The pair (a, b) of voxel q and its class.  u == nullptr: no field.  TU is float or double.
template <typename TU>
CVX_HD int sim_sample(const float* fixed, const float* moving, const TU* u, size_t cs, size_t vs, const unsigned char* mask, int H, int W, int D,
                      size_t q, int drop_outside, float& a, float& b) {
    a = b = 0.0f;
    if (mask && mask[q] == 0) return SIM_MASKED;
    a = fixed[q];
    if (!sim_finite(a)) return SIM_NON_FINITE;
    if (u) {
        const int i2 = (int)(q % (size_t)D), i1 = (int)((q / (size_t)D) % (size_t)W), i0 = (int)(q / ((size_t)D * (size_t)W));
        const double c0 = (double)i0 + (double)u[q * vs], c1 = (double)i1 + (double)u[cs + q * vs], c2 = (double)i2 + (double)u[2 * cs + q * vs];
        if (!(sim_finite(c0) && sim_finite(c1) && sim_finite(c2))) return SIM_NON_FINITE;
        const bool inside = c0 >= 0.0 && c0 <= (double)(H - 1) && c1 >= 0.0 && c1 <= (double)(W - 1) && c2 >= 0.0 && c2 <= (double)(D - 1);
        if (!inside && drop_outside) return SIM_OUTSIDE;
        b = (float)map_linear_f64(moving, 1, H, W, D, c0, c1, c2);
    } else {
        b = moving[q];
    }
    return sim_finite(b) ? SIM_KEPT : SIM_NON_FINITE;
}

// the bins' geometry of one call, from the four range values
struct SimBins {
    float lo_a, hi_a, lo_b, hi_b, scale_a, scale_b;
    int bins_a, bins_b;
};
CVX_HD SimBins sim_bins(const float* range, int bins_a, int bins_b) {
    SimBins g;
    g.lo_a = range[0], g.hi_a = range[1], g.lo_b = range[2], g.hi_b = range[3];
    g.scale_a = sim_scale(g.lo_a, g.hi_a, bins_a);
    g.scale_b = sim_scale(g.lo_b, g.hi_b, bins_b);
    g.bins_a = bins_a, g.bins_b = bins_b;
    return g;
}
// the cell of a KEPT pair in hist[bins_a][bins_b], and whether either value was clamped
CVX_HD int sim_cell(const SimBins& g, float a, float b, bool& clamped) {
    clamped = sim_clamped(a, g.lo_a, g.hi_a) || sim_clamped(b, g.lo_b, g.hi_b);
    return sim_bin(a, g.lo_a, g.scale_a, g.bins_a) * g.bins_b + sim_bin(b, g.lo_b, g.scale_b, g.bins_b);
}

// a whole volume, the way a single thread would take it (tools/simhist_host.cpp; the kernels split the voxels, integers do not care)
template <typename TU>
CVX_HD void sim_range_all(const float* fixed, const float* moving, const TU* u, size_t cs, size_t vs, const unsigned char* mask, int H, int W, int D,
                          int drop_outside, float* range_out, int64_t* stats) {
    uint32_t slot[4] = {SIM_SLOT_EMPTY, SIM_SLOT_EMPTY, SIM_SLOT_EMPTY, SIM_SLOT_EMPTY};
    for (int i = 0; i < SIM_STATS; ++i) stats[i] = 0;
    const size_t V = (size_t)H * W * D;
    for (size_t q = 0; q < V; ++q) {
        float a, b;
        const int cls = sim_sample(fixed, moving, u, cs, vs, mask, H, W, D, q, drop_outside, a, b);
        stats[cls] += 1;
        if (cls != SIM_KEPT) continue;
        const uint32_t ka = sim_key(a), kb = sim_key(b);
        slot[0] = ka < slot[0] ? ka : slot[0];
        slot[1] = ~ka < slot[1] ? ~ka : slot[1];
        slot[2] = kb < slot[2] ? kb : slot[2];
        slot[3] = ~kb < slot[3] ? ~kb : slot[3];
    }
    range_out[0] = sim_slot_lo(slot[0]);
    range_out[1] = sim_slot_hi(slot[1]);
    range_out[2] = sim_slot_lo(slot[2]);
    range_out[3] = sim_slot_hi(slot[3]);
}

template <typename TU>
CVX_HD void sim_hist_all(const float* fixed, const float* moving, const TU* u, size_t cs, size_t vs, const unsigned char* mask, int H, int W, int D,
                         int bins_a, int bins_b, const float* range, int drop_outside, int64_t* hist, int64_t* stats) {
    const SimBins g = sim_bins(range, bins_a, bins_b);
    for (int i = 0; i < SIM_STATS; ++i) stats[i] = 0;
    for (size_t i = 0; i < (size_t)bins_a * bins_b; ++i) hist[i] = 0;
    const size_t V = (size_t)H * W * D;
    for (size_t q = 0; q < V; ++q) {
        float a, b;
        const int cls = sim_sample(fixed, moving, u, cs, vs, mask, H, W, D, q, drop_outside, a, b);
        stats[cls] += 1;
        if (cls != SIM_KEPT) continue;
        bool clamped;
        hist[sim_cell(g, a, b, clamped)] += 1;
        stats[SIM_CLAMPED] += clamped;
    }
}

}  // namespace cvx
