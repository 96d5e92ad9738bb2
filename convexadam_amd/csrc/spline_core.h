// spline_core.h -- the arithmetic of spline.hip that a host program can run as it stands: cubic B-spline interpolation as
// scipy.ndimage does it for order=3 with its defaults (mode='constant', cval=0, prefilter=True), in float64.  The entry points are stated at
// include/convexadam_spline.h; this text IS the contract, tests/spline_restatement.py restates it with numpy and tools/spline_host.cpp runs
// it on the host under sanitizers.  Compiled with -ffp-contract=off: every operation below is rounded on its own, in the order written.
//
//   prefilter of one line c[0 .. n-1] (spline_prefilter_line; scipy initialises the recursion by mirroring for mode='constant'):
//       z = sqrt(3) - 2, one double literal;  n == 1: the line is left as it is (no gain)
//       every sample is first multiplied by gain = (1 - z) * (1 - 1 / z)
//       causal start, the exact mirror sum (no truncated horizon):  zn1 = z^(n-1) by sequential multiplication;
//           s = c[0] + zn1 c[n-1];  for i = 1 .. n-2:  s += zi (c[i] + zn1 c[n-1-i]),  zi *= z  (zi starts as z);  c[0] = s / (1 - zn1 zn1)
//       forward       c[i] += z c[i-1]                               i = 1 .. n-1
//       anti-causal   c[n-1] = (z / (z z - 1)) (c[n-1] + z c[n-2])
//       backward      c[i] = z (c[i+1] - c[i])                       i = n-2 .. 0
//   axes are filtered in the order 0, 1, 2 (spline_prefilter_all): the first pass reads the source (float or double, widened exactly) and
//   writes the coefficients, always double; the other two run in place
//   weights for t = c - floor(c), u = 1 - t (spline_weights):
//       w1 = (t t (t - 2) 3 + 4) / 6,  w2 = (u u (u - 2) 3 + 4) / 6,  w0 = u u u / 6,  w3 = 1 - w0 - w1 - w2   (completed to exactly one, as
//       the linear kernel's weights are)
//   taps      the first is floor(c) - 1; an index outside [0, n-1] is mirrored about 0 and n - 1 with period 2 (n - 1); every index of an
//             axis of length 1 maps to 0 (spline_mirror)
//   value     sum over the 64 taps, axis 0 slowest, of ((v w_a) w_b) w_c, started from 0.0 (taps_cubic_f64)
//   inside    map_cubic_f64: 0.0 unless 0 <= c <= n - 1 on every axis (scipy's rule, and map_linear_f64's);
//             itk_cubic_f64: itk_inside and itk_clamp of interp_f64.h, then the taps; the default value outside
//             Every comparison comes BEFORE the conversion to an integer: a NaN, an infinity or 1e300 never becomes an index.
// Plain C++ apart from the function qualifiers.
#pragma once
#include <math.h>
#include <stddef.h>

#include "interp_f64.h"

namespace cvx {

constexpr double SPLINE_POLE = -0.2679491924311228;          // sqrt(3) - 2

CVX_HD double spline_gain() { return (1.0 - SPLINE_POLE) * (1.0 - 1.0 / SPLINE_POLE); }
CVX_HD double spline_anti_gain() { return SPLINE_POLE / (SPLINE_POLE * SPLINE_POLE - 1.0); }
// z^k by k sequential multiplications
CVX_HD double spline_pole_power(int k) {
    double p = 1.0;
    for (int i = 0; i < k; ++i) p *= SPLINE_POLE;
    return p;
}
// The steps of the recursion, one sample each: the line function below and the chunked walk of spline.hip's contiguous-axis kernel are
// both written with them, so that the two cannot differ in a bit.  a, b are samples BEFORE the gain.
CVX_HD double spline_start_ends(double first, double last, double zn1, double gain) { return first * gain + zn1 * (last * gain); }
CVX_HD double spline_start_term(double s, double zi, double a, double b, double zn1, double gain) { return s + zi * (a * gain + zn1 * (b * gain)); }
CVX_HD double spline_start_done(double s, double zn1) { return s / (1.0 - zn1 * zn1); }
CVX_HD double spline_forward(double a, double prev, double gain) { return a * gain + SPLINE_POLE * prev; }
CVX_HD double spline_anti_start(double last, double before_last) { return spline_anti_gain() * (last + SPLINE_POLE * before_last); }
CVX_HD double spline_backward(double next, double c) { return SPLINE_POLE * (next - c); }

// one line: sample i of the source at src[i * stride], coefficient i at c[i * stride]; src == c (elements double) filters in place.
// Each pass takes SPLINE_BLOCK samples at a time: all of a block's loads stand in front of its arithmetic and its stores, so that a thread
// of the strided kernels has eight independent loads in flight instead of one per step of the recursion (src may be c, which keeps the
// compiler from moving a load over a store by itself).  The order of the arithmetic is that of the statement above, sample by sample.
constexpr int SPLINE_BLOCK = 8;
template <typename TS>
CVX_HD void spline_prefilter_line(const TS* src, double* c, size_t stride, int n) {
    if (n == 1) {
        c[0] = (double)src[0];
        return;
    }
    const double gain = spline_gain(), zn1 = spline_pole_power(n - 1);
    double s = spline_start_ends((double)src[0], (double)src[(size_t)(n - 1) * stride], zn1, gain), zi = SPLINE_POLE;
    double a[SPLINE_BLOCK], b[SPLINE_BLOCK];
    int i = 1;
    for (; i + SPLINE_BLOCK <= n - 1; i += SPLINE_BLOCK) {               // samples i .. i + 7 <= n - 2 and their mirror images
#pragma unroll
        for (int k = 0; k < SPLINE_BLOCK; ++k) {
            a[k] = (double)src[(size_t)(i + k) * stride];
            b[k] = (double)src[(size_t)(n - 1 - i - k) * stride];
        }
#pragma unroll
        for (int k = 0; k < SPLINE_BLOCK; ++k) {
            s = spline_start_term(s, zi, a[k], b[k], zn1, gain);
            zi *= SPLINE_POLE;
        }
    }
    for (; i <= n - 2; ++i) {
        s = spline_start_term(s, zi, (double)src[(size_t)i * stride], (double)src[(size_t)(n - 1 - i) * stride], zn1, gain);
        zi *= SPLINE_POLE;
    }
    double prev = spline_start_done(s, zn1), before = prev;
    c[0] = prev;
    i = 1;
    for (; i + SPLINE_BLOCK <= n; i += SPLINE_BLOCK) {                   // samples i .. i + 7 <= n - 1
#pragma unroll
        for (int k = 0; k < SPLINE_BLOCK; ++k) a[k] = (double)src[(size_t)(i + k) * stride];
#pragma unroll
        for (int k = 0; k < SPLINE_BLOCK; ++k) {
            const double v = spline_forward(a[k], prev, gain);
            c[(size_t)(i + k) * stride] = v;
            before = prev;
            prev = v;
        }
    }
    for (; i < n; ++i) {
        const double v = spline_forward((double)src[(size_t)i * stride], prev, gain);
        c[(size_t)i * stride] = v;
        before = prev;
        prev = v;
    }
    double next = spline_anti_start(prev, before);
    c[(size_t)(n - 1) * stride] = next;
    i = n - 2;
    for (; i - (SPLINE_BLOCK - 1) >= 0; i -= SPLINE_BLOCK) {             // coefficients i .. i - 7 >= 0
#pragma unroll
        for (int k = 0; k < SPLINE_BLOCK; ++k) a[k] = c[(size_t)(i - k) * stride];
#pragma unroll
        for (int k = 0; k < SPLINE_BLOCK; ++k) {
            next = spline_backward(next, a[k]);
            c[(size_t)(i - k) * stride] = next;
        }
    }
    for (; i >= 0; --i) {
        next = spline_backward(next, c[(size_t)i * stride]);
        c[(size_t)i * stride] = next;
    }
}

// a whole [H][W][D] volume, the way a single thread would take it (tools/spline_host.cpp; the kernels split the lines)
template <typename TS>
inline void spline_prefilter_all(const TS* src, double* coef, int H, int W, int D) {
    const size_t plane = (size_t)W * D;
    for (size_t q = 0; q < plane; ++q) spline_prefilter_line(src + q, coef + q, plane, H);                                  // axis 0
    for (int z = 0; z < H; ++z)
        for (int x = 0; x < D; ++x) spline_prefilter_line(coef + z * plane + x, coef + z * plane + x, (size_t)D, W);       // axis 1
    for (size_t l = 0; l < (size_t)H * W; ++l) spline_prefilter_line(coef + l * D, coef + l * D, 1, D);                   // axis 2
}

CVX_HD void spline_weights(double t, double (&w)[4]) {
    const double u = 1.0 - t;
    w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = u * u * u / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
}

// -1 <= i <= n + 1 is all the taps of a coordinate inside [0, n - 1] ask for; any int is answered
CVX_HD int spline_mirror(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int r = i % period;
    if (r < 0) r += period;
    return r > n - 1 ? period - r : r;
}

// coef[(z * W + y) * D + x], extents (H, W, D); the CALLER guarantees 0 <= c <= n - 1 on every axis
CVX_HD double taps_cubic_f64(const double* coef, int H, int W, int D, double cz, double cy, double cx) {
    const double fz = floor(cz), fy = floor(cy), fx = floor(cx);
    const int z0 = (int)fz - 1, y0 = (int)fy - 1, x0 = (int)fx - 1;
    double wz[4], wy[4], wx[4];
    spline_weights(cz - fz, wz);
    spline_weights(cy - fy, wy);
    spline_weights(cx - fx, wx);
    size_t zz[4], yy[4], xx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        zz[i] = (size_t)spline_mirror(z0 + i, H) * W;
        yy[i] = (size_t)spline_mirror(y0 + i, W);
        xx[i] = (size_t)spline_mirror(x0 + i, D);
    }
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) r += ((coef[(zz[i] + yy[j]) * D + xx[k]] * wz[i]) * wy[j]) * wx[k];
    return r;
}

CVX_HD double map_cubic_f64(const double* coef, int H, int W, int D, double cz, double cy, double cx) {
    if (!(cz >= 0.0 && cz <= (double)(H - 1) && cy >= 0.0 && cy <= (double)(W - 1) && cx >= 0.0 && cx <= (double)(D - 1))) return 0.0;
    return taps_cubic_f64(coef, H, W, D, cz, cy, cx);
}

// the cubic twin of k_resample_linear's rule: ITK's buffer is -0.5 <= c <= n - 0.5, a coordinate beyond the last sample is clamped onto it
CVX_HD double itk_cubic_f64(const double* coef, int H, int W, int D, double cz, double cy, double cx, double dflt) {
    if (!(itk_inside(cz, H) && itk_inside(cy, W) && itk_inside(cx, D))) return dflt;
    return taps_cubic_f64(coef, H, W, D, itk_clamp(cz, H), itk_clamp(cy, W), itk_clamp(cx, D));
}

}  // namespace cvx
