// fieldops_core.h -- the per-voxel arithmetic of fieldops.hip: fixed-point inversion of a displacement field and the
// composition of two.  The contract is stated at cvx_field_invert_f64 / cvx_field_compose_f64 (include/convexadam_field.h); this text IS
// that contract, tests/fieldops_restatement.py restates it with numpy, and tools/fieldops_host.cpp runs it on the host under sanitizers.
// Float64 throughout, plain multiplies and adds in the order written (no fused multiply-add: -ffp-contract=off), taps through
// taps_linear_f64 (interp_f64.h).  Every comparison comes BEFORE a coordinate reaches floor(): a NaN or an infinite coordinate fails
// field_clamp and never becomes an index.
// Plain C++ apart from the function qualifiers, so that a host program can run the same text.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>

#include "interp_f64.h"

namespace cvx {

enum { FIELD_OK = 0, FIELD_NOT_CONVERGED = 1, FIELD_NON_FINITE = 2 };

// max(a, b) in which a NaN wins and stays
CVX_HD double field_max_nan(double m, double d) { return (d > m || d != d) ? d : m; }

// y + v clamped to [0, n - 1] on the three axes; false when a coordinate is not finite (c untouched beyond that axis)
CVX_HD bool field_clamp(const double (&y)[3], const double (&v)[3], const int (&n)[3], double (&c)[3]) {
    for (int a = 0; a < 3; ++a) {
        double r = y[a] + v[a];
        if (!(r >= -DBL_MAX && r <= DBL_MAX)) return false;
        const double hi = (double)(n[a] - 1);
        if (r < 0.0) r = 0.0;
        if (r > hi) r = hi;
        c[a] = r;
    }
    return true;
}

// the three components of a field at one clamped coordinate: component a of voxel q at f[a * cs + q * vs]
template <typename T>
CVX_HD void field_sample(const T* f, size_t cs, size_t vs, const int (&n)[3], const double (&c)[3], double (&s)[3]) {
    for (int a = 0; a < 3; ++a) s[a] = taps_linear_f64(f + a * cs, vs, n[0], n[1], n[2], c[0], c[1], c[2]);
}

// v(y) = -u(y + v(y)) at voxel y = (i0, i1, i2) by v_{k+1} = -u(y + v_k).  Returns FIELD_OK, FIELD_NOT_CONVERGED (tol > 0 and the last of
// max_iters steps was above it) or FIELD_NON_FINITE (v and residual are NaN then); iters = iterations started, at most 255.
template <typename T>
CVX_HD int field_invert_voxel(const T* u, size_t cs, size_t vs, int H, int W, int D, int i0, int i1, int i2, int max_iters, double tol,
                              double (&v)[3], double& residual, int& iters) {
    const int n[3] = {H, W, D};
    const double y[3] = {(double)i0, (double)i1, (double)i2};
    const size_t q = (((size_t)i0 * W + i1) * D + i2) * vs;
    for (int a = 0; a < 3; ++a) v[a] = -(double)u[a * cs + q];
    double c[3], s[3];
    int it = 0;
    bool met = false, finite = true;
    while (it < max_iters) {
        ++it;
        finite = field_clamp(y, v, n, c);
        if (!finite) break;
        field_sample(u, cs, vs, n, c, s);
        double step = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double vn = -s[a];
            step = field_max_nan(step, fabs(vn - v[a]));
            v[a] = vn;
        }
        if (tol > 0.0 && step <= tol) {
            met = true;
            break;
        }
    }
    double r = 0.0;
    if (finite) finite = field_clamp(y, v, n, c);
    if (finite) {
        field_sample(u, cs, vs, n, c, s);
        for (int a = 0; a < 3; ++a) r = field_max_nan(r, fabs(v[a] + s[a]));
        finite = r <= DBL_MAX;
    }
    iters = it < 255 ? it : 255;
    if (!finite) {
        v[0] = v[1] = v[2] = residual = (double)NAN;
        return FIELD_NON_FINITE;
    }
    residual = r;
    return tol > 0.0 && !met ? FIELD_NOT_CONVERGED : FIELD_OK;
}

// out(x) = b(x) + a(clamp(x + b(x))): warping with a, then with b, as one field.  false (out = NaN) when a coordinate is not finite.
template <typename TA, typename TB>
CVX_HD bool field_compose_voxel(const TA* fa, size_t acs, size_t avs, const TB* fb, size_t bcs, size_t bvs, int H, int W, int D, int i0,
                                int i1, int i2, double (&out)[3]) {
    const int n[3] = {H, W, D};
    const double y[3] = {(double)i0, (double)i1, (double)i2};
    const size_t q = ((size_t)i0 * W + i1) * D + i2;
    double bv[3], c[3], s[3];
    for (int a = 0; a < 3; ++a) bv[a] = (double)fb[a * bcs + q * bvs];
    if (!field_clamp(y, bv, n, c)) {
        out[0] = out[1] = out[2] = (double)NAN;
        return false;
    }
    field_sample(fa, acs, avs, n, c, s);
    for (int a = 0; a < 3; ++a) out[a] = bv[a] + s[a];
    return true;
}

}  // namespace cvx
