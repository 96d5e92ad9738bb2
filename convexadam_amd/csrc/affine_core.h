// affine_core.h -- the arithmetic of affine.hip that a host program can run as it stands: the affine map of
// F.affine_grid(theta, align_corners=False) as a displacement field, and the 4 x 4 float64 solve of the least-trimmed affine fit.  The
// contract is stated at cvx_affine_field_f64 / cvx_affine_lts_f32 (include/convexadam_affine.h); this text IS that contract,
// tests/affine_restatement.py restates the field with numpy, and tools/affine_host.cpp runs both on the host under sanitizers.
// Float64 throughout, plain multiplies, adds and divisions in the order written (no fused multiply-add: -ffp-contract=off, as for
// fieldops_core.h).  The field is pure arithmetic on the coordinate: nothing here turns a coordinate into an index, so a NaN or an
// infinite displacement gives a non-finite output at its own voxel and touches nothing else.
// Plain C++ apart from the function qualifiers.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>

#include "interp_f64.h"

namespace cvx {

// out = A(x + u) - x at voxel x = (i0, i1, i2) of an (H, W, D) grid, in voxels, component a along array axis a.
//   p_a = x_a + u_a                                   (u == nullptr: p_a = x_a)
//   n_a = (2 p_a + 1) / S_a - 1                       the normalised coordinate of align_corners=False
//   g_r = ((th[r][0] n_2 + th[r][1] n_1) + th[r][2] n_0) + th[r][3]      r = 0, 1, 2: x along D (axis 2), y along W (1), z along H (0)
//   q_a = ((g_(2-a) + 1) S_a - 1) * 0.5               back to voxels
//   out_a = q_a - x_a
// th: 12 floats (3 x 4, row-major), widened to double; u: component a of voxel q at u[a * cs + q * vs].
template <typename T>
CVX_HD void affine_field_voxel(const float* th, const T* u, size_t cs, size_t vs, int H, int W, int D, int i0, int i1, int i2,
                               double (&out)[3]) {
    const double S[3] = {(double)H, (double)W, (double)D};
    const double x[3] = {(double)i0, (double)i1, (double)i2};
    const size_t q = (((size_t)i0 * W + i1) * D + i2) * vs;
    double n[3];
    for (int a = 0; a < 3; ++a) {
        const double p = u ? x[a] + (double)u[a * cs + q] : x[a];
        n[a] = (2.0 * p + 1.0) / S[a] - 1.0;
    }
    for (int a = 0; a < 3; ++a) {
        const int r = 2 - a;
        const double g = (((double)th[4 * r] * n[2] + (double)th[4 * r + 1] * n[1]) + (double)th[4 * r + 2] * n[0]) + (double)th[4 * r + 3];
        out[a] = ((g + 1.0) * S[a] - 1.0) * 0.5 - x[a];
    }
}

enum { AFFINE_FIT_OK = 0, AFFINE_FIT_NON_FINITE = 1, AFFINE_FIT_SINGULAR = 2 };

// Solves A X = B for X (4 x nrhs, nrhs <= 4) by Gaussian elimination with partial pivoting (the largest |entry| of the column, the first
// one among equals); aug holds [A | B] row by row, 8 doubles per row; A is destroyed and X replaces B (X[r][j] = aug[r][4 + j]).  A pivot
// that is zero or not finite, or a solution that is not finite, returns AFFINE_FIT_SINGULAR; an entry of aug that is not finite to begin
// with returns AFFINE_FIT_NON_FINITE.  Whatever aug holds after a failure is not a solution.
CVX_HD int affine_solve4(double (*aug)[8], int nrhs) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4 + nrhs; ++c)
            if (!(aug[r][c] >= -DBL_MAX && aug[r][c] <= DBL_MAX)) return AFFINE_FIT_NON_FINITE;
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        double best = fabs(aug[col][col]);
        for (int r = col + 1; r < 4; ++r) {
            const double v = fabs(aug[r][col]);
            if (v > best) { best = v; piv = r; }
        }
        if (!(best > 0.0 && best <= DBL_MAX)) return AFFINE_FIT_SINGULAR;
        if (piv != col)
            for (int c = 0; c < 4 + nrhs; ++c) {
                const double t = aug[col][c];
                aug[col][c] = aug[piv][c];
                aug[piv][c] = t;
            }
        for (int r = col + 1; r < 4; ++r) {
            const double f = aug[r][col] / aug[col][col];
            aug[r][col] = 0.0;
            for (int c = col + 1; c < 4 + nrhs; ++c) aug[r][c] = aug[r][c] - f * aug[col][c];
        }
    }
    for (int j = 0; j < nrhs; ++j)
        for (int r = 3; r >= 0; --r) {
            double s = aug[r][4 + j];
            for (int c = r + 1; c < 4; ++c) s = s - aug[r][c] * aug[c][4 + j];
            s = s / aug[r][r];
            if (!(s >= -DBL_MAX && s <= DBL_MAX)) return AFFINE_FIT_SINGULAR;
            aug[r][4 + j] = s;
        }
    return AFFINE_FIT_OK;
}

}  // namespace cvx
