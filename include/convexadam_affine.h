/*
 * convexadam_affine.h -- C ABI of the affine model of libconvexadam_hip.so (csrc/affine.hip): the least-trimmed affine fit
 * to two point sets (least_trimmed_squares of l2r_2020_convexAdam_CuRIOUS.py:272-278, the twin of least_trimmed_rigid) and the affine
 * map of F.affine_grid as a displacement field, each in one launch.
 *
 * The conventions are those of convexadam_hip.h: device pointers, `int` status (CVX_OK / CVX_ERR_*), cvx_last_error(), caller-provided
 * outputs, a stream argument, and every argument checked before anything is launched.  CVX_ABI_VERSION is unchanged: no struct crosses
 * this boundary.  The Python binding is convexadam_amd/_affine.py (AFFINE_SIGNATURES).
 */
#ifndef CONVEXADAM_AFFINE_H
#define CONVEXADAM_AFFINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

/* ---- least-trimmed affine fit ---------------------------------------------------------------------------------------------------------
 * X (4 x 4, row-major, float32) with  moving_i ~ fixed_i X  for the rows fixed_i, moving_i (4 floats each: three coordinates and the
 * homogeneous 1) at fixed + i * ld_fixed, moving + i * ld_moving.  `iters` fits in ONE launch of one 1024-thread workgroup: fit 0 on all n
 * points, fit k on the n / 2 points with the smallest residuals under fit k - 1.  Per fit, over the current set (F, M its rows):
 *   normal = 0   least squares: (F^T F) X[:, :3] = F^T M[:, :3]; column 3 of X is written as exactly (0, 0, 0, 1)
 *   normal = 1   the reference's equation (CuRIOUS:275, torch.solve(M^T M, M^T F)): (M^T F) X = M^T M, all four columns
 * The 4 x 4 moment matrices are float64 sums of float64 products in a fixed order (each thread walks i = tid, tid + 1024, ..., a butterfly
 * inside the wavefront, the 16 wavefront sums in order; no atomics: the same bits on every run); one lane solves the system in float64 by
 * Gaussian elimination with partial pivoting and rounds X to float32.  Between fits: float32 residuals r_i = || moving_i - fixed_i X ||
 * over all four columns, p = f0 X[0][a]; p = fma(f1, X[1][a], p); p = fma(f2, X[2][a], p); p = fma(f3, X[3][a], p); e = m[a] - p;
 * s = s + e e; r = sqrt(s) (normal = 0: the last column's term is m[3] - f[3]); the n / 2 smallest are kept, a NaN residual sorts last,
 * ties at the threshold go to the lowest index -- the selection of cvx_rigid_lts_f32, the same code.
 * ld == 3 (iters == 1 and normal == 0 only): rows of three coordinates, the homogeneous 1 is implied.  Otherwise ld >= 4.
 * inliers  optional [n] bytes: 1 for the points the returned fit used (all of them for iters == 1).
 * The call synchronises the stream once to read the fit's status.  A singular system (a pivot that is zero or not finite: coplanar
 * points) or a non-finite moment (a non-finite coordinate in a fit's set) returns CVX_ERR_INVALID_ARG with cvx_last_error() text and
 * leaves X and inliers unwritten.
 * Refused   CVX_ERR_INVALID_ARG: fixed, moving, X or workspace NULL; n outside 4 .. 2^28, or below 8 with iters >= 2; iters < 1; normal
 *           neither 0 nor 1; a leading dimension outside the rule above or beyond 2^20; a buffer not aligned to 4 bytes; X or inliers
 *           overlapping the points.  CVX_ERR_WORKSPACE: workspace_bytes below cvx_affine_lts_workspace_bytes(n), which is 0 for an n
 *           outside 4 .. 2^28. */
size_t cvx_affine_lts_workspace_bytes(int64_t n);
int cvx_affine_lts_f32(const float* fixed, int ld_fixed, const float* moving, int ld_moving, int64_t n, int iters, int normal, float* X,
                       unsigned char* inliers, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the affine map as a displacement field -------------------------------------------------------------------------------------------
 * out(x) = A(x + u(x)) - x in voxels, A the map F.affine_grid(theta, (1, C, H, W, D), align_corners=False) describes: the field that
 * apply_convex takes in place of affine_warp(.., theta) followed by the warp with u (u == NULL: the affine alone).  Per voxel
 * x = (i0, i1, i2), float64, plain operations in this order (S = (H, W, D)):
 *   p_a = x_a + (double)u_a(x);   n_a = (2 p_a + 1) / S_a - 1
 *   g_r = ((th[r][0] n_2 + th[r][1] n_1) + th[r][2] n_0) + th[r][3]       r = 0, 1, 2 -- x along D, y along W, z along H, as cvx_affine_warp_f32
 *   out_a = ((g_(2-a) + 1) S_a - 1) * 0.5 - x_a
 * The evaluation is analytic: no interpolation and no padding rule; a u(x) that is not finite gives a non-finite out(x) and nothing else.
 * theta  12 floats (3 x 4, row-major) in DEVICE memory, widened to double.
 * u, out use the addressing of convexadam_field.h: component a of voxel q = (i0 W + i1) D + i2 at p[a * comp_stride + q * voxel_stride],
 *        elements float (`*_f64` = 0) or double (1); a float output is the round-to-nearest cast.
 * Refused   CVX_ERR_INVALID_ARG: theta or out NULL; an extent < 1 or more than 2^31 - 1 voxels; strides that fold components onto each
 *           other; a buffer not aligned to its element; out overlapping u or theta. */
int cvx_affine_field_f64(const float* theta, int H, int W, int D, const void* u, int u_f64, int64_t u_comp_stride, int64_t u_voxel_stride,
                         void* out, int out_f64, int64_t out_comp_stride, int64_t out_voxel_stride, void* stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif

#endif /* CONVEXADAM_AFFINE_H */
