/*
 * convexadam_field.h -- C ABI of the displacement-field operators of libconvexadam_hip.so (csrc/fieldops.hip):
 * the inverse of a field and the composition of two, each in one launch.
 *
 * convex_adam_pt returns the forward field u on the fixed grid: apply_convex(u, moving)(x) = moving(x + u(x)).  The reference has no
 * function for the opposite direction; these two operators are what ITK, ANTs and VoxelMorph-style code call "invert this field" and
 * "compose these two".  The conventions are those of convexadam_hip.h: device pointers, `int` status (CVX_OK / CVX_ERR_*),
 * cvx_last_error(), caller-provided outputs, a stream argument, and every argument checked before anything is launched.  Neither entry
 * point takes a workspace.  CVX_ABI_VERSION is unchanged: no struct crosses this boundary.  The Python binding is
 * convexadam_amd/_field.py (FIELD_SIGNATURES).
 *
 * Field operands use the addressing of cvx_field_to_grid_f64: component a (0, 1, 2 = displacement along array axis 0, 1, 2, in voxels) of
 * voxel q = (i0 W + i1) D + i2 sits at p[a * comp_stride + q * voxel_stride]; elements are float (`*_f64` = 0) or double (1).
 * [H][W][D][3], what convex_adam_pt returns, is (1, 3); [3][H][W][D], what cvx_register_pair_f32 writes, is (H W D, 1).
 *
 * taps(f_a, c) below is the float64 linear gather of csrc/interp_f64.h (taps_linear_f64): the sum over the 8 taps (axis 0 slowest) of
 * ((value * w0) * w1) * w2 started from 0.0, weights { 1 - t, 1 - (1 - t) }, upper taps clamped to the last index; one coordinate and one
 * set of weights serve the three components.  clamp(c): per axis, c < 0 becomes 0.0 and c > n - 1 becomes n - 1.  A coordinate that is
 * not finite (NaN or +-Inf) is never clamped and never becomes an index: the voxel is "non-finite" and its outputs are NaN.
 * max(..) keeps a NaN: m = (d > m || d != d) ? d : m, started from the value stated.
 */
#ifndef CONVEXADAM_FIELD_H
#define CONVEXADAM_FIELD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

/* ---- inverse of a field by fixed-point iteration ------------------------------------------------------------------------------------
 * v with v(y) = -u(y + v(y)), so that apply_convex(v, fixed) brings the fixed image into the moving frame.  All iterations of a voxel
 * run in registers: u is read, v is written once.  Per voxel y = (i0, i1, i2), float64, plain multiplies and adds in this order:
 *   v_a = -(double)u_a(y)
 *   for it = 1 .. max_iters:
 *     c = clamp(y + v)                         (not finite: the voxel stops here, non-finite)
 *     vn_a = -taps(u_a, c);   step = max_a |vn_a - v_a| from 0.0;   v = vn
 *     if tol > 0 and step <= tol: stop (converged)
 *   residual = max_a |v_a + taps(u_a, clamp(y + v))| from 0.0      (a max-norm: no square root, every output is bit-reproducible;
 *                                                                   a coordinate or a residual that is not finite: non-finite)
 *   iters = min(it, 255)                                            (iterations started)
 * A non-finite voxel writes NaN to its three components and its residual.  A float output is the round-to-nearest cast.
 * v_out   as the field operands above, its own strides and element type.
 * residual [H][W][D] double, iters [H][W][D] uint8: optional (NULL).
 * stats   optional, device, 3 x int64: { voxels that ran max_iters iterations with tol > 0 and never met it (non-finite ones not counted),
 *         non-finite voxels, the bit pattern of the largest finite residual (a non-negative double) }.  The call zeroes it on the stream,
 *         the kernel uses integer atomics only (add, max), so it is the same on every run.
 * Refused   CVX_ERR_INVALID_ARG: u or v_out NULL; an extent < 1 or more than 2^31 - 1 voxels; strides that fold components onto each
 *           other (the rule of cvx_field_to_grid_f64); max_iters outside 1 .. 1000; tol negative or not finite; a buffer not aligned to
 *           its element; any output overlapping u or another output. */
int cvx_field_invert_f64(const void* u, int u_f64, int64_t u_comp_stride, int64_t u_voxel_stride, int H, int W, int D, int max_iters,
                         double tol, void* v_out, int v_f64, int64_t v_comp_stride, int64_t v_voxel_stride, double* residual,
                         unsigned char* iters, long long* stats, void* stream);

/* ---- composition of two fields --------------------------------------------------------------------------------------------------------
 * out(x) = b(x) + taps(a, clamp(x + b(x))): the single field equal to warping with a and then with b in apply_convex's convention,
 *   apply_convex(b, apply_convex(a, img)) ~ apply_convex(out, img).   cvx_field_compose_f64(a = u, b = v) is the vector whose max-norm
 * cvx_field_invert_f64 reports as `residual`.  A voxel whose coordinate x + b(x) is not finite writes NaN to its three components.
 * a, b, out on the same [H][W][D] grid, each with its own strides and element type.
 * Refused   CVX_ERR_INVALID_ARG: a, b or out NULL; an extent < 1 or more than 2^31 - 1 voxels; bad strides or alignment as above;
 *           out overlapping a or b. */
int cvx_field_compose_f64(const void* a, int a_f64, int64_t a_comp_stride, int64_t a_voxel_stride, const void* b, int b_f64,
                          int64_t b_comp_stride, int64_t b_voxel_stride, int H, int W, int D, void* out, int out_f64,
                          int64_t out_comp_stride, int64_t out_voxel_stride, void* stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif

#endif /* CONVEXADAM_FIELD_H */
