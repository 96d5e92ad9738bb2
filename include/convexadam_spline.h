/*
 * convexadam_spline.h -- C ABI of the cubic B-spline interpolation of libconvexadam_hip.so (csrc/spline.hip): order=3 of
 * scipy.ndimage with its defaults (mode='constant', cval=0, prefilter=True) in float64 -- the prefilter that turns samples into spline
 * coefficients, the warp of a volume by a displacement field, and the resampling of a volume onto another image grid.
 *
 * The conventions are those of convexadam_hip.h: device pointers, `int` status (CVX_OK / CVX_ERR_*), the last error's text, caller-provided
 * outputs, the stream as the last argument, and every argument checked before anything is enqueued.  No entry point takes a workspace or
 * uses atomics: the same bytes on every run.  CVX_ABI_VERSION is unchanged: no struct crosses this boundary.  The Python binding is
 * convexadam_amd/_spline.py (SPLINE_SIGNATURES).
 *
 * Volumes are [H][W][D] (axis 0 slowest), at most 2^31 - 1 voxels.  Coefficients are always double.
 * The arithmetic, operation by operation, is stated in csrc/spline_core.h.
 */
#ifndef CONVEXADAM_SPLINE_H
#define CONVEXADAM_SPLINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

/* ---- prefilter: samples -> coefficients ------------------------------------------------------------------------------------------------
 * src    [H][W][D] float (src_f64 = 0) or double (1).
 * coef   [H][W][D] double: the recursive filter with the pole sqrt(3) - 2 along every line of axis 0, then 1, then 2, each line started
 *        from the exact mirror sum (scipy's initialisation for mode='constant'); an axis of length 1 is left as it is.
 * Refused   CVX_ERR_INVALID_ARG: src or coef NULL; an extent < 1 or more than 2^31 - 1 voxels; a buffer not aligned to its element; coef
 *           overlapping src -- except src == coef with src_f64 = 1, which filters in place. */
int cvx_spline_prefilter_f64(const void* src, int src_f64, int H, int W, int D, double* coef, void* stream);

/* ---- warp: out(i) = spline(i + u(i)) -----------------------------------------------------------------------------------------------------
 * coef    what the prefilter wrote for the moving volume.
 * field   a field operand: component a (displacement along array axis a, in voxels) of voxel q = (i0 W + i1) D + i2 at
 *         field[a * comp_stride + q * voxel_stride], float (field_f64 = 0) or double (1), read in place.
 * out     [H][W][D] double; 0.0 where a coordinate lies outside 0 <= c <= n - 1 or is not finite.
 * Refused   CVX_ERR_INVALID_ARG: coef, field or out NULL; an extent < 1 or more than 2^31 - 1 voxels; field strides that fold components
 *           onto each other (positive, and voxel_stride >= 3 comp_stride or comp_stride >= H W D voxel_stride); a buffer not aligned to
 *           its element; out overlapping coef or the field. */
int cvx_map_coordinates_cubic_f64(const double* coef, const void* field, int field_f64, int64_t comp_stride, int64_t voxel_stride,
                                  int H, int W, int D, double* out, void* stream);

/* ---- resampling onto another grid --------------------------------------------------------------------------------------------------------
 * coef         [sz][sy][sx] double, what the prefilter wrote for the source volume.
 * map12_host   HOST memory, 12 doubles: source index (x, y, z) = m . output index (x, y, z) + t, m row-major in [0..8], t in [9..11].
 * out          [oz][oy][ox] float (out_f64 = 0, rounded to nearest) or double (1).  ITK's buffer rule: a voxel whose source index lies in
 *              -0.5 <= c <= n - 0.5 on every axis is interpolated at that index clamped to [0, n - 1]; every other voxel, and one whose
 *              index is not finite, is default_value.
 * Refused   CVX_ERR_INVALID_ARG: coef, out or map12_host NULL; an extent < 1 or more than 2^31 - 1 voxels on either grid; a buffer not
 *           aligned to its element; out overlapping coef; a non-finite index map or default value. */
int cvx_resample_cubic_f64(const double* coef, int sz, int sy, int sx, void* out, int out_f64, int oz, int oy, int ox,
                           const double* map12_host, double default_value, void* stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif

#endif /* CONVEXADAM_SPLINE_H */
