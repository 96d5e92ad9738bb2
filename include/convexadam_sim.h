/*
 * convexadam_sim.h -- C ABI of the intensity-similarity operators of libconvexadam_hip.so (csrc/simhist.hip): the value range and
 * the joint histogram of a fixed image and a moving image, the latter optionally warped by a displacement field inside the same pass.  The
 * histogram is what mutual information and normalised mutual information are computed from (convexadam_amd/similarity.py).
 *
 * The conventions are those of convexadam_hip.h: device pointers, `int` status (CVX_OK / CVX_ERR_*), cvx_last_error(), caller-provided
 * outputs, a stream argument, and every argument checked before anything is enqueued.  Neither launching entry point takes a workspace.
 * CVX_ABI_VERSION is unchanged: no struct crosses this boundary.  The Python binding is convexadam_amd/_sim.py (SIM_SIGNATURES).
 *
 * fixed, moving   [H][W][D] float32.
 * field           NULL, or a field operand as in convexadam_field.h: component a (displacement along array axis a, in voxels) of voxel
 *                 q = (i0 W + i1) D + i2 at field[a * field_comp_stride + q * field_voxel_stride], float (field_f64 = 0) or double (1).
 *                 The moving value of voxel q is then (float)taps(moving, i + u(q)), the float64 linear gather of csrc/interp_f64.h: the
 *                 arithmetic of cvx_map_coordinates_linear_f64 followed by a cast to float32, 0.0 for a coordinate outside
 *                 0 <= c <= n - 1 -- or, with drop_outside != 0, the voxel is dropped and counted.  Without a field the strides, the
 *                 element flag and drop_outside are ignored.
 * mask            NULL, or [H][W][D] uint8: a voxel takes part where its entry is non-zero.
 * stats           5 x int64 in device memory, written by the call: { kept, masked out, non-finite (either value or a coordinate is NaN
 *                 or +-Inf), outside (drop_outside only), kept but clamped into an end bin (a value outside its [lo, hi]; 0 from the
 *                 range pass) }.  The first four sum to H W D.
 * The arithmetic, voxel by voxel, is stated in csrc/simhist_core.h.  Integer atomics only: the same bytes on every run, whatever the split.
 */
#ifndef CONVEXADAM_SIM_H
#define CONVEXADAM_SIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

/* ---- value range of the kept voxels ---------------------------------------------------------------------------------------------------
 * range_out  4 x float32 in device memory: { lo_a, hi_a, lo_b, hi_b }, the smallest and largest kept value of the fixed (a) and of the
 *            sampled moving image (b); { +Inf, -Inf, +Inf, -Inf } when nothing is kept.  -0.0 counts as smaller than +0.0.
 * Refused   CVX_ERR_INVALID_ARG: fixed, moving, range_out or stats NULL; an extent < 1 or H W D >= 2^31; field strides that fold components
 *           onto each other (the rule of cvx_field_to_grid_f64); a buffer not aligned to its element; range_out or stats overlapping any
 *           other buffer. */
int cvx_sim_range_f32(const float* fixed, const float* moving, const void* field, int field_f64, int64_t field_comp_stride,
                      int64_t field_voxel_stride, const unsigned char* mask, int H, int W, int D, int drop_outside, float* range_out,
                      int64_t* stats, void* stream);

/* ---- joint histogram ------------------------------------------------------------------------------------------------------------------
 * range   4 x float32 in DEVICE memory, { lo_a, hi_a, lo_b, hi_b }: what cvx_sim_range_f32 wrote on the same stream, or the caller's.
 *         Per image: scale = (float)bins / (hi - lo), 0 when !(hi > lo) or when that is not finite; bin of x = 0 if t < 0, bins - 1 if
 *         t >= bins, else (int)t with t = (x - lo) * scale in float32.
 * hist    [bins_a][bins_b] int64, index a the fixed image.  The call resets hist and stats on the stream.
 * Two paths, decided by cvx_joint_hist_lds_bytes: up to 64 KiB of uint32 bins the workgroups count in LDS and flush their non-zero bins;
 * above that they add to hist directly.
 * Refused   CVX_ERR_INVALID_ARG: fixed, moving, range, hist or stats NULL; an extent < 1 or H W D >= 2^31; bins outside 2 .. 256; bad field
 *           strides; a buffer not aligned to its element; hist or stats overlapping any other buffer. */
int cvx_joint_hist_f32(const float* fixed, const float* moving, const void* field, int field_f64, int64_t field_comp_stride,
                       int64_t field_voxel_stride, const unsigned char* mask, int H, int W, int D, int bins_a, int bins_b, const float* range,
                       int drop_outside, int64_t* hist, int64_t* stats, void* stream);

/* Bytes of LDS a workgroup of cvx_joint_hist_f32 counts in: copies x bins_a x bins_b x 4 with 1 .. 4 copies; 0: the bins do not fit
 * (bins_a bins_b 4 > 64 KiB) and the call adds to hist directly; -1: bins the call refuses.  Host only, launches nothing. */
int cvx_joint_hist_lds_bytes(int bins_a, int bins_b);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif

#endif /* CONVEXADAM_SIM_H */
