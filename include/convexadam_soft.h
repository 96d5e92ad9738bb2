/*
 * convexadam_soft.h -- C ABI of the soft reading of a cost volume of libconvexadam_hip.so (csrc/softstats.hip): per coarse
 * cell the Boltzmann-weighted mean displacement, its 3 x 3 covariance, the partition sum and the mean excess energy, for the data term
 * alone or for the coupled energy around a given field.
 *
 * The conventions are those of convexadam_hip.h: device pointers, `int` status (CVX_OK / CVX_ERR_*), cvx_last_error(), caller-provided
 * outputs and workspace, a stream argument, and every argument checked before anything is launched.  CVX_ABI_VERSION is unchanged: no
 * struct crosses this boundary.  The Python binding is convexadam_amd/_soft.py (SOFT_SIGNATURES).
 */
#ifndef CONVEXADAM_SOFT_H
#define CONVEXADAM_SOFT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

/* ---- soft statistics of a cost volume -------------------------------------------------------------------------------------------------
 * ssd    the volume [K][V] as cvx_correlate_*_f32 writes it: K = (2 hw + 1)^3 displacements, V = h w d cells, float32 (ssd_is_half = 0) or
 *        float16 (1).  Entry k = (dD + hw) n^2 + (dW + hw) n + (dH + hw) is the displacement (dH, dW, dD), n = 2 hw + 1.
 * field  NULL, or [3][V] float32 in coarse voxels (what cvx_coupled_convex_* returns): the energy of an entry is then
 *        e = ssd + coupling * |delta - field|^2, float32; without a field it is the stored value and coupling must be 0.
 * out    [12][V] float32: 0..2 the mean displacement; 3..8 its covariance (00, 01, 02, 11, 12, 22; the diagonal clamped at 0); 9 the
 *        partition sum Z = sum_k exp(-beta (e_k - m)) >= 1; 10 the mean excess energy sum_k w_k (e_k - m) / Z; 11 the minimum m.
 *        The entropy of the weights is ln Z + beta * out[10].  A column whose minimum is not finite (a NaN, a -Inf, every entry +Inf) has
 *        NaN in all twelve channels; +Inf entries beside finite ones weigh nothing.
 * stats  one int64 in device memory: the number of non-finite columns (written by the call; integer atomics only).
 * The arithmetic, entry by entry, and the ORDER of every float64 sum are stated in csrc/softstats_core.h: the result does not depend on
 * how the work is split and is the same bits on every run.  Two launches: the minima of the D-shift planes into the workspace, then the
 * sums, one workgroup per 64 cells with the planes spread over its wavefronts and merged in plane order.
 * Refused   CVX_ERR_INVALID_ARG: ssd, out or stats NULL; an extent < 1; hw outside 0 .. 15; K V >= 2^31; beta not finite or <= 0;
 *           coupling negative or not finite, or non-zero without a field; a buffer not aligned to its element (the workspace: 8 bytes);
 *           out, stats or the workspace overlapping another buffer; workspace NULL or workspace_bytes below
 *           cvx_soft_stats_workspace_bytes(h, w, d, hw), which is 0 for extents or an hw that the call would refuse. */
size_t cvx_soft_stats_workspace_bytes(int h, int w, int d, int hw);
int cvx_soft_stats_f32(const void* ssd, int ssd_is_half, const float* field, float coupling, float beta, int h, int w, int d, int hw,
                       float* out, int64_t* stats, void* workspace, size_t workspace_bytes, void* stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif

#endif /* CONVEXADAM_SOFT_H */
