/*
 * convexadam_prep.h -- C ABI of the nnU-Net preprocessing helpers of libconvexadam_hip.so (csrc/prep.hip).
 *
 * The reference keeps these helpers in src/convexAdam/convex_adam_utils.py:142-170, 196-265 (and again in
 * self_configuring/convexAdam_hyper_util.py:295-420).  The conventions are those of convexadam_hip.h: device pointers, `int`
 * status (CVX_OK / CVX_ERR_*), cvx_last_error(), caller-provided outputs, a workspace sized by the matching *_workspace_bytes()
 * query, a stream argument, and every argument checked before anything is launched.  CVX_ABI_VERSION is unchanged: no struct
 * crosses this boundary.  The Python binding is convexadam_amd/_prep.py (PREP_SIGNATURES).
 *
 * The parameter block ("params") is four float32 on the DEVICE: { mean, std, lo, hi }.
 */
#ifndef CONVEXADAM_PREP_H
#define CONVEXADAM_PREP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

#define CVX_PREP_CLAMP 1       /* flags of cvx_prep_stats_f32: x = min(max(x, clamp_lo), clamp_hi) as it is loaded (a NaN stays a NaN) */
#define CVX_PREP_POSITIVE 2    /*                              only elements with x > 0 count (a NaN does not) */

/* ---- statistics of a volume: mean, standard deviation, two quantiles --------------------------------------------------------------
 * Replaces   img.mean(), img.std(), torch.quantile(img, q) of nnUNetCTnorm (convex_adam_utils.py:163-167) and img[mask].mean(),
 *            img[mask].std() with mask = img > 0 of nnUNetNorm (:143-145); no host synchronisation, the results stay on the device.
 * Arithmetic, in operation order (n elements x[0 .. n); y = x, or the clamped x with CVX_PREP_CLAMP; an element "counts" unless
 * CVX_PREP_POSITIVE is set and !(y > 0)):
 *   moments, float64, the addition order of cvx_field_mean_f64 (no floating-point atomics):
 *     span b owns elements [b S, (b + 1) S), S = 4096 = 256 K, K = 16.  Thread t of the span adds its elements b S + k 256 + t,
 *     k = 0 .. 15 in that order, into one accumulator started at 0.0 (an element that does not count, or lies behind n, adds nothing).
 *     The 256 accumulators are combined by the stride-halving tree: s = 128, 64, .., 1: acc[t] += acc[t + s] for t < s.  acc[0] is the
 *     span's partial.  The finish lets thread t add partials t, t + 256, .. in order from 0.0 and runs the same tree.
 *     pass 1: the terms are (double)y; count = the number of elements that count (n without CVX_PREP_POSITIVE);
 *             mean = total / (double)count.
 *     pass 2: the terms are d * d with d = (double)y - mean (a product, then an addition: no fused multiply-add);  ss = total.
 *     params[0] = (float)mean;  params[1] = count > 1 ? (float)sqrt(ss / (double)(count - 1)) : NaN.  count = 0 gives a NaN mean (0 / 0);
 *     both as torch.
 *   quantiles (n_quantiles = 2; fractions q0, q1 as float32), torch.quantile's linear interpolation:
 *     n <= 2^24: rank = q * (float)(n - 1) in float32; below = floorf(rank), above = ceilf(rank), w = rank - below (float32).
 *     n >  2^24 (where torch.quantile refuses the input): rank = (double)q * (double)(n - 1); below = floor, above = ceil,
 *               w = (float)(rank - below).
 *     a, b = the order statistics `below` and `above` of y (exact: radix select over a monotone 32-bit key; -0.0 and +0.0 are equal,
 *     the result is +0.0), then  w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w)   in float32.
 *     If any element is NaN both quantiles are NaN.   params[2] = quantile q0, params[3] = quantile q1.
 *     With n_quantiles = 0: params[2] = -inf, params[3] = +inf.
 *   The volume is read three times with quantiles (sum + first histogram, centred squares + second histogram, third histogram),
 *   twice without.
 * moments3 (optional, device, 3 doubles): { (double)count, mean, ss }.
 * Refused   CVX_ERR_INVALID_ARG: x or params null; n < 1 or n > 2^31 - 1; unknown flag bits; n_quantiles not 0 or 2; a fraction
 *           outside [0, 1] or NaN; quantiles together with CVX_PREP_POSITIVE; clamp bounds NaN or lo > hi with CVX_PREP_CLAMP;
 *           an output overlapping x, the workspace or the other output.   CVX_ERR_WORKSPACE: workspace null or shorter than the query. */
size_t cvx_prep_stats_workspace_bytes(long long n);
int cvx_prep_stats_f32(const float* x, long long n, int flags, float clamp_lo, float clamp_hi, int n_quantiles, float q0, float q1,
                       float* params, double* moments3, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the elementwise step --------------------------------------------------------------------------------------------------------
 * Replaces   torch.clamp(img, lo, hi); (img - mean) / std   of nnUNetCTnorm (:168-169) and nnUNetNormProps (:156-157), and
 *            (img - mean) / (std + 1e-8); img[mask == 0] = 0   of nnUNetNorm (:146-147).
 * The parameter block comes from the device (params, as cvx_prep_stats_f32 left it) or from four host numbers (params_host =
 * { mean, std, lo, hi }, copied into the launch arguments); exactly one of the two is given.
 * Arithmetic, float32, in this order, IEEE division (never a multiplication by a reciprocal):
 *   mode 0:  t = x < lo ? lo : x;  t = t > hi ? hi : t;  out = (t - mean) / std                (a NaN x stays NaN, like torch.clamp)
 *   mode 1:  out = x > 0 ? (x - mean) / (std + 1e-8f) : 0                                       (lo, hi unused)
 * out may be x itself (in place) but must not overlap it otherwise.
 * Refused   CVX_ERR_INVALID_ARG: x or out null; both or neither of params / params_host; n < 1 or n > 2^31 - 1; mode not 0 or 1;
 *           out partially overlapping x; params overlapping out. */
int cvx_prep_normalise_f32(const float* x, long long n, const float* params, const float* params_host, int mode, float* out,
                           void* stream);

/* ---- non-zero mask with filled holes, its box and its count -----------------------------------------------------------------------
 * Replaces   create_nonzero_mask (:240-248): OR over the channels of data[c] != 0, then scipy.ndimage.binary_fill_holes (default
 *            6-connected structure; 4-connected for ndim = 2), and get_bbox_from_mask (:251-259) of the result.
 * data [C][H][W][D] float32 (ndim = 3), or [C][W][D] with H = 1 (ndim = 2).  Steps:
 *   1. mask = OR_c (data[c] != 0)  (a NaN is non-zero);  reached = !mask on the voxels that lie on a face of the array (the faces of the
 *      W and D axes only when ndim = 2).
 *   2. a round = for the axes H, W, D in this order (H skipped when ndim = 2) one launch, one thread per line: a forward walk, then a
 *      backward walk, with  carry = !mask[i] && (carry || reached[i]);  reached[i] |= carry.   Rounds repeat until one changes no voxel;
 *      the host reads one device flag per round (the call SYNCHRONISES the stream).  `reached` grows strictly in every round but the
 *      last, so at most H W D + 1 rounds run; past that cap the call returns CVX_ERR_LAUNCH.  No kernel waits for another workgroup.
 *   3. mask_out = mask | !reached (bytes 0 / 1);  box6 = { min, max + 1 } of the set voxels' indices per axis H, W, D (int32; an empty
 *      mask leaves { INT_MAX, 0 } per axis);  count = number of set voxels.  Integer atomics only.
 * rounds_host (optional, HOST int): rounds run, the last (unchanged) one included.   count (optional, device int64).
 * Refused   CVX_ERR_INVALID_ARG: data, mask_out or box6 null; C < 1; an extent < 1 or more than 2^31 - 1 voxels; C H W D >= 2^40 elements
 *           of data; ndim not 2 or 3;
 *           ndim = 2 with H != 1; outputs overlapping data, the workspace or each other.   CVX_ERR_WORKSPACE as above. */
size_t cvx_prep_nonzero_mask_workspace_bytes(int H, int W, int D);
int cvx_prep_nonzero_mask_u8(const float* data, int C, int H, int W, int D, int ndim, unsigned char* mask_out, int* box6, long long* count,
                             int* rounds_host, void* workspace, size_t workspace_bytes, void* stream);

/* ---- box of a byte mask -------------------------------------------------------------------------------------------------------------
 * Replaces   get_bbox_from_mask (:251-259) for a mask that is already on the device: mask [H][W][D] bytes, non-zero = set (the caller
 *            forms mask != outside_value).  box6 and count as above; the caller downloads the 24 bytes of box6.
 * Refused   CVX_ERR_INVALID_ARG: mask or box6 null; an extent < 1 or more than 2^31 - 1 voxels; outputs overlapping the mask or each other. */
int cvx_prep_mask_bbox_i32(const unsigned char* mask, int H, int W, int D, int* box6, long long* count, void* stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif

#endif /* CONVEXADAM_PREP_H */
