// affine.hip -- the affine model (include/convexadam_affine.h): least_trimmed_squares of l2r_2020_convexAdam_CuRIOUS.py:272-278
// and the affine map of F.affine_grid as a displacement field.
//
//   lts     k_affine_lts: the whole least-trimmed affine fit in ONE launch of one 1024-thread workgroup, built like k_rigid_lts.  Fit 0 uses
//           all n points, every later fit the n/2 points with the smallest residuals under the previous fit.  Per fit:
//             1. two 4 x 4 float64 moment matrices over the set, A = L^T F and B = L^T M (L = F for normal = 0, the least-squares normal
//                equations; L = M for normal = 1, the reference's torch.solve(M^T M, M^T F)), summed in the fixed order of lts_common.h
//                (wg_sum): no atomics, the same bits on every run.  Two walks of 16 sums each keep the accumulators in registers;
//             2. one lane solves A X = B in float64 (affine_core.h::affine_solve4: Gaussian elimination with partial pivoting) and stores X
//                as float32; normal = 0 solves three columns and writes the fourth as (0, 0, 0, 1).  A non-finite moment or a zero or
//                non-finite pivot leaves a status word and stops the kernel before X or the inlier mask is written;
//             3. unless it is the last fit: the float32 residuals and the selection of lts_common.h (lts_select) -- the rigid fit's code.
//   field   k_affine_field: out(x) = A(x + u(x)) - x, one thread per voxel, float64, the arithmetic of affine_core.h; u is read once, out
//           written once, theta comes from device memory (12 wave-uniform loads), so a fitted T feeds it without a host round trip.
// Neither is on the timed path of bench.py.
#include <limits.h>
#include <math.h>

#include "cvx_common.h"
#include "lts_common.h"
#include "interp_f64.h"
#include "geometry_args.h"
#include "affine_core.h"
#include "convexadam_affine.h"

namespace cvx {

constexpr int64_t AFFINE_MIN_N = 4;
constexpr int AFFINE_MAX_LD = 1 << 20;

// a point row as four floats; ld == 3: the homogeneous 1 is implied
__device__ __forceinline__ void load_row(const float* __restrict__ p, int ld, float (&r)[4]) {
    r[0] = p[0]; r[1] = p[1]; r[2] = p[2];
    r[3] = ld >= 4 ? p[3] : 1.0f;
}

__global__ __launch_bounds__(LTS_THREADS) void k_affine_lts(const float* __restrict__ fixed, int ldf, const float* __restrict__ moving, int ldm,
                                                            int n, int iters, int normal, float* __restrict__ X,
                                                            unsigned char* __restrict__ inliers, unsigned* rbits, unsigned char* sel,
                                                            int* __restrict__ status) {
    __shared__ double red[LTS_WAVES * 16], tot[16], aug[4][8];
    __shared__ LtsSelectLds lds;
    __shared__ float Xs[16];          // X row-major
    __shared__ int flag;
    const int tid = threadIdx.x;
    const int K = n / 2, nrhs = normal ? 4 : 3;
    int mode = 0, bad = 0;
    unsigned thr = 0;
    for (int it = 0; it < iters; ++it) {
        for (int half = 0; half < 2; ++half) {                                  // A = L^T F, then B = L^T M
            double acc[16];
            for (int k = 0; k < 16; ++k) acc[k] = 0.0;
            for (int i = tid; i < n; i += LTS_THREADS)
                if (in_set(mode, i, rbits, sel, thr)) {
                    float f[4], m[4];
                    load_row(fixed + (size_t)i * ldf, ldf, f);
                    load_row(moving + (size_t)i * ldm, ldm, m);
                    float l[4], r[4];
                    for (int a = 0; a < 4; ++a) { l[a] = normal ? m[a] : f[a]; r[a] = half ? m[a] : f[a]; }
                    const int nc = half ? nrhs : 4;
                    for (int a = 0; a < 4; ++a)
                        for (int b = 0; b < 4; ++b)
                            if (b < nc) acc[4 * a + b] += (double)l[a] * (double)r[b];
                }
            wg_sum<16>(acc, red, tot);
            if (tid < 16) aug[tid >> 2][4 * half + (tid & 3)] = tot[tid];
        }
        cvx_barrier();
        if (tid == 0) {
            const int rc = affine_solve4(aug, nrhs);
            flag = rc;
            if (rc == AFFINE_FIT_OK)
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 4; ++b) Xs[4 * a + b] = b < nrhs ? (float)aug[a][4 + b] : (a == 3 ? 1.0f : 0.0f);
        }
        cvx_barrier();
        bad = flag;
        if (bad) break;                                                         // uniform: every thread read the same flag
        if (it == iters - 1) break;

        // residuals + selection of the K points with the smallest patterns; Xc holds X by columns
        float Xc[16];
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) Xc[4 * b + a] = Xs[4 * a + b];
        if (normal)
            mode = lts_select(n, K, rbits, sel, lds, thr, [&](int i) { return residual_bits<false>(fixed + (size_t)i * ldf, moving + (size_t)i * ldm, Xc); });
        else
            mode = lts_select(n, K, rbits, sel, lds, thr, [&](int i) { return residual_bits<true>(fixed + (size_t)i * ldf, moving + (size_t)i * ldm, Xc); });
    }
    if (!bad) {
        if (tid < 16) X[tid] = Xs[tid];
        if (inliers)
            for (int i = tid; i < n; i += LTS_THREADS) inliers[i] = (unsigned char)in_set(mode, i, rbits, sel, thr);
    }
    if (tid == 0) *status = bad;
}

template <typename TU, typename TO>
__global__ __launch_bounds__(256) void k_affine_field(const float* __restrict__ theta, int H, int W, int D, const TU* __restrict__ u, size_t ucs,
                                                      size_t uvs, TO* __restrict__ out, size_t ocs, size_t ovs) {
    const unsigned V = (unsigned)H * (unsigned)W * (unsigned)D;               // at most 2^31 - 1, and at most 2^28 threads: q + stride < 2^32
    float th[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) th[k] = theta[k];
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < V; q += gridDim.x * 256u) {
        const unsigned r = q / (unsigned)D, i01 = r / (unsigned)W;
        const int i2 = (int)(q - r * (unsigned)D), i1 = (int)(r - i01 * (unsigned)W), i0 = (int)i01;
        double o[3];
        affine_field_voxel(th, u, ucs, uvs, H, W, D, i0, i1, i2, o);
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a * ocs + (size_t)q * ovs] = (TO)o[a];     // float: round to nearest
    }
}

template <typename TU, typename TO>
static void launch_affine_field(const float* theta, int H, int W, int D, const void* u, size_t ucs, size_t uvs, void* out, size_t ocs, size_t ovs,
                                hipStream_t s) {
    const long long blocks = cdiv64((int64_t)H * W * D, 256);
    hipLaunchKernelGGL((k_affine_field<TU, TO>), dim3((unsigned)(blocks < (1ll << 20) ? blocks : (1ll << 20))), dim3(256), 0, s, theta, H, W, D,
                       static_cast<const TU*>(u), ucs, uvs, static_cast<TO*>(out), ocs, ovs);
}


}  // namespace cvx

using namespace cvx;

extern "C" size_t cvx_affine_lts_workspace_bytes(int64_t n) {
    if (n < AFFINE_MIN_N || n > LTS_MAX_N) return 0;
    Carver m; lts_layout(m, n); return ws_query(m);
}

extern "C" int cvx_affine_lts_f32(const float* fixed, int ld_fixed, const float* moving, int ld_moving, int64_t n, int iters, int normal, float* X,
                                  unsigned char* inliers, void* workspace, size_t workspace_bytes, void* stream) {
    CVX_REQUIRE(fixed && moving && X && workspace, "cvx_affine_lts_f32: null pointer");
    CVX_REQUIRE(n >= AFFINE_MIN_N && n <= LTS_MAX_N, "cvx_affine_lts_f32: n = %lld outside %lld..%lld", (long long)n, (long long)AFFINE_MIN_N,
                (long long)LTS_MAX_N);
    CVX_REQUIRE(iters >= 1, "cvx_affine_lts_f32: iters = %d < 1", iters);
    CVX_REQUIRE(normal == 0 || normal == 1, "cvx_affine_lts_f32: normal %d is neither 0 (least squares) nor 1 (the reference's equation)", normal);
    CVX_REQUIRE(iters == 1 || n >= 8, "cvx_affine_lts_f32: the trimmed fit needs n >= 8 (n / 2 >= 4 points per fit), got %lld", (long long)n);
    const int ld_min = iters == 1 && normal == 0 ? 3 : 4;
    CVX_REQUIRE(ld_fixed >= ld_min && ld_moving >= ld_min && ld_fixed <= AFFINE_MAX_LD && ld_moving <= AFFINE_MAX_LD,
                "cvx_affine_lts_f32: ld %d, %d outside %d..%d (three columns only for a single fit with normal = 0)", ld_fixed, ld_moving, ld_min,
                AFFINE_MAX_LD);
    CVX_REQUIRE(field_aligned(fixed, 0) && field_aligned(moving, 0) && field_aligned(X, 0), "cvx_affine_lts_f32: a buffer is not aligned to 4 bytes");
    const size_t fb = ((size_t)(n - 1) * ld_fixed + (ld_fixed >= 4 ? 4 : 3)) * 4, mb = ((size_t)(n - 1) * ld_moving + (ld_moving >= 4 ? 4 : 3)) * 4;
    const Span ins[2] = {{fixed, fb}, {moving, mb}}, outs[2] = {{X, 64}, {inliers, (size_t)n}};
    const Overlaps ov = find_overlaps(outs, ins);
    CVX_REQUIRE(ov.out != 0, "cvx_affine_lts_f32: X overlaps the points");
    CVX_REQUIRE(ov.out < 0 && ov.a < 0, "cvx_affine_lts_f32: inliers overlaps the points or X");
    const size_t need = cvx_affine_lts_workspace_bytes(n);
    if (workspace_bytes < need) return fail(CVX_ERR_WORKSPACE, "cvx_affine_lts_f32: workspace %zu < %zu bytes", workspace_bytes, need);
    Carver cv(workspace);
    const auto [rbits, sel, status] = lts_layout(cv, n);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_affine_lts, dim3(1), dim3(LTS_THREADS), 0, s, fixed, ld_fixed, moving, ld_moving, (int)n, iters, normal, X, inliers, rbits,
                       sel, status);
    int rc = check_last("affine_lts");
    if (rc != CVX_OK) return rc;
    int h_status = 0;
    if (hipMemcpyAsync(&h_status, status, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CVX_ERR_LAUNCH, "cvx_affine_lts_f32: reading the fit status failed");
    }
    if (h_status == AFFINE_FIT_NON_FINITE)
        return fail(CVX_ERR_INVALID_ARG, "cvx_affine_lts_f32: non-finite moment matrix (a non-finite coordinate among the points of a fit); X not written");
    if (h_status)
        return fail(CVX_ERR_INVALID_ARG, "cvx_affine_lts_f32: singular system (a zero or non-finite pivot: coplanar points?); X not written");
    return CVX_OK;
}

extern "C" int cvx_affine_field_f64(const float* theta, int H, int W, int D, const void* u, int u_f64, int64_t u_comp_stride, int64_t u_voxel_stride,
                                    void* out, int out_f64, int64_t out_comp_stride, int64_t out_voxel_stride, void* stream) {
    CVX_REQUIRE(theta && out, "cvx_affine_field_f64: null pointer");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_affine_field_f64: bad extent (%dx%dx%d)", H, W, D);
    const size_t V = voxels(H, W, D);
    CVX_REQUIRE(V, "cvx_affine_field_f64: more than 2^31 - 1 voxels (%dx%dx%d)", H, W, D);
    const FieldArg fu = {u, u_f64, u_comp_stride, u_voxel_stride}, fo = {out, out_f64, out_comp_stride, out_voxel_stride};
    CVX_REQUIRE(!u || fu.strides_ok(V), "cvx_affine_field_f64: bad field strides of u (component %lld, voxel %lld)", (long long)u_comp_stride,
                (long long)u_voxel_stride);
    CVX_REQUIRE(fo.strides_ok(V), "cvx_affine_field_f64: bad field strides of out (component %lld, voxel %lld)", (long long)out_comp_stride,
                (long long)out_voxel_stride);
    CVX_REQUIRE(field_aligned(theta, 0) && fu.aligned() && fo.aligned(), "cvx_affine_field_f64: a buffer is not aligned to its element");
    const Span ins[2] = {{theta, 48}, fu.span(V)}, outs[1] = {fo.span(V)};
    CVX_REQUIRE(find_overlaps(outs, ins).out < 0, "cvx_affine_field_f64: out overlaps an input");
    hipStream_t s = as_stream(stream);
    const size_t ucs = u ? (size_t)u_comp_stride : 0, uvs = u ? (size_t)u_voxel_stride : 0, ocs = (size_t)out_comp_stride, ovs = (size_t)out_voxel_stride;
    with_real(u && u_f64, [&](auto tu) {                                        // no u: the float instance, whatever u_f64 says
        with_real(out_f64, [&](auto to) { launch_affine_field<decltype(tu), decltype(to)>(theta, H, W, D, u, ucs, uvs, out, ocs, ovs, s); });
    });
    return check_last("affine_field");
}
