// rigid.hip -- least-trimmed rigid fit and fused affine warp (l2r_2020_convexAdam_CuRIOUS.py:349-390; find_rigid_3d and
// least_trimmed_rigid of convex_adam_utils.py:173-193).
//
//   lts     k_rigid_lts: the whole least-trimmed fit in ONE launch of one 1024-thread workgroup.  Fit 0 uses all n points, every later
//           fit the n/2 points with the smallest residuals under the previous fit.  Per fit:
//             1. centroids x_bar, y_bar of columns 0..2 over the set, then the centred cross-covariance H = sum (x - x_bar)(y - y_bar)^T,
//                both in float64 in a fixed order (each thread walks i = tid, tid + 1024, ... in order, then a shuffle butterfly inside
//                each wave, then the 16 wave sums in wave order): no atomics, so the result is the same bit for bit on every run;
//             2. one lane solves for the optimal proper rotation in float64 by Horn's quaternion method (the eigenvector of the largest
//                eigenvalue of the symmetric 4x4 matrix built from H, cyclic Jacobi): the same rotation as the reference's Kabsch SVD
//                with its diag(1, 1, det(V U^T)) fix, without a separate reflection case; t = y_bar - R x_bar; T stored as float32;
//             3. unless it is the last fit: float32 residuals r_i = || moving_i - fixed_i T^T || over all four columns (the reference's
//                expression), as bit patterns in the workspace (non-negative floats order like their bits; NaN is mapped to 0x7fffffff
//                so it sorts last, as in torch.topk), then a three-pass radix select (11 + 11 + 10 bits, LDS histograms) of the n/2-th
//                smallest pattern t.  The next set is {r < t} plus the LOWEST-INDEX points with r == t until n/2 are chosen (torch
//                leaves the order of ties unspecified); when every r == t point is needed the set is simply {r <= t} and no pass is
//                spent on it, otherwise an ordered ballot scan writes the set as a byte mask.
//           Every global word a thread reads back (patterns, set mask, inlier mask) is one it wrote itself: the strided walk gives
//           point i to thread i % 1024 in every pass, so the passes need nothing beyond the workgroup barriers between them.
//           The workgroup sum, the residual pattern and the selection live in lts_common.h, shared with the affine fit (affine.hip).
//           A non-finite centroid or covariance (a non-finite coordinate among the points a fit uses; the reference's torch.svd raises
//           on it) stops the kernel before T or the inlier mask is written and leaves status = 1, which the host reads back.
//   warp    k_affine_warp: F.grid_sample(vol, F.affine_grid(theta, (1,C,ho,wo,do), align_corners=False), mode, zeros, False) with the
//           grid computed in the kernel: the affine_grid base coordinates (cvx_affine_base_host's formula; x along do, y along wo,
//           z along ho), then a = bx th[i][0]; a = fma(by, th[i][1], a); a = fma(bz, th[i][2], a); a = a + th[i][3] -- the chain
//           that equals ATen's CPU affine_grid bit for bit -- and ATen's unnormalisation.  Bilinear: the corner weights and
//           interpolation order of cvx_grid_sample_f32 (tri_setup / tri_sample); nearest: rintf (round half to even, ATen's
//           nearbyint).  theta lives in device memory, so a fitted T feeds the warp without a host round trip; the C channels share
//           one coordinate computation.
#include "cvx_common.h"
#include "lts_common.h"

namespace cvx {

// ---- least-trimmed rigid fit (workgroup sum, residual pattern and selection: lts_common.h) ---------------------------------------------
// Eigen-decomposition of a symmetric 4x4 matrix by cyclic Jacobi rotations (A is diagonalised in place, V gets the eigenvectors).
__device__ void jacobi4(double A[4][4], double V[4][4]) {
    for (int p = 0; p < 4; ++p)
        for (int q = 0; q < 4; ++q) V[p][q] = p == q ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 4; ++p) {
            diag += A[p][p] * A[p][p];
            for (int q = p + 1; q < 4; ++q) off += A[p][q] * A[p][q];
        }
        if (!(off > 1e-30 * diag)) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double at = fabs(theta);
                double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {                                   // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {                                   // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 4; ++k) {                                   // V <- V J
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// Optimal proper rotation R (y ~ R x + t) for the centred cross-covariance S[a][b] = sum x'_a y'_b (Horn 1987), T = [R t] as float32.
__device__ void horn_rotation(const double S[9], const double xm[3], const double ym[3], float* T12) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4];
    jacobi4(N, V);
    double best = N[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];      // first largest eigenvalue
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (N[k][k] > best) { best = N[k][k]; q0 = V[0][k]; q1 = V[1][k]; q2 = V[2][k]; q3 = V[3][k]; }
    const double nq = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    q0 /= nq; q1 /= nq; q2 /= nq; q3 /= nq;
    const double R[3][3] = {{q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2.0 * (q1 * q2 - q0 * q3), 2.0 * (q1 * q3 + q0 * q2)},
                            {2.0 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2.0 * (q2 * q3 - q0 * q1)},
                            {2.0 * (q1 * q3 - q0 * q2), 2.0 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3}};
    for (int a = 0; a < 3; ++a) {
        const double t = ym[a] - (R[a][0] * xm[0] + R[a][1] * xm[1] + R[a][2] * xm[2]);
        for (int b = 0; b < 3; ++b) T12[4 * a + b] = (float)R[a][b];
        T12[4 * a + 3] = (float)t;
    }
}

__global__ __launch_bounds__(LTS_THREADS) void k_rigid_lts(const float* __restrict__ fixed, int ldf, const float* __restrict__ moving, int ldm,
                                                           int n, int iters, float* __restrict__ T, unsigned char* __restrict__ inliers,
                                                           unsigned* rbits, unsigned char* sel, int* __restrict__ status) {
    __shared__ double red[LTS_WAVES * 9], tot[9];
    __shared__ LtsSelectLds lds;
    __shared__ float T12[12];
    const int tid = threadIdx.x;
    const int K = n / 2;
    int mode = 0, bad = 0;
    unsigned thr = 0;
    for (int it = 0; it < iters; ++it) {
        const double cnt = it == 0 ? (double)n : (double)K;
        double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += LTS_THREADS)
            if (in_set(mode, i, rbits, sel, thr)) {
                const float* f = fixed + (size_t)i * ldf;
                const float* m = moving + (size_t)i * ldm;
                for (int a = 0; a < 3; ++a) { c[a] += (double)f[a]; c[3 + a] += (double)m[a]; }
            }
        wg_sum<6>(c, red, tot);
        double xm[3], ym[3];
        for (int a = 0; a < 3; ++a) { xm[a] = tot[a] / cnt; ym[a] = tot[3 + a] / cnt; }
        double h[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += LTS_THREADS)
            if (in_set(mode, i, rbits, sel, thr)) {
                const float* f = fixed + (size_t)i * ldf;
                const float* m = moving + (size_t)i * ldm;
                const double dx[3] = {(double)f[0] - xm[0], (double)f[1] - xm[1], (double)f[2] - xm[2]};
                const double dy[3] = {(double)m[0] - ym[0], (double)m[1] - ym[1], (double)m[2] - ym[2]};
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) h[3 * a + b] += dx[a] * dy[b];
            }
        wg_sum<9>(h, red, tot);
        for (int k = 0; k < 9; ++k) bad |= !isfinite(tot[k]);
        for (int a = 0; a < 3; ++a) bad |= !isfinite(xm[a]) || !isfinite(ym[a]);
        if (bad) break;                                                         // uniform: every thread read the same totals
        if (tid == 0) {
            double S[9];
            for (int k = 0; k < 9; ++k) S[k] = tot[k];
            horn_rotation(S, xm, ym, T12);
        }
        cvx_barrier();
        if (it == iters - 1) break;

        // residuals + selection of the K points with the smallest patterns
        float Tl[12];
        for (int k = 0; k < 12; ++k) Tl[k] = T12[k];
        mode = lts_select(n, K, rbits, sel, lds, thr, [&](int i) { return residual_bits<true>(fixed + (size_t)i * 4, moving + (size_t)i * 4, Tl); });
    }
    if (!bad) {
        if (tid < 16) T[tid] = tid < 12 ? T12[tid] : (tid == 15 ? 1.0f : 0.0f);
        if (inliers)
            for (int i = tid; i < n; i += LTS_THREADS) inliers[i] = (unsigned char)in_set(mode, i, rbits, sel, thr);
    }
    if (tid == 0) *status = bad;
}

// ---- fused affine_grid + grid_sample -----------------------------------------------------------------------------------------------
// F.affine_grid's base coordinate i of an axis of size S (align_corners=False): linspace(-1, 1, S)[i] * (S - 1) / S; S == 1 -> 0
__device__ __forceinline__ float affine_base_at(int i, int S) {
    if (S <= 1) return 0.0f;
    const float step = 2.0f / (float)(S - 1);
    const float lin = (i < S / 2) ? __builtin_fmaf(step, (float)i, -1.0f) : __builtin_fmaf(-step, (float)(S - 1 - i), 1.0f);
    return fdiv(lin * (float)(S - 1), (float)S);
}

template <bool NEAREST>
__global__ __launch_bounds__(256) void k_affine_warp(const float* __restrict__ vol, int C, int h, int w, int d, const float* __restrict__ th,
                                                     int ho, int wo, int dd, float* __restrict__ out) {
    const unsigned vo = (unsigned)ho * (unsigned)wo * (unsigned)dd;
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= vo) return;
    const unsigned r = p / (unsigned)dd, k = p - r * (unsigned)dd, i = r / (unsigned)wo, j = r - i * (unsigned)wo;
    const float bx = affine_base_at((int)k, dd), by = affine_base_at((int)j, wo), bz = affine_base_at((int)i, ho);
    float g[3];
    for (int a = 0; a < 3; ++a) {
        float acc = bx * th[4 * a];
        acc = __builtin_fmaf(by, th[4 * a + 1], acc);
        acc = __builtin_fmaf(bz, th[4 * a + 2], acc);
        g[a] = acc + th[4 * a + 3];
    }
    const size_t vi = (size_t)h * w * d;
    if (NEAREST) {
        const float fx = rintf(unnormalize(g[0], d)), fy = rintf(unnormalize(g[1], w)), fz = rintf(unnormalize(g[2], h));
        const bool inside = fz >= 0.0f && fz <= (float)(h - 1) && fy >= 0.0f && fy <= (float)(w - 1) && fx >= 0.0f && fx <= (float)(d - 1);
        const size_t src = inside ? ((size_t)(int)fz * w + (int)fy) * d + (int)fx : 0;
        for (int c = 0; c < C; ++c) out[(size_t)c * vo + p] = inside ? vol[(size_t)c * vi + src] : 0.0f;
    } else {
        Tri t;
        tri_setup(t, g[0], g[1], g[2], h, w, d);
        for (int c = 0; c < C; ++c) out[(size_t)c * vo + p] = tri_sample(t, vol + (size_t)c * vi, h, w, d);
    }
}

}  // namespace cvx

using namespace cvx;

extern "C" size_t cvx_rigid_lts_workspace_bytes(int64_t n) {
    if (n < 2 || n > LTS_MAX_N) return 0;
    Carver m; lts_layout(m, n); return align_up(m.used, 256);          // (no slack: the status word rounded to its granule, as this query always was)
}

extern "C" int cvx_rigid_lts_f32(const float* fixed, int ld_fixed, const float* moving, int ld_moving, int64_t n, int iters, float* T,
                                 unsigned char* inliers, void* workspace, size_t workspace_bytes, void* stream) {
    CVX_REQUIRE(fixed && moving && T && workspace, "cvx_rigid_lts_f32: null pointer");
    CVX_REQUIRE(n >= 2 && n <= LTS_MAX_N, "cvx_rigid_lts_f32: n = %lld outside 2..%lld", (long long)n, (long long)LTS_MAX_N);
    CVX_REQUIRE(iters >= 1, "cvx_rigid_lts_f32: iters = %d < 1", iters);
    if (iters == 1)
        CVX_REQUIRE(ld_fixed >= 3 && ld_moving >= 3, "cvx_rigid_lts_f32: a single fit needs ld >= 3 (got %d, %d)", ld_fixed, ld_moving);
    else
        CVX_REQUIRE(ld_fixed == 4 && ld_moving == 4, "cvx_rigid_lts_f32: the trimmed fit needs (n, 4) points (ld %d, %d)", ld_fixed, ld_moving);
    const size_t need = cvx_rigid_lts_workspace_bytes(n);
    if (workspace_bytes < need) return fail(CVX_ERR_WORKSPACE, "cvx_rigid_lts_f32: workspace %zu < %zu bytes", workspace_bytes, need);
    Carver cv(workspace);
    const auto [rbits, sel, status] = lts_layout(cv, n);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_rigid_lts, dim3(1), dim3(LTS_THREADS), 0, s, fixed, ld_fixed, moving, ld_moving, (int)n, iters, T, inliers, rbits, sel, status);
    int rc = check_last("rigid_lts");
    if (rc != CVX_OK) return rc;
    int h_status = 0;
    if (hipMemcpyAsync(&h_status, status, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CVX_ERR_LAUNCH, "cvx_rigid_lts_f32: reading the fit status failed");
    }
    if (h_status)
        return fail(CVX_ERR_INVALID_ARG, "cvx_rigid_lts_f32: non-finite centroid or cross-covariance (a non-finite coordinate among the "
                    "points of a fit); T not written");
    return CVX_OK;
}

extern "C" int cvx_affine_warp_f32(const float* vol, int C, int h, int w, int d, const float* theta, int ho, int wo, int dd, int mode,
                                   float* out, void* stream) {
    CVX_REQUIRE(vol && theta && out, "cvx_affine_warp_f32: null pointer");
    CVX_REQUIRE(C > 0 && h > 0 && w > 0 && d > 0 && ho > 0 && wo > 0 && dd > 0, "cvx_affine_warp_f32: bad extent");
    CVX_REQUIRE(mode == 0 || mode == 1, "cvx_affine_warp_f32: mode %d is neither 0 (bilinear) nor 1 (nearest)", mode);
    const uint64_t vo = (uint64_t)ho * (uint64_t)wo * (uint64_t)dd;
    if (vo > 0xffffff00ull) return fail(CVX_ERR_UNSUPPORTED, "cvx_affine_warp_f32: %llu output voxels exceed 2^32", (unsigned long long)vo);
    const dim3 grid((unsigned)cdiv64((int64_t)vo, 256));
    if (mode == 1) hipLaunchKernelGGL(k_affine_warp<true>, grid, dim3(256), 0, as_stream(stream), vol, C, h, w, d, theta, ho, wo, dd, out);
    else hipLaunchKernelGGL(k_affine_warp<false>, grid, dim3(256), 0, as_stream(stream), vol, C, h, w, d, theta, ho, wo, dd, out);
    return check_last("affine_warp");
}
