// rigidreg.hip -- the pieces of the CuRIOUS rigid registration script around its convex stage (l2r_2020_convexAdam_CuRIOUS.py):
//   k_threshold_pool_mask : F.avg_pool3d((img > t).float(), g, stride=g) > .5                          (:328,330)
//   k_label_centroids     : per label the voxel count and the three coordinate sums of mesh[:, idx]     (:312-316,378-380,387-389)
//   k_compact_cells, k_rigid_samples : the rigid fit's rows T1, T2 of the kept coarse cells, from the coarse field (:359-365)
#include "cvx_common.h"

namespace cvx {

// One thread per coarse cell.  The pooled value is count / g^3 with count the number of voxels above the threshold: an exact integer
// sum (< 2^24) and ONE correctly rounded division, so it exceeds 0.5 exactly when 2 * count > g^3 -- for 2 * count == g^3 the quotient is
// 0.5 itself, below it rounding is monotonic and stays <= 0.5, above it count / g^3 >= 0.5 + 1 / (2 g^3) lies at least one float spacing
// (2^-24) above 0.5 for g^3 <= 2^18.  A NaN voxel compares false, as in torch.
__global__ __launch_bounds__(256) void k_threshold_pool_mask(const float* __restrict__ img, int W, int D, float thresh, int g, int h,
                                                             int w, int d, unsigned char* __restrict__ mask) {
    const size_t v = (size_t)h * w * d;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v) return;
    const int x = (int)(i % d), y = (int)((i / d) % w), z = (int)(i / ((size_t)d * w));
    int count = 0;
    for (int a = 0; a < g; ++a)
        for (int b = 0; b < g; ++b) {
            const float* row = img + ((size_t)(z * g + a) * W + (size_t)(y * g + b)) * D + (size_t)x * g;
            for (int c = 0; c < g; ++c) count += row[c] > thresh ? 1 : 0;
        }
    mask[i] = 2 * count > g * g * g ? 1 : 0;
}

// acc[l] = {count, sum of the H coordinate, sum of the W coordinate, sum of the D coordinate} over the voxels with (int)seg == l.
// A wavefront whose 64 voxels carry one label (background, the inside of a structure) reduces them with shuffles and issues one set of
// LDS atomics; a mixed wavefront issues them per lane.  Each workgroup then adds its non-empty partials to `acc` with one 64-bit
// integer atomic per entry: integer sums, the same result on every run and for every launch shape.
__global__ __launch_bounds__(256) void k_label_centroids(const float* __restrict__ seg, int W, int D, size_t V, int max_label,
                                                         unsigned long long* __restrict__ acc) {
    extern __shared__ unsigned long long sh_acc[];
    for (int i = threadIdx.x; i < 4 * (max_label + 1); i += blockDim.x) sh_acc[i] = 0ull;
    cvx_barrier();
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
    const float top = (float)(max_label + 1);
    for (size_t i0 = wave * 64; i0 < V; i0 += nwaves * 64) {          // i0 is uniform in the wavefront: all 64 lanes stay in the loop
        const size_t i = i0 + lane;
        int l = -1;
        unsigned cx = 0, cy = 0, cz = 0;
        if (i < V) {
            const float f = seg[i];
            if (f > -1.0f && f < top) l = (int)f;                     // truncation, like .short() / cvx_label_histogram_i64; NaN: no label
            cx = (unsigned)(i % D); cy = (unsigned)((i / D) % W); cz = (unsigned)(i / ((size_t)D * W));
        }
        const int l0 = __shfl(l, 0);
        if (__all(l == l0)) {
            if (l0 < 0) continue;
            unsigned sx = cx, sy = cy, sz = cz;                       // 64 coordinates below 2^24: no overflow
            for (int o = 32; o > 0; o >>= 1) { sx += __shfl_down(sx, o); sy += __shfl_down(sy, o); sz += __shfl_down(sz, o); }
            if (lane == 0) {
                atomicAdd(&sh_acc[4 * l0], 64ull);
                atomicAdd(&sh_acc[4 * l0 + 1], (unsigned long long)sz);
                atomicAdd(&sh_acc[4 * l0 + 2], (unsigned long long)sy);
                atomicAdd(&sh_acc[4 * l0 + 3], (unsigned long long)sx);
            }
        } else if (l >= 0) {
            atomicAdd(&sh_acc[4 * l], 1ull);
            atomicAdd(&sh_acc[4 * l + 1], (unsigned long long)cz);
            atomicAdd(&sh_acc[4 * l + 2], (unsigned long long)cy);
            atomicAdd(&sh_acc[4 * l + 3], (unsigned long long)cx);
        }
    }
    cvx_barrier();
    for (int i = threadIdx.x; i < 4 * (max_label + 1); i += blockDim.x)
        if (sh_acc[i]) atomicAdd(&acc[i], sh_acc[i]);
}

// ---- rigid-fit samples straight from the coarse field (:354-365) ---------------------------------------------------------------------
// torch.nonzero order of the kept cells: one workgroup walks the mask in chunks of 1024 cells (ballot + per-wavefront counts)
__global__ __launch_bounds__(1024) void k_compact_cells(const unsigned char* __restrict__ mask, int v, int* __restrict__ list,
                                                        int* __restrict__ count) {
    __shared__ int wave_cnt[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) base = 0;
    cvx_barrier();
    for (int i0 = 0; i0 < v; i0 += 1024) {
        const int i = i0 + tid;
        const bool k = i < v && mask[i] != 0;
        const unsigned long long b = __ballot(k);
        if (lane == 0) wave_cnt[wv] = __popcll(b);
        cvx_barrier();
        int off = base;
        for (int q = 0; q < wv; ++q) off += wave_cnt[q];
        if (k) list[off + __popcll(b & ((1ull << lane) - 1ull))] = i;
        cvx_barrier();
        if (tid == 0) { int t = 0; for (int q = 0; q < 16; ++q) t += wave_cnt[q]; base += t; }
        cvx_barrier();
    }
    if (tid == 0) *count = base;
}

// One thread per kept cell: the rows T1 = grid_sample(identity volume) and T2 = grid_sample(identity + disp0) at the cell's
// F.affine_grid(eye, coarse) coordinate, as rigid.py::_field_samples forms them from a full-resolution field -- but every corner voxel's
// displacement is evaluated here from the COARSE field with k_resize's chain (lin_coef + resize_chain), then
// ident + disp.flip / (size - 1) * 2 in the reference's order, then cvx_grid_sample_f32's weights and corner order (tri_setup, the
// accumulation of tri_sample): bit-identical to _field_samples(resize(coarse)) without the 226 MB field and the coordinate volumes.
__global__ __launch_bounds__(64) void k_rigid_samples(const float* __restrict__ coarse, const int* __restrict__ list, int M, int h, int w,
                                                      int d, int H, int W, int D, const float* __restrict__ ch, const float* __restrict__ cw,
                                                      const float* __restrict__ cd, const float* __restrict__ bh,
                                                      const float* __restrict__ bw, const float* __restrict__ bd, float* __restrict__ T1,
                                                      float* __restrict__ T2) {
    const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (m >= M) return;
    const int c = list[m];
    const int x = c % d, y = (c / d) % w, z = c / (d * w);
    Tri t;
    tri_setup(t, cd[x], cw[y], ch[z], H, W, D);
    const float wt[8] = {t.tnw, t.tne, t.tsw, t.tse, t.bnw, t.bne, t.bsw, t.bse};
    const size_t cs = (size_t)h * w * d;
    const float sD = (float)(D - 1), sW = (float)(W - 1), sH = (float)(H - 1);
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                      // corner order of tri_sample: z slowest, x fastest
        const int Z = t.z0 + (k >> 2), Y = t.y0 + ((k >> 1) & 1), X = t.x0 + (k & 1);
        if (!inb3(Z, Y, X, H, W, D)) continue;                         // ATen adds the in-range corners only
        int z0, z1, y0, y1, x0, x1;
        float lz0, lz1, ly0, ly1, lx0, lx1;
        lin_coef(Z, h, H, z0, z1, lz0, lz1);
        lin_coef(Y, w, W, y0, y1, ly0, ly1);
        lin_coef(X, d, D, x0, x1, lx0, lx1);
        const size_t o00 = ((size_t)z0 * w + y0) * d, o01 = ((size_t)z0 * w + y1) * d, o10 = ((size_t)z1 * w + y0) * d,
                     o11 = ((size_t)z1 * w + y1) * d;
        float dv[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float* ic = coarse + (size_t)a * cs;
            const float v[8] = {ic[o00 + x0], ic[o00 + x1], ic[o01 + x0], ic[o01 + x1], ic[o10 + x0], ic[o10 + x1], ic[o11 + x0], ic[o11 + x1]};
            dv[a] = resize_chain(v, 1.0f, lx0, lx1, ly0, ly1, lz0, lz1);
        }
        const float i0 = bd[X], i1 = bw[Y], i2 = bh[Z];               // the identity volume, (x, y, z) channel order
        const float m0 = i0 + fdiv(dv[2], sD) * 2.0f, m1 = i1 + fdiv(dv[1], sW) * 2.0f, m2 = i2 + fdiv(dv[0], sH) * 2.0f;
        a0 = a0 + i0 * wt[k]; a1 = a1 + i1 * wt[k]; a2 = a2 + i2 * wt[k];
        b0 = b0 + m0 * wt[k]; b1 = b1 + m1 * wt[k]; b2 = b2 + m2 * wt[k];
    }
    T1[4 * (size_t)m] = a0; T1[4 * (size_t)m + 1] = a1; T1[4 * (size_t)m + 2] = a2; T1[4 * (size_t)m + 3] = 1.0f;
    T2[4 * (size_t)m] = b0; T2[4 * (size_t)m + 1] = b1; T2[4 * (size_t)m + 2] = b2; T2[4 * (size_t)m + 3] = 1.0f;
}

struct SamplesWs { int *list, *count; float *ch, *cw, *cd, *bh, *bw, *bd; };
static SamplesWs samples_layout(Carver& cv, int h, int w, int d, int H, int W, int D) {
    SamplesWs s;
    s.list = cv.take<int>((size_t)h * w * d);
    s.count = cv.take<int>(1);
    s.ch = cv.take<float>(h); s.cw = cv.take<float>(w); s.cd = cv.take<float>(d);
    s.bh = cv.take<float>(H); s.bw = cv.take<float>(W); s.bd = cv.take<float>(D);
    return s;
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_threshold_pool_mask_u8(const float* img, int H, int W, int D, float thresh, int g, unsigned char* mask, void* stream) {
    CVX_REQUIRE(img && mask, "cvx_threshold_pool_mask_u8: null pointer");
    CVX_REQUIRE(g >= 1 && g <= 64, "cvx_threshold_pool_mask_u8: grid spacing %d outside 1..64", g);
    CVX_REQUIRE(H >= g && W >= g && D >= g, "cvx_threshold_pool_mask_u8: extent %d x %d x %d smaller than one cell of %d", H, W, D, g);
    const int h = H / g, w = W / g, d = D / g;
    const size_t v = (size_t)h * w * d;
    hipLaunchKernelGGL(k_threshold_pool_mask, dim3((unsigned)cdiv64((int64_t)v, 256)), dim3(256), 0, as_stream(stream), img, W, D, thresh, g, h, w,
                       d, mask);
    return check_last("threshold_pool_mask");
}

extern "C" int cvx_label_centroids_i64(const float* seg, int H, int W, int D, int max_label, int64_t* acc, void* stream) {
    CVX_REQUIRE(seg && acc, "cvx_label_centroids_i64: null pointer");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0 && H < (1 << 24) && W < (1 << 24) && D < (1 << 24), "cvx_label_centroids_i64: bad extent %d x %d x %d", H, W, D);
    CVX_REQUIRE(max_label >= 0 && max_label < 1024, "cvx_label_centroids_i64: max_label %d outside 0..1023", max_label);
    hipStream_t s = as_stream(stream);
    const size_t n = 4 * (size_t)(max_label + 1), V = (size_t)H * W * D;
    if (hipMemsetAsync(acc, 0, sizeof(int64_t) * n, s) != hipSuccess) return fail(CVX_ERR_LAUNCH, "cvx_label_centroids_i64: memset failed");
    const int64_t want = cdiv64((int64_t)V, 256 * 16);
    const int nb = (int)(want < 1024 ? want : 1024);
    hipLaunchKernelGGL(k_label_centroids, dim3(nb), dim3(256), sizeof(unsigned long long) * n, s, seg, W, D, V, max_label,
                       reinterpret_cast<unsigned long long*>(acc));
    return check_last("label_centroids");
}

extern "C" size_t cvx_rigid_samples_workspace_bytes(int h, int w, int d, int H, int W, int D) {
    if (h < 1 || w < 1 || d < 1 || H < 1 || W < 1 || D < 1) return 0;
    Carver m;
    samples_layout(m, h, w, d, H, W, D);
    return ws_query(m);
}

extern "C" int cvx_rigid_samples_f32(const float* coarse_field, const unsigned char* mask, int h, int w, int d, int H, int W, int D, float* T1,
                                     float* T2, int64_t* count_host, void* workspace, size_t workspace_bytes, void* stream) {
    CVX_REQUIRE(coarse_field && mask && T1 && T2 && count_host && workspace, "cvx_rigid_samples_f32: null pointer");
    CVX_REQUIRE(h >= 1 && w >= 1 && d >= 1 && H >= 2 && W >= 2 && D >= 2 && (double)h * w * d < 2.0e9, "cvx_rigid_samples_f32: bad extents");
    if (workspace_bytes < cvx_rigid_samples_workspace_bytes(h, w, d, H, W, D)) return fail(CVX_ERR_WORKSPACE, "cvx_rigid_samples_f32: workspace too small");
    hipStream_t s = as_stream(stream);
    Carver cv(workspace);
    const SamplesWs L = samples_layout(cv, h, w, d, H, W, D);
    const int v = h * w * d;
    hipLaunchKernelGGL(k_compact_cells, dim3(1), dim3(1024), 0, s, mask, v, L.list, L.count);
    int rc;
    if ((rc = cvx_affine_base_f32(h, L.ch, stream)) || (rc = cvx_affine_base_f32(w, L.cw, stream)) || (rc = cvx_affine_base_f32(d, L.cd, stream)) ||
        (rc = cvx_affine_base_f32(H, L.bh, stream)) || (rc = cvx_affine_base_f32(W, L.bw, stream)) || (rc = cvx_affine_base_f32(D, L.bd, stream))) return rc;
    int M = 0;                                     // the one value that has to reach the host: the fit needs the number of rows
    if (hipMemcpyAsync(&M, L.count, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(CVX_ERR_LAUNCH, "cvx_rigid_samples_f32: reading the cell count failed");
    *count_host = M;
    if (M > 0)
        hipLaunchKernelGGL(k_rigid_samples, dim3((unsigned)cdiv(M, 64)), dim3(64), 0, s, coarse_field, L.list, M, h, w, d, H, W, D, L.ch, L.cw, L.cd, L.bh,
                           L.bw, L.bd, T1, T2);
    return check_last("rigid_samples");
}
