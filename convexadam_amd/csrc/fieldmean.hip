// fieldmean.hip -- the reduction of convex_adam_translation (convex_adam_translation.py:88-103): the sum of a displacement
// field over the voxels that count, and their number, so that the host divides three sums by one count instead of downloading the field.
//   k_field_mean_blocks   reads the field once where it lies (float32 or float64, any layout the two strides describe), optionally through
//                         convex_adam_pt's float16 round trip, and decides per voxel whether it counts: always, by a byte mask, or by
//                         sampling a segmentation on its own grid exactly as k_resample_linear does (same index map, same float64 taps,
//                         same cast) and testing `> 0` -- the resampled segmentation is never written
//   k_field_mean_finish   one workgroup adds the block partials
// The ORDER of the float64 additions is the contract (no floating-point atomics, nothing that depends on scheduling):
//   voxel v = (z W + y) D + x; block b owns [b S, (b + 1) S), S = 256 K, K = 16; thread t adds its voxels b S + k 256 + t, k = 0 .. K - 1, in
//   that order into three accumulators started at 0.0 (an excluded voxel adds nothing); the 256 accumulators of a block are combined by
//   the stride-halving tree (s = 128, 64, .., 1: acc[t] += acc[t + s] for t < s; LDS across wavefronts, __shfl_down inside one); the finish
//   lets thread t add partials t, t + 256, .. in order from 0.0 and runs the same tree.  Counts are integers.
// HBM-bound: 12 (float32) or 24 bytes read per voxel, + 1 with a mask; the segmentation taps are served by the caches.
#include <type_traits>

#include <hip/hip_fp16.h>

#include "cvx_common.h"
#include "interp_f64.h"
#include "geometry_args.h"

namespace cvx {

constexpr int FM_THREADS = 256;                     // the tree below is written for 256 threads = 4 wavefronts of 64
constexpr int FM_K = 16;                            // voxels per thread
constexpr int FM_SPAN = FM_THREADS * FM_K;          // S: voxels per block
enum { FM_ALL = 0, FM_MASK = 1, FM_SEG = 2 };

// workspace: the block partials, sums [3][nblocks] and counts [nblocks] -- ONE layout for the size query and the launcher
struct FieldMeanWs { double* sums; long long* counts; };
static FieldMeanWs field_mean_layout(Carver& c, size_t nblocks) {
    FieldMeanWs w;
    w.sums = c.take<double>(3 * nblocks);
    w.counts = c.take<long long>(nblocks);
    return w;
}

// acc[t] += acc[t + s] for s = 128 .. 1, t < s; thread 0 ends with the block's totals
__device__ __forceinline__ void fm_tree(double (&a)[3], long long& n, double (*sm)[FM_THREADS], long long* sn) {
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) sm[c][t] = a[c];
    sn[t] = n;
    cvx_barrier();
    if (t < 128) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] += sm[c][t + 128]; sm[c][t] = a[c]; }
        n += sn[t + 128];
        sn[t] = n;
    }
    cvx_barrier();
    if (t < 64) {                                   // wavefront 0, whole
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] += sm[c][t + 64];
        n += sn[t + 64];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {         // lane t < s reads lane t + s < 2 s, which the step before left valid
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] += __shfl_down(a[c], s, 64);
            n += __shfl_down(n, s, 64);
        }
    }
}

// does output voxel p = (z W + y) D + x count?  the segmentation sampled as k_resample_linear samples it (default 0), then the cast
// resample_device applies to a source of that kind, then `> 0`
template <typename TS>
__device__ __forceinline__ bool fm_seg_counts(const TS* __restrict__ seg, int sz, int sy, int sx, const IndexMap& g, int kind, size_t p, int W,
                                              int D) {
    const double i = (double)(int)(p % D), j = (double)(int)((p / D) % W), k = (double)(int)(p / ((size_t)D * W));
    const double cx = index_map_axis(g, 0, i, j, k), cy = index_map_axis(g, 1, i, j, k), cz = index_map_axis(g, 2, i, j, k);
    double r = 0.0;
    if (itk_inside(cx, sx) && itk_inside(cy, sy) && itk_inside(cz, sz))
        r = taps_linear_f64(seg, 1, sz, sy, sx, itk_clamp(cz, sz), itk_clamp(cy, sy), itk_clamp(cx, sx));
    if (kind == 2) return rint(r) > 0.0;            // integer source: half to even, like torch.round / np.rint
    if (kind == 1) return (float)r > 0.0f;          // float32 source: the round-to-nearest cast of the resampled volume
    return r > 0.0;
}

template <typename TF, int MODE, typename TS>
__global__ __launch_bounds__(FM_THREADS) void k_field_mean_blocks(const TF* __restrict__ field, size_t cs, size_t vs, size_t V, int W, int D,
                                                                  int quantize, const unsigned char* __restrict__ mask,
                                                                  const TS* __restrict__ seg, int sz, int sy, int sx, IndexMap g, int kind,
                                                                  double* __restrict__ psum, long long* __restrict__ pcnt, size_t nblocks) {
    __shared__ double sm[3][FM_THREADS];
    __shared__ long long sn[FM_THREADS];
    double a[3] = {0.0, 0.0, 0.0};
    long long n = 0;
    const size_t v0 = (size_t)blockIdx.x * FM_SPAN + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < FM_K; ++k) {
        const size_t v = v0 + (size_t)k * FM_THREADS;
        if (v >= V) break;
        bool in = true;
        if (MODE == FM_MASK) in = mask[v] != 0;
        if (MODE == FM_SEG) in = fm_seg_counts(seg, sz, sy, sx, g, kind, v, W, D);
        if (!in) continue;
        const TF* q = field + v * vs;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            TF x = q[c * cs];
            if constexpr (std::is_same<TF, float>::value) {
                if (quantize) x = __half2float(__float2half_rn(x));
            }
            a[c] += (double)x;
        }
        n += 1;
    }
    fm_tree(a, n, sm, sn);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) psum[c * nblocks + blockIdx.x] = a[c];
        pcnt[blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(FM_THREADS) void k_field_mean_finish(const double* __restrict__ psum, const long long* __restrict__ pcnt,
                                                                  size_t nblocks, double* __restrict__ sums3, long long* __restrict__ count) {
    __shared__ double sm[3][FM_THREADS];
    __shared__ long long sn[FM_THREADS];
    double a[3] = {0.0, 0.0, 0.0};
    long long n = 0;
    for (size_t i = threadIdx.x; i < nblocks; i += FM_THREADS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] += psum[c * nblocks + i];
        n += pcnt[i];
    }
    fm_tree(a, n, sm, sn);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) sums3[c] = a[c];
        *count = n;
    }
}

struct FieldMeanArgs {
    const void* field; size_t cs, vs, V; int W, D, quantize;
    const unsigned char* mask;
    const void* seg; int sz, sy, sx, kind; IndexMap g;
    FieldMeanWs ws; size_t nblocks;
};

template <typename TF, int MODE, typename TS>
static void launch_field_mean(const FieldMeanArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_field_mean_blocks<TF, MODE, TS>), dim3((unsigned)a.nblocks), dim3(FM_THREADS), 0, s, static_cast<const TF*>(a.field), a.cs,
                       a.vs, a.V, a.W, a.D, a.quantize, a.mask, static_cast<const TS*>(a.seg), a.sz, a.sy, a.sx, a.g, a.kind, a.ws.sums,
                       a.ws.counts, a.nblocks);
}
// the field's element comes from with_real; this holds the mode and the segmentation's element
template <typename TF>
static void launch_field_mean_for(const FieldMeanArgs& a, hipStream_t s) {
    if (a.seg) {
        if (a.kind == 1) launch_field_mean<TF, FM_SEG, float>(a, s);
        else launch_field_mean<TF, FM_SEG, double>(a, s);
    } else if (a.mask) {
        launch_field_mean<TF, FM_MASK, double>(a, s);
    } else {
        launch_field_mean<TF, FM_ALL, double>(a, s);
    }
}

}  // namespace cvx

using namespace cvx;

extern "C" size_t cvx_field_mean_workspace_bytes(int H, int W, int D) {
    const size_t V = voxels(H, W, D);
    if (!V) {
        fail(CVX_ERR_INVALID_ARG, "cvx_field_mean_workspace_bytes: bad extent or more than 2^31 - 1 voxels (%dx%dx%d)", H, W, D);
        return 0;
    }
    Carver m;
    field_mean_layout(m, (size_t)cdiv64((int64_t)V, FM_SPAN));
    return ws_query(m);
}

extern "C" int cvx_field_mean_f64(const void* field, int field_is_f64, long long comp_stride, long long voxel_stride, int H, int W, int D,
                                  int quantize, const unsigned char* mask, const void* seg, int seg_kind, int sH, int sW, int sD,
                                  const double* map12, double* sums3, long long* count, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    CVX_REQUIRE(field && sums3 && count, "cvx_field_mean_f64: null pointer (field, sums3 or count)");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_field_mean_f64: bad extent (field %dx%dx%d)", H, W, D);
    const size_t V = voxels(H, W, D);
    CVX_REQUIRE(V, "cvx_field_mean_f64: more than 2^31 - 1 voxels (field %dx%dx%d)", H, W, D);
    CVX_REQUIRE(quantize == 0 || quantize == 1, "cvx_field_mean_f64: quantize must be 0 (as it is) or 1 (float16)");
    CVX_REQUIRE(!(quantize == 1 && field_is_f64), "cvx_field_mean_f64: quantize = 1 needs a float32 field");
    CVX_REQUIRE(!(mask && seg), "cvx_field_mean_f64: both a mask and a segmentation given");
    size_t Vs = 0;
    if (seg) {
        CVX_REQUIRE(map12, "cvx_field_mean_f64: a segmentation needs its index map (map12 is null)");
        CVX_REQUIRE(seg_kind >= 0 && seg_kind <= 2, "cvx_field_mean_f64: seg_kind %d (0 float64, 1 float32, 2 integer as float64)", seg_kind);
        CVX_REQUIRE(sH > 0 && sW > 0 && sD > 0, "cvx_field_mean_f64: bad extent (segmentation %dx%dx%d)", sH, sW, sD);
        Vs = voxels(sH, sW, sD);
        CVX_REQUIRE(Vs, "cvx_field_mean_f64: more than 2^31 - 1 voxels (segmentation %dx%dx%d)", sH, sW, sD);
    }
    CVX_REQUIRE(!map12 || all_finite(map12, 12), "cvx_field_mean_f64: non-finite index map");
    const FieldArg f = {field, field_is_f64, comp_stride, voxel_stride};
    CVX_REQUIRE(f.strides_ok(V), "cvx_field_mean_f64: bad field strides (component %lld, voxel %lld)", comp_stride, voxel_stride);
    const size_t nblocks = (size_t)cdiv64((int64_t)V, FM_SPAN);
    const size_t need = cvx_field_mean_workspace_bytes(H, W, D);
    const Span ins[3] = {f.span(V), {mask, V}, {seg, Vs * (seg_kind == 1 ? 4 : 8)}};
    const Span outs[3] = {{sums3, 3 * sizeof(double)}, {count, sizeof(long long)}, {workspace, need}};
    const Overlaps ov = find_overlaps(outs, ins);
    CVX_REQUIRE(ov.out < 0, "cvx_field_mean_f64: an output overlaps an input");
    CVX_REQUIRE(ov.a < 0, "cvx_field_mean_f64: outputs overlap each other");
    if (!workspace || workspace_bytes < need)
        return fail(CVX_ERR_WORKSPACE, "cvx_field_mean_f64: workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, need);
    FieldMeanArgs a;
    a.field = field; a.cs = (size_t)comp_stride; a.vs = (size_t)voxel_stride; a.V = V; a.W = W; a.D = D; a.quantize = quantize;
    a.mask = mask;
    a.seg = seg; a.sz = sH; a.sy = sW; a.sx = sD; a.kind = seg_kind;
    if (seg) a.g = make_map(map12);
    else a.g = IndexMap{};
    Carver cv(workspace);
    a.ws = field_mean_layout(cv, nblocks);
    a.nblocks = nblocks;
    hipStream_t s = as_stream(stream);
    with_real(field_is_f64, [&](auto tf) { launch_field_mean_for<decltype(tf)>(a, s); });
    const int st = check_last("cvx_field_mean_f64");
    if (st != CVX_OK) return st;
    hipLaunchKernelGGL(k_field_mean_finish, dim3(1), dim3(FM_THREADS), 0, s, a.ws.sums, a.ws.counts, nblocks, sums3, count);
    return check_last("cvx_field_mean_f64 (finish)");
}
