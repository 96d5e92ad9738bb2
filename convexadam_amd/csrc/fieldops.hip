// fieldops.hip -- the inverse of a displacement field and the composition of two (include/convexadam_field.h).
//   k_field_invert    v(y) = -u(y + v(y)) by v_{k+1}(y) = -u(y + v_k(y)): the update of a voxel reads u and its OWN v_k only, so all
//                     iterations of a voxel run in registers inside one launch -- u is read, v is written once, where K launches of one
//                     iteration each would read and write a volume-sized v K times
//   k_field_compose   out(x) = b(x) + a(clamp(x + b(x)))
// One thread per voxel; the per-voxel arithmetic is fieldops_core.h (float64, the contract).  u is gathered through L1 / L2: neighbouring
// voxels read neighbouring or identical taps, no LDS staging.  Lanes leave the iteration loop at different counts; its body holds no
// wave-wide operation, so that is plain divergence.  The statistics are reduced over the wavefront AFTER the loop and leave as integer
// atomics (add, and max on the bits of a non-negative double): the same on every run.
// Workgroup footprint: 256 threads as a brick of 4 x 4 x 16 voxels (FB0 x FB1 x FB2).  Measured against 4 rows of 64 along D on the
// benchmark pair's field, 20 iterations: 2.10 against 2.55 ms, rounds within 0.05 ms of each other, so the row form is
// gone; the likely reason, not confirmed by counters, is that a brick's taps fall into fewer cache lines than those of four long rows.
// The tiles of a grid are walked by a grid-stride loop (a wave-uniform trip count), so that no extent needs more than 2^23 workgroups.
// None of this is on the timed path of bench.py.
#include <limits.h>
#include <math.h>

#include "cvx_common.h"
#include "interp_f64.h"
#include "geometry_args.h"
#include "fieldops_core.h"
#include "convexadam_field.h"

namespace cvx {

constexpr int FB0 = 4, FB1 = 4, FB2 = 16;

struct FieldTiles { int n1, n2; long long count; };

template <int B0, int B1, int B2>
static FieldTiles field_tiles(int H, int W, int D) {
    FieldTiles t;
    t.n1 = cdiv(W, B1);
    t.n2 = cdiv(D, B2);
    t.count = (long long)cdiv(H, B0) * t.n1 * t.n2;
    return t;
}

// voxel of this thread in tile `tile`; false when it lies outside the grid
template <int B0, int B1, int B2>
__device__ __forceinline__ bool field_voxel(long long tile, const FieldTiles& ft, int H, int W, int D, int& i0, int& i1, int& i2) {
    static_assert(B0 * B1 * B2 == 256, "one workgroup of 256 threads");
    const int t = (int)threadIdx.x;
    const int t2 = (int)(tile % ft.n2), t1 = (int)((tile / ft.n2) % ft.n1);
    const long long t0 = tile / ((long long)ft.n2 * ft.n1);
    i2 = t2 * B2 + t % B2;
    i1 = t1 * B1 + (t / B2) % B1;
    i0 = (int)(t0 * B0) + t / (B2 * B1);
    return i0 < H && i1 < W && i2 < D;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(x, o, 64);
        x = y > x ? y : x;
    }
    return x;
}

template <typename TU, typename TV, int B0, int B1, int B2>
__global__ __launch_bounds__(256) void k_field_invert(const TU* __restrict__ u, size_t ucs, size_t uvs, int H, int W, int D, int max_iters,
                                                      double tol, TV* __restrict__ v_out, size_t vcs, size_t vvs,
                                                      double* __restrict__ residual, unsigned char* __restrict__ iters,
                                                      unsigned long long* __restrict__ stats, FieldTiles ft) {
    unsigned long long not_converged = 0, non_finite = 0, rmax = 0;
    for (long long tile = blockIdx.x; tile < ft.count; tile += gridDim.x) {
        int i0, i1, i2;
        if (!field_voxel<B0, B1, B2>(tile, ft, H, W, D, i0, i1, i2)) continue;
        double v[3], r;
        int it;
        const int flag = field_invert_voxel(u, ucs, uvs, H, W, D, i0, i1, i2, max_iters, tol, v, r, it);
        const size_t q = ((size_t)i0 * W + i1) * D + i2;
#pragma unroll
        for (int a = 0; a < 3; ++a) v_out[a * vcs + q * vvs] = (TV)v[a];           // float: round to nearest
        if (residual) residual[q] = r;
        if (iters) iters[q] = (unsigned char)it;
        not_converged += flag == FIELD_NOT_CONVERGED;
        non_finite += flag == FIELD_NON_FINITE;
        if (flag != FIELD_NON_FINITE) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(r);      // r >= 0 and finite: the bits order like the values
            rmax = bits > rmax ? bits : rmax;
        }
    }
    if (!stats) return;
    // every lane of the wavefront arrives here: the loop's trip count is the same for the whole workgroup
    not_converged = wave_sum(not_converged);
    non_finite = wave_sum(non_finite);
    rmax = wave_max(rmax);
    if ((threadIdx.x & 63) == 0) {
        if (not_converged) atomicAdd(stats, not_converged);
        if (non_finite) atomicAdd(stats + 1, non_finite);
        if (rmax) atomicMax(stats + 2, rmax);
    }
}

template <typename TA, typename TB, typename TO, int B0, int B1, int B2>
__global__ __launch_bounds__(256) void k_field_compose(const TA* __restrict__ fa, size_t acs, size_t avs, const TB* __restrict__ fb, size_t bcs,
                                                       size_t bvs, int H, int W, int D, TO* __restrict__ out, size_t ocs, size_t ovs,
                                                       FieldTiles ft) {
    for (long long tile = blockIdx.x; tile < ft.count; tile += gridDim.x) {
        int i0, i1, i2;
        if (!field_voxel<B0, B1, B2>(tile, ft, H, W, D, i0, i1, i2)) continue;
        double o[3];
        field_compose_voxel(fa, acs, avs, fb, bcs, bvs, H, W, D, i0, i1, i2, o);
        const size_t q = ((size_t)i0 * W + i1) * D + i2;
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a * ocs + q * ovs] = (TO)o[a];
    }
}

static unsigned field_blocks(const FieldTiles& ft) { return (unsigned)(ft.count < (1ll << 23) ? ft.count : (1ll << 23)); }

struct InvertArgs {
    const void* u; size_t ucs, uvs; int H, W, D, max_iters; double tol; void* v; size_t vcs, vvs; double* residual; unsigned char* iters;
    unsigned long long* stats;
};

template <typename TU, typename TV, int B0, int B1, int B2>
static void launch_invert(const InvertArgs& a, hipStream_t s) {
    const FieldTiles ft = field_tiles<B0, B1, B2>(a.H, a.W, a.D);
    hipLaunchKernelGGL((k_field_invert<TU, TV, B0, B1, B2>), dim3(field_blocks(ft)), dim3(256), 0, s, static_cast<const TU*>(a.u), a.ucs, a.uvs,
                       a.H, a.W, a.D, a.max_iters, a.tol, static_cast<TV*>(a.v), a.vcs, a.vvs, a.residual, a.iters, a.stats, ft);
}

struct ComposeArgs { const void *a, *b; size_t acs, avs, bcs, bvs; int H, W, D; void* out; size_t ocs, ovs; };

template <typename TA, typename TB, typename TO>
static void launch_compose(const ComposeArgs& c, hipStream_t s) {
    const FieldTiles ft = field_tiles<FB0, FB1, FB2>(c.H, c.W, c.D);
    hipLaunchKernelGGL((k_field_compose<TA, TB, TO, FB0, FB1, FB2>), dim3(field_blocks(ft)), dim3(256), 0, s, static_cast<const TA*>(c.a), c.acs, c.avs,
                       static_cast<const TB*>(c.b), c.bcs, c.bvs, c.H, c.W, c.D, static_cast<TO*>(c.out), c.ocs, c.ovs, ft);
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_field_invert_f64(const void* u, int u_f64, int64_t u_comp_stride, int64_t u_voxel_stride, int H, int W, int D, int max_iters,
                                    double tol, void* v_out, int v_f64, int64_t v_comp_stride, int64_t v_voxel_stride, double* residual,
                                    unsigned char* iters, long long* stats, void* stream) {
    CVX_REQUIRE(u && v_out, "cvx_field_invert_f64: null pointer");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_field_invert_f64: bad extent (%dx%dx%d)", H, W, D);
    const size_t V = voxels(H, W, D);
    CVX_REQUIRE(V, "cvx_field_invert_f64: more than 2^31 - 1 voxels (%dx%dx%d)", H, W, D);
    const FieldArg fu = {u, u_f64, u_comp_stride, u_voxel_stride}, fv = {v_out, v_f64, v_comp_stride, v_voxel_stride};
    CVX_REQUIRE(fu.strides_ok(V), "cvx_field_invert_f64: bad field strides of u (component %lld, voxel %lld)", (long long)u_comp_stride,
                (long long)u_voxel_stride);
    CVX_REQUIRE(fv.strides_ok(V), "cvx_field_invert_f64: bad field strides of v_out (component %lld, voxel %lld)", (long long)v_comp_stride,
                (long long)v_voxel_stride);
    CVX_REQUIRE(max_iters >= 1 && max_iters <= 1000, "cvx_field_invert_f64: max_iters %d outside 1 .. 1000", max_iters);
    CVX_REQUIRE(isfinite(tol) && tol >= 0.0, "cvx_field_invert_f64: tol must be finite and not negative");
    CVX_REQUIRE(fu.aligned() && fv.aligned() && field_aligned(residual, 1) && field_aligned(stats, 1),
                "cvx_field_invert_f64: a buffer is not aligned to its element");
    const Span ins[1] = {fu.span(V)}, outs[4] = {fv.span(V), {residual, V * sizeof(double)}, {iters, V}, {stats, 3 * sizeof(long long)}};
    const Overlaps ov = find_overlaps(outs, ins);
    CVX_REQUIRE(ov.out < 0, "cvx_field_invert_f64: an output overlaps u");
    CVX_REQUIRE(ov.a < 0, "cvx_field_invert_f64: two outputs overlap");
    hipStream_t s = as_stream(stream);
    if (stats && hipMemsetAsync(stats, 0, 3 * sizeof(long long), s) != hipSuccess) return fail(CVX_ERR_LAUNCH, "cvx_field_invert_f64: memset failed");
    const InvertArgs a = {u, (size_t)u_comp_stride, (size_t)u_voxel_stride, H, W, D, max_iters, tol, v_out, (size_t)v_comp_stride,
                          (size_t)v_voxel_stride, residual, iters, reinterpret_cast<unsigned long long*>(stats)};
    with_real(u_f64, [&](auto tu) {
        with_real(v_f64, [&](auto tv) { launch_invert<decltype(tu), decltype(tv), FB0, FB1, FB2>(a, s); });
    });
    return check_last("field_invert");
}

extern "C" int cvx_field_compose_f64(const void* a, int a_f64, int64_t a_comp_stride, int64_t a_voxel_stride, const void* b, int b_f64,
                                     int64_t b_comp_stride, int64_t b_voxel_stride, int H, int W, int D, void* out, int out_f64,
                                     int64_t out_comp_stride, int64_t out_voxel_stride, void* stream) {
    CVX_REQUIRE(a && b && out, "cvx_field_compose_f64: null pointer");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_field_compose_f64: bad extent (%dx%dx%d)", H, W, D);
    const size_t V = voxels(H, W, D);
    CVX_REQUIRE(V, "cvx_field_compose_f64: more than 2^31 - 1 voxels (%dx%dx%d)", H, W, D);
    const FieldArg fa = {a, a_f64, a_comp_stride, a_voxel_stride}, fb = {b, b_f64, b_comp_stride, b_voxel_stride},
                   fo = {out, out_f64, out_comp_stride, out_voxel_stride};
    CVX_REQUIRE(fa.strides_ok(V), "cvx_field_compose_f64: bad field strides of a (component %lld, voxel %lld)", (long long)a_comp_stride,
                (long long)a_voxel_stride);
    CVX_REQUIRE(fb.strides_ok(V), "cvx_field_compose_f64: bad field strides of b (component %lld, voxel %lld)", (long long)b_comp_stride,
                (long long)b_voxel_stride);
    CVX_REQUIRE(fo.strides_ok(V), "cvx_field_compose_f64: bad field strides of out (component %lld, voxel %lld)", (long long)out_comp_stride,
                (long long)out_voxel_stride);
    CVX_REQUIRE(fa.aligned() && fb.aligned() && fo.aligned(), "cvx_field_compose_f64: a buffer is not aligned to its element");
    CVX_REQUIRE(!ranges_overlap(out, fo.bytes(V), a, fa.bytes(V)) && !ranges_overlap(out, fo.bytes(V), b, fb.bytes(V)),
                "cvx_field_compose_f64: out overlaps an input");
    const ComposeArgs c = {a, b, (size_t)a_comp_stride, (size_t)a_voxel_stride, (size_t)b_comp_stride, (size_t)b_voxel_stride, H, W, D, out,
                           (size_t)out_comp_stride, (size_t)out_voxel_stride};
    hipStream_t s = as_stream(stream);
    with_real(a_f64, [&](auto ta) {
        with_real(b_f64, [&](auto tb) {
            with_real(out_f64, [&](auto to) { launch_compose<decltype(ta), decltype(tb), decltype(to)>(c, s); });
        });
    });
    return check_last("field_compose");
}
