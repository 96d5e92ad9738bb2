// geometry.hip -- the physical-space steps around a registration: what the reference does with SimpleITK's
// resampler before and after convex_adam_pt, as two float64 gathers.
//   k_resample_linear   convex_adam_utils.py:282-306   resample_img / resample_moving_to_fixed: ITK-convention linear resampling of a
//                                                      scalar volume onto another grid (identity transform, default value outside)
//   k_field_to_grid     convex_adam_utils.py:309-351   rescale_displacement_field: the three components resampled onto the moving grid,
//                       apply_convex.py:27-78          rotated by inv(D_fixed) D_moving, scaled by the spacing ratio -- and, in the same
//                                                      pass, apply_convex of the original moving image with that vector
// One output voxel per thread, x fastest; no workspace, no atomics.  The arithmetic (interp_f64.h) is float64 and is the contract: the
// index map is evaluated as ((m0 i + m1 j) + m2 k) + t with plain multiplies and adds, the taps as in k_map_linear_f64 (metrics.hip).
// HBM-bound: 4 or 8 bytes written per resampled voxel, 24 + 4 per carried + warped voxel; the gathers are served by the caches (adjacent
// threads read adjacent or identical taps).  None of this is on the timed path of bench.py.
#include <limits.h>
#include <math.h>

#include "cvx_common.h"
#include "interp_f64.h"
#include "geometry_args.h"

namespace cvx {

// rotation between the two direction-cosine frames and spacing ratio, both in x, y, z order
struct FieldFrame { double r[9], ratio[3]; };

template <typename TS, typename TO>
__global__ __launch_bounds__(256) void k_resample_linear(const TS* __restrict__ src, int sz, int sy, int sx, TO* __restrict__ out, int oz,
                                                         int oy, int ox, IndexMap g, double dflt) {
    const size_t V = (size_t)oz * oy * ox;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= V) return;
    const double i = (double)(int)(p % ox), j = (double)(int)((p / ox) % oy), k = (double)(int)(p / ((size_t)ox * oy));
    const double cx = index_map_axis(g, 0, i, j, k), cy = index_map_axis(g, 1, i, j, k), cz = index_map_axis(g, 2, i, j, k);
    double r = dflt;
    if (itk_inside(cx, sx) && itk_inside(cy, sy) && itk_inside(cz, sz))
        r = taps_linear_f64(src, 1, sz, sy, sx, itk_clamp(cz, sz), itk_clamp(cy, sy), itk_clamp(cx, sx));
    out[p] = (TO)r;                                   // float output: round to nearest, like .astype(np.float32)
}

// field: component c of voxel q at field[c * cs + q * vs] (c = 0, 1, 2: displacement along z, y, x in voxels of the field's grid)
template <typename TF, typename TM, typename TW>
__global__ __launch_bounds__(256) void k_field_to_grid(const TF* __restrict__ field, size_t cs, size_t vs, int fz, int fy, int fx, IndexMap g,
                                                       FieldFrame fr, const TM* __restrict__ moving, int mz, int my, int mx,
                                                       double* __restrict__ carried, TW* __restrict__ warped) {
    const size_t V = (size_t)mz * my * mx;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= V) return;
    const int x = (int)(p % mx), y = (int)((p / mx) % my), z = (int)(p / ((size_t)mx * my));
    const double i = (double)x, j = (double)y, k = (double)z;
    const double cx = index_map_axis(g, 0, i, j, k), cy = index_map_axis(g, 1, i, j, k), cz = index_map_axis(g, 2, i, j, k);
    double vz = 0.0, vy = 0.0, vx = 0.0;
    if (itk_inside(cx, fx) && itk_inside(cy, fy) && itk_inside(cz, fz)) {
        const double qz = itk_clamp(cz, fz), qy = itk_clamp(cy, fy), qx = itk_clamp(cx, fx);
        vz = taps_linear_f64(field, vs, fz, fy, fx, qz, qy, qx);
        vy = taps_linear_f64(field + cs, vs, fz, fy, fx, qz, qy, qx);
        vx = taps_linear_f64(field + 2 * cs, vs, fz, fy, fx, qz, qy, qx);
    }
    // (vx, vy, vz) @ R, then the spacing ratio: moved[..., ::-1] @ rot * ratio of the reference, written out
    double s[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) s[b] = ((vx * fr.r[b] + vy * fr.r[3 + b]) + vz * fr.r[6 + b]) * fr.ratio[b];
    if (carried) {
        carried[3 * p] = s[2];
        carried[3 * p + 1] = s[1];
        carried[3 * p + 2] = s[0];
    }
    if (warped) warped[p] = (TW)map_linear_f64(moving, 1, mz, my, mx, s[2] + k, s[1] + j, s[0] + i);
}

template <typename TS, typename TO>
static void launch_resample(const void* src, int sz, int sy, int sx, void* out, int oz, int oy, int ox, size_t V, const IndexMap& g,
                            double dflt, hipStream_t s) {
    hipLaunchKernelGGL((k_resample_linear<TS, TO>), dim3((unsigned)cdiv64((int64_t)V, 256)), dim3(256), 0, s, static_cast<const TS*>(src), sz,
                       sy, sx, static_cast<TO*>(out), oz, oy, ox, g, dflt);
}

template <typename TF, typename TM, typename TW>
static void launch_field(const void* field, size_t cs, size_t vs, int fz, int fy, int fx, const IndexMap& g, const FieldFrame& fr,
                         const void* moving, int mz, int my, int mx, size_t V, double* carried, void* warped, hipStream_t s) {
    hipLaunchKernelGGL((k_field_to_grid<TF, TM, TW>), dim3((unsigned)cdiv64((int64_t)V, 256)), dim3(256), 0, s, static_cast<const TF*>(field),
                       cs, vs, fz, fy, fx, g, fr, static_cast<const TM*>(moving), mz, my, mx, carried, static_cast<TW*>(warped));
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_resample_linear_f64(const void* src, int src_f64, int sz, int sy, int sx, void* out, int out_f64, int oz, int oy, int ox,
                                       const double* map12_host, double default_value, void* stream) {
    CVX_REQUIRE(src && out && map12_host, "cvx_resample_linear_f64: null pointer");
    const size_t Vs = voxels(sz, sy, sx), Vo = voxels(oz, oy, ox);
    CVX_REQUIRE(sz > 0 && sy > 0 && sx > 0 && oz > 0 && oy > 0 && ox > 0, "cvx_resample_linear_f64: bad extent (source %dx%dx%d, output %dx%dx%d)", sz,
                sy, sx, oz, oy, ox);
    CVX_REQUIRE(Vs && Vo, "cvx_resample_linear_f64: more than 2^31 - 1 voxels (source %dx%dx%d, output %dx%dx%d)", sz, sy, sx, oz, oy, ox);
    CVX_REQUIRE(!ranges_overlap(src, Vs * (src_f64 ? 8 : 4), out, Vo * (out_f64 ? 8 : 4)), "cvx_resample_linear_f64: out overlaps src");
    CVX_REQUIRE(all_finite(map12_host, 12) && isfinite(default_value), "cvx_resample_linear_f64: non-finite index map or default value");
    const IndexMap g = make_map(map12_host);
    hipStream_t s = as_stream(stream);
    with_real(src_f64, [&](auto ts) {
        with_real(out_f64, [&](auto to) {
            launch_resample<decltype(ts), decltype(to)>(src, sz, sy, sx, out, oz, oy, ox, Vo, g, default_value, s);
        });
    });
    return check_last("resample_linear");
}

extern "C" int cvx_field_to_grid_f64(const void* field, int field_f64, int64_t comp_stride, int64_t voxel_stride, int fz, int fy, int fx,
                                     const double* map12_host, const double* rot9_host, const double* ratio3_host, const void* moving,
                                     int moving_f64, int mz, int my, int mx, double* carried, void* warped, int warped_f64, void* stream) {
    CVX_REQUIRE(field && map12_host && rot9_host && ratio3_host, "cvx_field_to_grid_f64: null pointer");
    CVX_REQUIRE(carried || warped, "cvx_field_to_grid_f64: no output requested");
    CVX_REQUIRE(!warped || moving, "cvx_field_to_grid_f64: a warped output needs the moving volume");
    const size_t Vf = voxels(fz, fy, fx), Vm = voxels(mz, my, mx);
    CVX_REQUIRE(fz > 0 && fy > 0 && fx > 0 && mz > 0 && my > 0 && mx > 0, "cvx_field_to_grid_f64: bad extent (field %dx%dx%d, moving %dx%dx%d)", fz, fy,
                fx, mz, my, mx);
    CVX_REQUIRE(Vf && Vm, "cvx_field_to_grid_f64: more than 2^31 - 1 voxels (field %dx%dx%d, moving %dx%dx%d)", fz, fy, fx, mz, my, mx);
    const FieldArg f = {field, field_f64, comp_stride, voxel_stride};
    CVX_REQUIRE(f.strides_ok(Vf), "cvx_field_to_grid_f64: bad field strides (component %lld, voxel %lld)", (long long)comp_stride,
                (long long)voxel_stride);
    const Span ins[2] = {f.span(Vf), {moving, Vm * (moving_f64 ? 8 : 4)}};
    const Span outs[2] = {{carried, Vm * 3 * sizeof(double)}, {warped, Vm * (warped_f64 ? 8 : 4)}};
    const Overlaps ov = find_overlaps(outs, ins);
    CVX_REQUIRE(ov.out != 0, "cvx_field_to_grid_f64: carried overlaps an input");
    CVX_REQUIRE(ov.out != 1, "cvx_field_to_grid_f64: warped overlaps an input");
    CVX_REQUIRE(ov.a < 0, "cvx_field_to_grid_f64: the two outputs overlap");
    CVX_REQUIRE(all_finite(map12_host, 12) && all_finite(rot9_host, 9) && all_finite(ratio3_host, 3),
                "cvx_field_to_grid_f64: non-finite index map, rotation or spacing ratio");
    const IndexMap g = make_map(map12_host);
    FieldFrame fr;
    for (int i = 0; i < 9; ++i) fr.r[i] = rot9_host[i];
    for (int i = 0; i < 3; ++i) fr.ratio[i] = ratio3_host[i];
    hipStream_t s = as_stream(stream);
    const size_t cs = (size_t)comp_stride, vs = (size_t)voxel_stride;
    with_real(field_f64, [&](auto tf) {
        with_real(moving_f64, [&](auto tm) {
            with_real(warped_f64, [&](auto tw) {
                launch_field<decltype(tf), decltype(tm), decltype(tw)>(field, cs, vs, fz, fy, fx, g, fr, moving, mz, my, mx, Vm, carried, warped, s);
            });
        });
    });
    return check_last("field_to_grid");
}
