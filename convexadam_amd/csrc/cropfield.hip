// cropfield.hip -- a field on the crop + resize grid of a registration carried to the original fixed image at half resolution:
// what the abdomen MR-CT script does between its thin-plate spline and the file it submits.
//   k_crop_field_half   l2r_2021_convexAdam_task1_docker.py:390-397   voxel field -> displacement in millimetres (at the taps, on the fly)
//                       :38-105  convert_crop_field                   inverse fixed crop affine, border-clamped trilinear sample of disp_p,
//                                                                     spacings, moving crop affine, d = m - x, axis flips with sign change,
//                                                                     F.interpolate(scale_factor=0.5, trilinear), cast to float16
//                       task2:308-315, task3:213-217                  the same halving alone (identity mode)
// One thread per four consecutive half-resolution outputs along the last axis: it evaluates the chain at their 2 x 2 x 8 source voxels of the
// original grid -- each one a float64 gather of 8 taps x 3 components from the small registration-grid field, which the caches serve --
// averages them in float in ATen's order and stores 3 x 8 bytes (float16) or 3 x 16 (float32).  Nothing of the size of the original volume
// is read or written; no workspace, no atomics.  The arithmetic is the contract stated at cvx_crop_field_half_f32 (include/convexadam_hip.h):
// float64 per source voxel in a fixed order, rounded to float once, then ATen's float32 halving; tests/cropfield_restatement.py restates it.
#include <limits.h>
#include <math.h>

#include "cvx_common.h"
#include "interp_f64.h"
#include "geometry_args.h"

namespace cvx {

// the eight per-axis constants of the chain, in the order of geom27_host
struct CropGeom { double fs[3], lo[3], nfsp[3], nmsp[3], ms[3], mlo[3], pfs[3], pms[3]; };

enum { CROP_PHYSICAL = 0, CROP_VOXELS = 1, CROP_IDENTITY = 2 };

// one axis of one source voxel: the index on the registration grid and its two clamped taps
struct AxisTap { double x, g, w[2]; int i[2]; };

// source index of tap b (0, 1) of output o along an axis of extent S: 2 o + b clamped, on the flipped grid when `flip`
__device__ __forceinline__ int half_source(int o, int b, int S, bool flip) {
    const int p = 2 * o + b < S - 1 ? 2 * o + b : S - 1;
    return flip ? S - 1 - p : p;
}

__device__ __forceinline__ AxisTap axis_tap(const CropGeom& G, int a, int xs, int n) {
    AxisTap t;
    t.x = (double)xs;
    t.g = G.fs[a] * (t.x - G.lo[a]);
    double c = t.g > 0.0 ? t.g : 0.0;                          // a NaN fails the comparison and becomes 0: never an index
    const double hi = (double)(n - 1);
    c = c > hi ? hi : c;
    const double f = floor(c), r = c - f;
    t.i[0] = (int)f;
    t.i[1] = t.i[0] + 1 < n ? t.i[0] + 1 : n - 1;
    t.w[0] = 1.0 - r;
    t.w[1] = 1.0 - (1.0 - r);
    return t;
}

// d = m - x of one voxel of the original fixed grid, flipped sign included, rounded to float
template <bool VOX>
__device__ __forceinline__ void chain_voxel(const float* __restrict__ field, size_t cs, size_t vs, int W, int D, const CropGeom& G,
                                            const AxisTap& t0, const AxisTap& t1, const AxisTap& t2, int flip, float (&d)[3]) {
    double p[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int y[3] = {t0.i[i], t1.i[j], t2.i[k]};
                const size_t q = (((size_t)y[0] * W + y[1]) * D + y[2]) * vs;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float u = field[a * cs + q];
                    if (VOX) u = ((float)y[a] + u) * (float)G.pms[a] - (float)y[a] * (float)G.pfs[a];      // the reference's float32 disp_p, its order
                    p[a] += (((double)u * t0.w[i]) * t1.w[j]) * t2.w[k];
                }
            }
    const double g[3] = {t0.g, t1.g, t2.g}, x[3] = {t0.x, t1.x, t2.x};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double m = ((g[a] * G.nfsp[a] + p[a]) / G.nmsp[a]) / G.ms[a] + G.mlo[a];
        const double r = m - x[a];
        d[a] = (float)((flip >> a) & 1 ? -r : r);
    }
}

template <typename TO> struct CropStore;
template <> struct CropStore<float> {
    static __device__ __forceinline__ void put(float* p, const float (&v)[4], int n) {
        const uintptr_t addr = (uintptr_t)p;
        if (n == 4 && (addr & 15) == 0) {
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else if (n == 4 && (addr & 7) == 0) {
            *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
            *reinterpret_cast<float2*>(p + 2) = make_float2(v[2], v[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) p[i] = v[i];
        }
    }
};
template <> struct CropStore<_Float16> {
    typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
    typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ void put(_Float16* p, const float (&v)[4], int n) {
        const _Float16 h[4] = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};          // round to nearest even, inf beyond 65504
        const uintptr_t addr = (uintptr_t)p;
        if (n == 4 && (addr & 7) == 0) {
            const h16x4 o = {h[0], h[1], h[2], h[3]};
            *reinterpret_cast<h16x4*>(p) = o;
        } else if (n == 4 && (addr & 3) == 0) {
            const h16x2 a = {h[0], h[1]}, b = {h[2], h[3]};
            *reinterpret_cast<h16x2*>(p) = a;
            *reinterpret_cast<h16x2*>(p + 2) = b;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) p[i] = h[i];
        }
    }
};

// field [H][W][D] through (cs, vs); out [3][O0][O1][O2] with O = S / 2; thread = (o0, o1, group of four o2)
template <int MODE, typename TO>
__global__ __launch_bounds__(256) void k_crop_field_half(const float* __restrict__ field, size_t cs, size_t vs, int H, int W, int D, CropGeom G,
                                                         int S0, int S1, int S2, int flip, TO* __restrict__ out) {
    const int O0 = S0 / 2, O1 = S1 / 2, O2 = S2 / 2, G2 = (O2 + 3) / 4;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (size_t)O0 * O1 * G2) return;
    const int j4 = (int)(tid % G2) * 4, o1 = (int)((tid / G2) % O1), o0 = (int)(tid / ((size_t)G2 * O1));
    const int x0[2] = {half_source(o0, 0, S0, flip & 1), half_source(o0, 1, S0, flip & 1)};
    const int x1[2] = {half_source(o1, 0, S1, flip & 2), half_source(o1, 1, S1, flip & 2)};
    AxisTap t0[2], t1[2];
    if (MODE != CROP_IDENTITY) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            t0[b] = axis_tap(G, 0, x0[b], H);
            t1[b] = axis_tap(G, 1, x1[b], W);
        }
    }
    // the chain's loops over the outputs and their tap pairs stay rolled (registers: 24 float64 gathers per source voxel); identity mode has
    // six loads per tap pair and unrolls everything, so that all 96 are in flight at once
    constexpr int UNROLL_K = MODE == CROP_IDENTITY ? 4 : 1;
    float res[3][4] = {};
#pragma unroll UNROLL_K
    for (int k = 0; k < 4; ++k) {
        const int o2 = j4 + k < O2 ? j4 + k : O2 - 1;          // a group's overhang recomputes the row's last output; it is not stored
        const int x2[2] = {half_source(o2, 0, S2, flip & 4), half_source(o2, 1, S2, flip & 4)};
        AxisTap t2[2];
        if (MODE != CROP_IDENTITY) {
#pragma unroll
            for (int b = 0; b < 2; ++b) t2[b] = axis_tap(G, 2, x2[b], D);
        }
        // the four (axis 0, axis 1) tap pairs: their taps by selection, the two outer averaging steps as running sums --
        // s = r_0 * 0.5 + r_1 * 0.5, value = s_0 * 0.5 + s_1 * 0.5, the same operations in the same order
        float s[3] = {0.0f, 0.0f, 0.0f}, val[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll UNROLL_K
        for (int bb = 0; bb < 4; ++bb) {
            const bool b0 = bb >> 1, b1 = bb & 1;
            const int xs0 = b0 ? x0[1] : x0[0], xs1 = b1 ? x1[1] : x1[0];
            const AxisTap ta = b0 ? t0[1] : t0[0], tb = b1 ? t1[1] : t1[0];
            float d[2][3];
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2) {
                if (MODE == CROP_IDENTITY) {
                    const size_t q = (((size_t)xs0 * S1 + xs1) * S2 + x2[b2]) * vs;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const float v = field[a * cs + q];
                        d[b2][a] = (flip >> a) & 1 ? -v : v;
                    }
                } else {
                    chain_voxel<MODE == CROP_VOXELS>(field, cs, vs, W, D, G, ta, tb, t2[b2], flip, d[b2]);
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float r = d[0][a] * 0.5f + d[1][a] * 0.5f;
                s[a] = b1 ? s[a] + r * 0.5f : r * 0.5f;
                if (b1) val[a] = b0 ? val[a] + s[a] * 0.5f : s[a] * 0.5f;
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            res[a][0] = res[a][1];                              // a register shift instead of an indexed write: the loop may be rolled
            res[a][1] = res[a][2];
            res[a][2] = res[a][3];
            res[a][3] = val[a];
        }
    }
    const size_t Vo = (size_t)O0 * O1 * O2, at = ((size_t)o0 * O1 + o1) * O2 + j4;
    const int n = O2 - j4 < 4 ? O2 - j4 : 4;
#pragma unroll
    for (int a = 0; a < 3; ++a) CropStore<TO>::put(out + a * Vo + at, res[a], n);
}

template <int MODE, typename TO>
static void launch_crop(const float* field, size_t cs, size_t vs, int H, int W, int D, const CropGeom& G, int S0, int S1, int S2, int flip,
                        void* out, hipStream_t s) {
    const int64_t threads = (int64_t)(S0 / 2) * (S1 / 2) * ((S2 / 2 + 3) / 4);
    hipLaunchKernelGGL((k_crop_field_half<MODE, TO>), dim3((unsigned)cdiv64(threads, 256)), dim3(256), 0, s, field, cs, vs, H, W, D, G, S0, S1, S2,
                       flip, static_cast<TO*>(out));
}
template <int MODE>
static void launch_crop_for(const float* field, size_t cs, size_t vs, int H, int W, int D, const CropGeom& G, int S0, int S1, int S2, int flip,
                            void* out, bool out_f32, hipStream_t s) {
    if (out_f32) launch_crop<MODE, float>(field, cs, vs, H, W, D, G, S0, S1, S2, flip, out, s);
    else launch_crop<MODE, _Float16>(field, cs, vs, H, W, D, G, S0, S1, S2, flip, out, s);
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_crop_field_half_f32(const float* field, int64_t comp_stride, int64_t voxel_stride, int H, int W, int D,
                                       const double* geom27_host, int S0, int S1, int S2, int flip_mask, int flags, void* out, void* stream) {
    CVX_REQUIRE(field && out, "cvx_crop_field_half_f32: null pointer");
    CVX_REQUIRE((flags & ~(CVX_CROP_FIELD_VOXELS | CVX_CROP_OUT_F32 | CVX_CROP_IDENTITY)) == 0, "cvx_crop_field_half_f32: unknown flag in %d", flags);
    CVX_REQUIRE(flip_mask >= 0 && flip_mask <= 7, "cvx_crop_field_half_f32: unknown flip mask %d (bits 0..2 = axes 0..2)", flip_mask);
    const bool identity = (flags & CVX_CROP_IDENTITY) != 0, voxels_in = (flags & CVX_CROP_FIELD_VOXELS) != 0, out_f32 = (flags & CVX_CROP_OUT_F32) != 0;
    CVX_REQUIRE(!(identity && voxels_in), "cvx_crop_field_half_f32: unknown flag combination (identity with a voxel field)");
    CVX_REQUIRE(identity || geom27_host, "cvx_crop_field_half_f32: null pointer (geometry, without CVX_CROP_IDENTITY)");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0 && S0 > 0 && S1 > 0 && S2 > 0, "cvx_crop_field_half_f32: bad extent (field %dx%dx%d, original %dx%dx%d)", H, W,
                D, S0, S1, S2);
    CVX_REQUIRE(S0 > 1 && S1 > 1 && S2 > 1, "cvx_crop_field_half_f32: bad extent (original %dx%dx%d: an axis of 1 has no half-resolution output)", S0,
                S1, S2);
    const size_t Vf = voxels(H, W, D), Vs = voxels(S0, S1, S2);
    CVX_REQUIRE(Vf && Vs, "cvx_crop_field_half_f32: more than 2^31 - 1 voxels (field %dx%dx%d, original %dx%dx%d)", H, W, D, S0, S1, S2);
    const FieldArg f = {field, 0, comp_stride, voxel_stride};
    CVX_REQUIRE(f.strides_ok(Vf), "cvx_crop_field_half_f32: bad field strides (component %lld, voxel %lld)", (long long)comp_stride,
                (long long)voxel_stride);
    const size_t esize = out_f32 ? 4 : 2;
    CVX_REQUIRE(((uintptr_t)out & (esize - 1)) == 0 && f.aligned(), "cvx_crop_field_half_f32: a buffer is not aligned to its element");
    const size_t Vo = (size_t)(S0 / 2) * (S1 / 2) * (S2 / 2);
    CVX_REQUIRE(!ranges_overlap(out, 3 * Vo * esize, field, f.bytes(Vf)), "cvx_crop_field_half_f32: out overlaps the field");
    CropGeom G = {};
    if (identity) {
        CVX_REQUIRE(H == S0 && W == S1 && D == S2, "cvx_crop_field_half_f32: shape mismatch (identity mode: field %dx%dx%d, original %dx%dx%d)", H, W,
                    D, S0, S1, S2);
    } else {
        CVX_REQUIRE(all_finite(geom27_host, 27), "cvx_crop_field_half_f32: non-finite scale, spacing or crop");
        const double* g = geom27_host;
        const int n[3] = {H, W, D};
        for (int a = 0; a < 3; ++a) {
            G.fs[a] = g[a]; G.lo[a] = g[3 + a]; G.nfsp[a] = g[6 + a]; G.nmsp[a] = g[9 + a];
            G.ms[a] = g[12 + a]; G.mlo[a] = g[15 + a]; G.pfs[a] = g[18 + a]; G.pms[a] = g[21 + a];
            CVX_REQUIRE(G.fs[a] != 0.0 && G.nfsp[a] != 0.0 && G.nmsp[a] != 0.0 && G.ms[a] != 0.0 && G.pfs[a] != 0.0 && G.pms[a] != 0.0,
                        "cvx_crop_field_half_f32: zero scale or spacing on axis %d", a);
            const double want = rint(G.fs[a] * (g[24 + a] - G.lo[a]));
            CVX_REQUIRE(want == (double)n[a], "cvx_crop_field_half_f32: shape mismatch (axis %d: the case's crop resizes to %.17g voxels, the field has %d)",
                        a, want, n[a]);
        }
    }
    hipStream_t s = as_stream(stream);
    const size_t cs = (size_t)comp_stride, vs = (size_t)voxel_stride;
    if (identity) launch_crop_for<CROP_IDENTITY>(field, cs, vs, H, W, D, G, S0, S1, S2, flip_mask, out, out_f32, s);
    else if (voxels_in) launch_crop_for<CROP_VOXELS>(field, cs, vs, H, W, D, G, S0, S1, S2, flip_mask, out, out_f32, s);
    else launch_crop_for<CROP_PHYSICAL>(field, cs, vs, H, W, D, G, S0, S1, S2, flip_mask, out, out_f32, s);
    return check_last("crop_field_half");
}
