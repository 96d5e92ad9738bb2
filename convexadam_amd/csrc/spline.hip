// spline.hip -- cubic B-spline interpolation in float64: scipy.ndimage's order=3 with its defaults (include/convexadam_spline.h).
// The arithmetic of a line and of a sample is csrc/spline_core.h; this file only decides who takes which line or voxel.  No workspace, no
// atomics, and no thread's result depends on another's: the same bytes on every run.
//   k_spline_strided   the prefilter along axis 0 or axis 1: one thread per line, neighbouring threads on neighbouring x, so that every
//                      step of the recursion is one coalesced access of the wavefront.  The axis-0 pass reads the source (float or
//                      double) and writes the coefficients; it runs for every volume, also where H = 1 (the line function then copies).
//   k_spline_contig    the prefilter along axis 2, in place.  A line is contiguous there: a thread walking its own line would touch 64
//                      different 64-byte segments per wave-instruction.  A workgroup of one wavefront takes SPL_LINES = 64 lines and
//                      stages them through LDS in chunks of SPL_CHUNK = 32 samples: rows of 256 contiguous bytes between global memory
//                      and LDS, and in LDS thread t walks row t of pitch 33 doubles (66 dwords: the 32 lanes of a ds_read_b64 group fall
//                      on banks 2 t, 2 t + 1 -- no conflict).  A line of any length is walked chunk by chunk with the recursion state in
//                      registers: the start sum (one pass over the whole line, the chunk and its mirror image staged side by side), the
//                      forward pass (chunks ascending, written back), the backward pass (chunks descending).  The steps are the
//                      functions of spline_core.h that spline_prefilter_line is written with: the two cannot differ in a bit.
//   k_map_cubic_f64    out(q) = spline at q + u(q), the field read in place through (pointer, is_f64, comp_stride, voxel_stride)
//   k_resample_cubic_f64   out(q) = spline at the index map of q, ITK's buffer rule, a default value outside
//                      One thread per output voxel, x fastest; 64 float64 taps per voxel, served by the caches (adjacent threads read
//                      adjacent or identical taps).
// Offsets are 64-bit throughout; a volume has at most 2^31 - 1 voxels.  None of this is on the timed path of bench.py.
#include <limits.h>
#include <math.h>

#include "cvx_common.h"
#include "geometry_args.h"
#include "convexadam_spline.h"
#include "spline_core.h"

namespace cvx {

constexpr int SPL_THREADS = 256;                    // the strided passes and the gathers
constexpr int SPL_LINES = 64;                       // lines (= threads: one wavefront) per workgroup of the contiguous pass
constexpr int SPL_CHUNK = 32;                       // samples of a line staged at once
constexpr int SPL_PITCH = SPL_CHUNK + 1;            // doubles per staged row

// line p of `lines`: its first sample at (p / inner) * outer_stride + p % inner, sample i a further i * stride on.  src may be coef.
template <typename TS>
__global__ __launch_bounds__(SPL_THREADS) void k_spline_strided(const TS* src, double* coef, int n, size_t stride, size_t inner, size_t outer_stride,
                                                                size_t lines) {
    const size_t p = (size_t)blockIdx.x * SPL_THREADS + threadIdx.x;
    if (p >= lines) return;
    const size_t base = (p / inner) * outer_stride + p % inner;
    spline_prefilter_line(src + base, coef + base, stride, n);
}

// rows r < nl of the workgroup's lines, samples x0 .. x0 + len - 1, between global memory (g: the first line's first sample) and a staged tile
__device__ __forceinline__ void spl_stage_in(double* tile, const double* g, int n, int nl, int x0, int len, int t) {
#pragma unroll 4
    for (int e = t; e < SPL_LINES * SPL_CHUNK; e += SPL_LINES) {
        const int r = e / SPL_CHUNK, c = e % SPL_CHUNK;
        if (r < nl && c < len) tile[r * SPL_PITCH + c] = g[(size_t)r * n + (size_t)(x0 + c)];
    }
}
__device__ __forceinline__ void spl_stage_out(const double* tile, double* g, int n, int nl, int x0, int len, int t) {
#pragma unroll 4
    for (int e = t; e < SPL_LINES * SPL_CHUNK; e += SPL_LINES) {
        const int r = e / SPL_CHUNK, c = e % SPL_CHUNK;
        if (r < nl && c < len) g[(size_t)r * n + (size_t)(x0 + c)] = tile[r * SPL_PITCH + c];
    }
}

// n >= 2 (the launcher skips an axis of length 1).  Every trip count and every barrier below is uniform over the workgroup.
__global__ __launch_bounds__(SPL_LINES) void k_spline_contig(double* coef, int n, size_t lines) {
    __shared__ double tile_a[SPL_LINES * SPL_PITCH], tile_b[SPL_LINES * SPL_PITCH];
    const int t = threadIdx.x;
    const size_t line0 = (size_t)blockIdx.x * SPL_LINES, left = lines - line0;
    const int nl = left < (size_t)SPL_LINES ? (int)left : SPL_LINES;
    double* g = coef + line0 * (size_t)n;
    const bool mine = t < nl;
    double* row_a = tile_a + t * SPL_PITCH;
    double* row_b = tile_b + t * SPL_PITCH;
    const double gain = spline_gain(), zn1 = spline_pole_power(n - 1);

    // the start sum: samples i = 1 .. n - 2 in tile_a, their mirror images n - 1 - i in tile_b (row_b reads backwards)
    double s = 0.0, zi = SPLINE_POLE;
    if (mine) s = spline_start_ends(g[(size_t)t * n], g[(size_t)t * n + (size_t)(n - 1)], zn1, gain);
    for (int i0 = 1; i0 <= n - 2; i0 += SPL_CHUNK) {
        const int len = n - 1 - i0 < SPL_CHUNK ? n - 1 - i0 : SPL_CHUNK;
        spl_stage_in(tile_a, g, n, nl, i0, len, t);
        spl_stage_in(tile_b, g, n, nl, n - i0 - len, len, t);
        cvx_barrier();
        if (mine)
            for (int c = 0; c < len; ++c) {
                s = spline_start_term(s, zi, row_a[c], row_b[len - 1 - c], zn1, gain);
                zi *= SPLINE_POLE;
            }
        cvx_barrier();
    }
    // forward, chunks ascending
    double prev = spline_start_done(s, zn1), before = prev;
    for (int x0 = 0; x0 < n; x0 += SPL_CHUNK) {
        const int len = n - x0 < SPL_CHUNK ? n - x0 : SPL_CHUNK;
        spl_stage_in(tile_a, g, n, nl, x0, len, t);
        cvx_barrier();
        if (mine)
            for (int c = 0; c < len; ++c) {
                if (x0 + c > 0) {
                    const double v = spline_forward(row_a[c], prev, gain);
                    before = prev;
                    prev = v;
                }
                row_a[c] = prev;
            }
        cvx_barrier();
        spl_stage_out(tile_a, g, n, nl, x0, len, t);
        cvx_barrier();                              // the stores are visible to the workgroup, and tile_a is free, before the next stage-in
    }
    // backward, chunks descending
    double next = spline_anti_start(prev, before);
    for (int x0 = (n - 1) / SPL_CHUNK * SPL_CHUNK; x0 >= 0; x0 -= SPL_CHUNK) {
        const int len = n - x0 < SPL_CHUNK ? n - x0 : SPL_CHUNK;
        spl_stage_in(tile_a, g, n, nl, x0, len, t);
        cvx_barrier();
        if (mine)
            for (int c = len - 1; c >= 0; --c) {
                if (x0 + c < n - 1) next = spline_backward(next, row_a[c]);
                row_a[c] = next;
            }
        cvx_barrier();
        spl_stage_out(tile_a, g, n, nl, x0, len, t);
        cvx_barrier();
    }
}

template <typename TU>
__global__ __launch_bounds__(SPL_THREADS) void k_map_cubic_f64(const double* __restrict__ coef, const TU* __restrict__ u, size_t cs, size_t vs, int H, int W,
                                                               int D, double* __restrict__ out) {
    const size_t V = (size_t)H * W * D;
    const size_t p = (size_t)blockIdx.x * SPL_THREADS + threadIdx.x;
    if (p >= V) return;
    const int x = (int)(p % D), y = (int)((p / D) % W), z = (int)(p / ((size_t)D * W));
    const double cz = (double)u[p * vs] + (double)z, cy = (double)u[cs + p * vs] + (double)y, cx = (double)u[2 * cs + p * vs] + (double)x;
    out[p] = map_cubic_f64(coef, H, W, D, cz, cy, cx);
}

template <typename TO>
__global__ __launch_bounds__(SPL_THREADS) void k_resample_cubic_f64(const double* __restrict__ coef, int sz, int sy, int sx, TO* __restrict__ out, int oz, int oy,
                                                                    int ox, IndexMap g, double dflt) {
    const size_t V = (size_t)oz * oy * ox;
    const size_t p = (size_t)blockIdx.x * SPL_THREADS + threadIdx.x;
    if (p >= V) return;
    const double i = (double)(int)(p % ox), j = (double)(int)((p / ox) % oy), k = (double)(int)(p / ((size_t)ox * oy));
    const double cx = index_map_axis(g, 0, i, j, k), cy = index_map_axis(g, 1, i, j, k), cz = index_map_axis(g, 2, i, j, k);
    out[p] = (TO)itk_cubic_f64(coef, sz, sy, sx, cz, cy, cx, dflt);          // float output: round to nearest, like .astype(np.float32)
}

static unsigned spl_blocks(size_t items, int per_block) { return (unsigned)((items + (size_t)per_block - 1) / (size_t)per_block); }

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_spline_prefilter_f64(const void* src, int src_f64, int H, int W, int D, double* coef, void* stream) {
    CVX_REQUIRE(src && coef, "cvx_spline_prefilter_f64: null pointer");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_spline_prefilter_f64: bad extent (%dx%dx%d)", H, W, D);
    const size_t V = voxels(H, W, D);
    CVX_REQUIRE(V, "cvx_spline_prefilter_f64: more than 2^31 - 1 voxels (%dx%dx%d)", H, W, D);
    CVX_REQUIRE(((uintptr_t)src & (src_f64 ? 7 : 3)) == 0 && ((uintptr_t)coef & 7) == 0, "cvx_spline_prefilter_f64: a buffer is not aligned to its element");
    const bool in_place = src_f64 && src == (const void*)coef;
    CVX_REQUIRE(in_place || !ranges_overlap(src, V * (src_f64 ? 8 : 4), coef, V * 8),
                "cvx_spline_prefilter_f64: coef overlaps src (only src == coef with double samples filters in place)");
    hipStream_t s = as_stream(stream);
    const size_t plane = (size_t)W * D;
    with_real(src_f64 != 0, [&](auto ts) {
        hipLaunchKernelGGL((k_spline_strided<decltype(ts)>), dim3(spl_blocks(plane, SPL_THREADS)), dim3(SPL_THREADS), 0, s,
                           static_cast<const decltype(ts)*>(src), coef, H, plane, plane, (size_t)0, plane);
    });
    if (W > 1)
        hipLaunchKernelGGL((k_spline_strided<double>), dim3(spl_blocks((size_t)H * D, SPL_THREADS)), dim3(SPL_THREADS), 0, s, (const double*)coef, coef, W,
                           (size_t)D, (size_t)D, plane, (size_t)H * D);
    if (D > 1)
        hipLaunchKernelGGL(k_spline_contig, dim3(spl_blocks((size_t)H * W, SPL_LINES)), dim3(SPL_LINES), 0, s, coef, D, (size_t)H * W);
    return check_last("spline_prefilter");
}

extern "C" int cvx_map_coordinates_cubic_f64(const double* coef, const void* field, int field_f64, int64_t comp_stride, int64_t voxel_stride, int H,
                                             int W, int D, double* out, void* stream) {
    CVX_REQUIRE(coef && field && out, "cvx_map_coordinates_cubic_f64: null pointer");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_map_coordinates_cubic_f64: bad extent (%dx%dx%d)", H, W, D);
    const size_t V = voxels(H, W, D);
    CVX_REQUIRE(V, "cvx_map_coordinates_cubic_f64: more than 2^31 - 1 voxels (%dx%dx%d)", H, W, D);
    const FieldArg f = {field, field_f64 != 0, comp_stride, voxel_stride};
    CVX_REQUIRE(f.strides_ok(V), "cvx_map_coordinates_cubic_f64: bad field strides (component %lld, voxel %lld)", (long long)comp_stride,
                (long long)voxel_stride);
    CVX_REQUIRE(((uintptr_t)coef & 7) == 0 && f.aligned() && ((uintptr_t)out & 7) == 0, "cvx_map_coordinates_cubic_f64: a buffer is not aligned to its element");
    const Span ins[2] = {{coef, V * 8}, f.span(V)};
    const Span outs[1] = {{out, V * 8}};
    CVX_REQUIRE(find_overlaps(outs, ins).out < 0, "cvx_map_coordinates_cubic_f64: out overlaps an input");
    hipStream_t s = as_stream(stream);
    with_real(f.f64 != 0, [&](auto tu) {
        hipLaunchKernelGGL((k_map_cubic_f64<decltype(tu)>), dim3(spl_blocks(V, SPL_THREADS)), dim3(SPL_THREADS), 0, s, coef, static_cast<const decltype(tu)*>(field),
                           (size_t)comp_stride, (size_t)voxel_stride, H, W, D, out);
    });
    return check_last("map_coordinates_cubic");
}

extern "C" int cvx_resample_cubic_f64(const double* coef, int sz, int sy, int sx, void* out, int out_f64, int oz, int oy, int ox, const double* map12_host,
                                      double default_value, void* stream) {
    CVX_REQUIRE(coef && out && map12_host, "cvx_resample_cubic_f64: null pointer");
    CVX_REQUIRE(sz > 0 && sy > 0 && sx > 0 && oz > 0 && oy > 0 && ox > 0, "cvx_resample_cubic_f64: bad extent (source %dx%dx%d, output %dx%dx%d)", sz, sy,
                sx, oz, oy, ox);
    const size_t Vs = voxels(sz, sy, sx), Vo = voxels(oz, oy, ox);
    CVX_REQUIRE(Vs && Vo, "cvx_resample_cubic_f64: more than 2^31 - 1 voxels (source %dx%dx%d, output %dx%dx%d)", sz, sy, sx, oz, oy, ox);
    CVX_REQUIRE(((uintptr_t)coef & 7) == 0 && ((uintptr_t)out & (out_f64 ? 7 : 3)) == 0, "cvx_resample_cubic_f64: a buffer is not aligned to its element");
    CVX_REQUIRE(!ranges_overlap(coef, Vs * 8, out, Vo * (out_f64 ? 8 : 4)), "cvx_resample_cubic_f64: out overlaps an input");
    CVX_REQUIRE(all_finite(map12_host, 12) && isfinite(default_value), "cvx_resample_cubic_f64: non-finite index map or default value");
    const IndexMap g = make_map(map12_host);
    hipStream_t s = as_stream(stream);
    with_real(out_f64 != 0, [&](auto to) {
        hipLaunchKernelGGL((k_resample_cubic_f64<decltype(to)>), dim3(spl_blocks(Vo, SPL_THREADS)), dim3(SPL_THREADS), 0, s, coef, sz, sy, sx,
                           static_cast<decltype(to)*>(out), oz, oy, ox, g, default_value);
    });
    return check_last("resample_cubic");
}
