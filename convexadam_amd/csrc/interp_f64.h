// interp_f64.h -- the float64 linear gather shared by metrics.hip (k_map_linear_f64, apply_convex) and geometry.hip (resampling between
// image grids, carrying a field to the moving image's frame).  One statement of the arithmetic, so that the kernels agree bit for bit:
//   taps_linear_f64   sum over the 8 taps (axis 0 slowest) of ((v * w0) * w1) * w2, started from 0.0, weights {1 - t, 1 - (1 - t)}
//                     -- scipy.ndimage.map_coordinates(order=1) completes its spline weights so that they sum to exactly one
//   map_linear_f64    ... with mode='constant', cval=0: 0 unless 0 <= c <= n - 1 on every axis
//   itk_linear_f64    ... with ITK's buffer rule: inside means -0.5 <= c <= n - 0.5, neighbours beyond the edge are clamped
// Every comparison comes BEFORE the conversion to an integer: a NaN or a huge coordinate fails them and never becomes an index.
// Plain C++ apart from the function qualifiers, so that a host program can run the same text.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define CVX_HD __host__ __device__ __forceinline__
#else
#define CVX_HD inline
#endif

namespace cvx {

// vol[((z * W + y) * D + x) * stride], extents (H, W, D); the CALLER guarantees 0 <= c <= n - 1 on every axis
template <typename T>
CVX_HD double taps_linear_f64(const T* vol, size_t stride, int H, int W, int D, double cz, double cy, double cx) {
    const double fz = floor(cz), fy = floor(cy), fx = floor(cx);
    const double tz = cz - fz, ty = cy - fy, tx = cx - fx;
    const int z0 = (int)fz, y0 = (int)fy, x0 = (int)fx;
    const int z1 = z0 + 1 < H ? z0 + 1 : H - 1, y1 = y0 + 1 < W ? y0 + 1 : W - 1, x1 = x0 + 1 < D ? x0 + 1 : D - 1;
    const int zz[2] = {z0, z1}, yy[2] = {y0, y1}, xx[2] = {x0, x1};
    // w1 = 1 - w0 (not t)
    const double wz[2] = {1.0 - tz, 1.0 - (1.0 - tz)}, wy[2] = {1.0 - ty, 1.0 - (1.0 - ty)}, wx[2] = {1.0 - tx, 1.0 - (1.0 - tx)};
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) r += (((double)vol[(((size_t)zz[i] * W + yy[j]) * D + xx[k]) * stride] * wz[i]) * wy[j]) * wx[k];
    return r;
}

template <typename T>
CVX_HD double map_linear_f64(const T* vol, size_t stride, int H, int W, int D, double cz, double cy, double cx) {
    if (!(cz >= 0.0 && cz <= (double)(H - 1) && cy >= 0.0 && cy <= (double)(W - 1) && cx >= 0.0 && cx <= (double)(D - 1))) return 0.0;
    return taps_linear_f64(vol, stride, H, W, D, cz, cy, cx);
}

CVX_HD bool itk_inside(double c, int n) { return c >= -0.5 && c <= (double)n - 0.5; }
CVX_HD double itk_clamp(double c, int n) {           // min(max(c, 0), n - 1) of a coordinate that passed itk_inside
    const double lo = c < 0.0 ? 0.0 : c, hi = (double)(n - 1);
    return lo > hi ? hi : lo;
}

// index map between two image grids: source index (x, y, z) = m . output index (x, y, z) + t, plain multiplies and adds in this order
struct IndexMap { double m[9], t[3]; };
CVX_HD double index_map_axis(const IndexMap& g, int a, double i, double j, double k) {
    return ((g.m[3 * a] * i + g.m[3 * a + 1] * j) + g.m[3 * a + 2] * k) + g.t[a];
}

}  // namespace cvx
