// geometry_args.h -- the host-side argument checks shared by the entry points of geometry.hip and fieldmean.hip: one statement of what an
// overlap, a finite host array, an acceptable volume and an index map are.  Included after cvx_common.h and interp_f64.h.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>

namespace cvx {

static bool ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bbytes && pb < pa + abytes;
}
static bool all_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!isfinite(v[i])) return false;
    return true;
}
// voxels of a volume, or 0 when an extent is below 1 or the product does not fit an int
static size_t voxels(int a, int b, int c) {
    if (a < 1 || b < 1 || c < 1) return 0;
    const uint64_t ab = (uint64_t)a * (uint64_t)b;
    if (ab > (uint64_t)INT_MAX) return 0;
    const uint64_t v = ab * (uint64_t)c;
    if (v > (uint64_t)INT_MAX) return 0;
    return (size_t)v;
}
static IndexMap make_map(const double* map12) {
    IndexMap g;
    for (int i = 0; i < 9; ++i) g.m[i] = map12[i];
    for (int i = 0; i < 3; ++i) g.t[i] = map12[9 + i];
    return g;
}

}  // namespace cvx
