// geometry_args.h -- the host-side argument checks shared by the entry points of geometry.hip, fieldmean.hip, fieldops.hip and
// affine.hip: one statement of what an overlap, a finite host array, an acceptable volume, a field operand and an index map are.
// Included after cvx_common.h and interp_f64.h.
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
// a field operand (include/convexadam_field.h, convexadam_affine.h): the strides do not fold components onto each other (the rule of
// cvx_field_to_grid_f64), the bytes it spans, and the base aligned to its element
static bool field_strides_ok(int64_t cs, int64_t vs, size_t V) {
    const bool range = cs > 0 && vs > 0 && cs < ((int64_t)1 << 40) && vs < ((int64_t)1 << 20);
    return range && (vs >= 3 * cs || cs >= (int64_t)V * vs);
}
static size_t field_bytes(int64_t cs, int64_t vs, size_t V, int f64) { return (size_t)(2 * cs + (int64_t)(V - 1) * vs + 1) * (f64 ? 8 : 4); }
static bool field_aligned(const void* p, int f64) { return ((uintptr_t)p & (f64 ? 7 : 3)) == 0; }
static IndexMap make_map(const double* map12) {
    IndexMap g;
    for (int i = 0; i < 9; ++i) g.m[i] = map12[i];
    for (int i = 0; i < 3; ++i) g.t[i] = map12[9 + i];
    return g;
}

}  // namespace cvx
