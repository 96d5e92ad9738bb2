// geometry_args.h -- the host-side argument handling shared by the entry points of geometry.hip, fieldmean.hip, cropfield.hip, fieldops.hip,
// affine.hip, ranksum.hip, prep.hip and ssim.hip: one statement of what an overlap (of two ranges, of nullable ranges, among the outputs
// and inputs of a call), a finite host array, an acceptable volume, a field operand, a float/double element flag and an index map are.
// Included after cvx_common.h.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "interp_f64.h"

namespace cvx {

static bool ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bbytes && pb < pa + abytes;
}
// ... of two buffers either of which may be absent
static bool overlap_any(const void* a, size_t ab, const void* b, size_t bb) { return a && b && ranges_overlap(a, ab, b, bb); }

// the buffers of a call: `out` is the first output that overlaps an input (-1: none does), `a` < `b` the first two outputs that overlap
// each other (-1: no two do); absent buffers (null) are skipped.  The entry point words the refusal, inputs first.
struct Span { const void* p; size_t bytes; };
struct Overlaps { int out, a, b; };
template <int NO, int NI>
static Overlaps find_overlaps(const Span (&outs)[NO], const Span (&ins)[NI]) {
    Overlaps r = {-1, -1, -1};
    for (int o = 0; o < NO; ++o) {
        for (int i = 0; i < NI; ++i)
            if (r.out < 0 && overlap_any(outs[o].p, outs[o].bytes, ins[i].p, ins[i].bytes)) r.out = o;
        for (int q = o + 1; q < NO; ++q)
            if (r.a < 0 && overlap_any(outs[o].p, outs[o].bytes, outs[q].p, outs[q].bytes)) r.a = o, r.b = q;
    }
    return r;
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
// a field operand (include/convexadam_field.h, convexadam_affine.h): component c of voxel q at p[c * cs + q * vs].  The strides do not fold
// components onto each other -- interleaved [..][3] (strides 1, 3), planar [3][..] (V, 1), or any other such layout --, the bytes it spans,
// and the base aligned to its element
static bool field_strides_ok(int64_t cs, int64_t vs, size_t V) {
    const bool range = cs > 0 && vs > 0 && cs < ((int64_t)1 << 40) && vs < ((int64_t)1 << 20);
    return range && (vs >= 3 * cs || cs >= (int64_t)V * vs);
}
static size_t field_bytes(int64_t cs, int64_t vs, size_t V, int f64) { return (size_t)(2 * cs + (int64_t)(V - 1) * vs + 1) * (f64 ? 8 : 4); }
static bool field_aligned(const void* p, int f64) { return ((uintptr_t)p & (f64 ? 7 : 3)) == 0; }
struct FieldArg {
    const void* p; int f64; int64_t cs, vs;
    bool strides_ok(size_t V) const { return field_strides_ok(cs, vs, V); }
    size_t bytes(size_t V) const { return field_bytes(cs, vs, V, f64); }
    bool aligned() const { return field_aligned(p, f64); }
    Span span(size_t V) const { return {p, p ? bytes(V) : 0}; }
};

// an element flag (`*_f64`) as a type: calls f(double{}) or f(float{}); nested where several operands vary
template <class F>
static void with_real(bool f64, F&& f) {
    if (f64) f(double{});
    else f(float{});
}

static IndexMap make_map(const double* map12) {
    IndexMap g;
    for (int i = 0; i < 9; ++i) g.m[i] = map12[i];
    for (int i = 0; i < 3; ++i) g.t[i] = map12[9 + i];
    return g;
}

}  // namespace cvx
