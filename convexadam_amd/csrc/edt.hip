// edt.hip -- exact Euclidean feature transform on the device: for every voxel the coordinates of the nearest
// ZERO voxel, with the tie-breaking of scipy.ndimage.distance_transform_edt(return_indices=True), which the reference's
// masked feature path calls on the host (convex_adam_MIND.py:44,49).  Algorithm: Maurer, Qi & Raghavan (TPAMI 2003) as in
// scipy's ni_measure.c (_VoronoiFT / _ComputeFT): three passes, one per axis; in a pass every line along that axis is
// independent -- one thread per line, its site stack g[] and the line's copy f[][3] in a thread-interleaved scratch.
// Integer / comparison work on a few MB: latency-bound, three short launches.
#include "cvx_common.h"

namespace cvx {

// obj != 0 -> no site (-1), else the voxel's own coordinates
__global__ __launch_bounds__(256) void k_ft_init(const float* __restrict__ obj, int H, int W, int D, int* __restrict__ feat) {
    const size_t V = (size_t)H * W * D;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const bool site = obj[i] == 0.0f;
    const int x = (int)(i % D), y = (int)((i / D) % W), z = (int)(i / ((size_t)D * W));
    feat[i] = site ? z : -1;
    feat[V + i] = site ? y : -1;
    feat[2 * V + i] = site ? x : -1;
}

// one thread = one line along AXIS; scratch element e of thread t lives at scr[e * nlines + t]
template <int AXIS>
__global__ __launch_bounds__(128) void k_ft_pass(int* __restrict__ feat, int H, int W, int D, int* __restrict__ scr) {
    const int len = AXIS == 0 ? H : (AXIS == 1 ? W : D);
    const int n1 = AXIS == 0 ? W : H, n2 = AXIS == 2 ? W : D;            // the two fixed coordinates (slow, fast)
    const int nlines = n1 * n2;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlines) return;
    const int c1 = t / n2, c2 = t % n2;
    int coor[3];
    size_t base, stride;
    const size_t V = (size_t)H * W * D;
    if (AXIS == 0) { coor[0] = 0; coor[1] = c1; coor[2] = c2; base = (size_t)c1 * D + c2; stride = (size_t)W * D; }
    else if (AXIS == 1) { coor[0] = c1; coor[1] = 0; coor[2] = c2; base = (size_t)c1 * W * D + c2; stride = D; }
    else { coor[0] = c1; coor[1] = c2; coor[2] = 0; base = ((size_t)c1 * W + c2) * D; stride = 1; }
    int* pf = feat + base;
    // scratch views: f[ii][jj] and g[l]
    auto F = [&](int ii, int jj) -> int& { return scr[((size_t)(ii * 3 + jj)) * nlines + t]; };
    auto G = [&](int l) -> int& { return scr[((size_t)(3 * len + l)) * nlines + t]; };
    for (int ii = 0; ii < len; ++ii)
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) F(ii, jj) = pf[ii * stride + jj * V];
    int l = -1;
    for (int ii = 0; ii < len; ++ii) {
        if (F(ii, 0) < 0) continue;
        const double fd = F(ii, AXIS);
        double wR = 0.0;
#pragma unroll
        for (int jj = 0; jj < 3; ++jj)
            if (jj != AXIS) { const double tw = F(ii, jj) - coor[jj]; wR += tw * tw; }
        while (l >= 1) {
            const int idx1 = G(l), idx2 = G(l - 1);
            const double f1 = F(idx1, AXIS), a = f1 - F(idx2, AXIS), b = fd - f1, c = a + b;
            double uR = 0.0, vR = 0.0;
#pragma unroll
            for (int jj = 0; jj < 3; ++jj)
                if (jj != AXIS) {
                    const double cc = coor[jj], tu = F(idx2, jj) - cc, tv = F(idx1, jj) - cc;
                    uR += tu * tu; vR += tv * tv;
                }
            if (c * vR - b * uR - a * wR - a * b * c <= 0.0) break;      // integer-valued doubles: exact
            --l;
        }
        G(++l) = ii;
    }
    const int maxl = l;
    if (maxl < 0) return;
    l = 0;
    for (int ii = 0; ii < len; ++ii) {
        auto dist2 = [&](int site) {
            double s = 0.0;
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) { const double tt = jj == AXIS ? F(site, jj) - ii : F(site, jj) - coor[jj]; s += tt * tt; }
            return s;
        };
        double delta1 = dist2(G(l));
        while (l < maxl) {
            const double delta2 = dist2(G(l + 1));
            if (delta1 <= delta2) break;
            delta1 = delta2;
            ++l;
        }
        const int idx1 = G(l);
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) pf[ii * stride + jj * V] = F(idx1, jj);
    }
}

// the reference's flat index into the half-resolution volume: idx[0]*D//2*W//2 + idx[1]*D//2 + idx[2] with the FULL-resolution
// W, D (convex_adam_MIND.py:45,50), i.e. ((f0*D)//2*W)//2 + (f1*D)//2 + f2 in Python's left-to-right integer arithmetic
__global__ __launch_bounds__(256) void k_ft_flat_index(const int* __restrict__ feat, size_t V, int Wfull, int Dfull,
                                                       int64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const int64_t f0 = feat[i], f1 = feat[V + i], f2 = feat[2 * V + i];
    auto fdiv2 = [](int64_t a) { return a >= 0 ? a / 2 : -((-a + 1) / 2); };    // Python floor division
    out[i] = fdiv2(fdiv2(f0 * Dfull) * Wfull) + fdiv2(f1 * Dfull) + f2;
}


// ---- squared Euclidean distance transform, distances only (HD95 needs no indices) -----------------------------------------------
// Meijster, Roerdink & Hesselink (2000): a 1-D pass along x (distance to the nearest zero voxel of the row) and two lower-envelope
// passes along y and z.  Integer arithmetic throughout: the result is the exact squared distance whatever the order of ties, so it
// equals round(scipy.ndimage.distance_transform_edt(obj)**2) bit for bit.  Rows without a zero voxel carry EDT_INF.
// The y / z passes run one thread per line with the threads of a wavefront on adjacent x (coalesced); their stacks live in a
// thread-interleaved scratch.  A volume without any zero voxel yields values >= EDT_INF^2 (clamped to INT_MAX).
constexpr long long EDT_INF = 1 << 20;

// one wavefront per row: nearest zero to the left / right by scans over the lanes' segments
// SEG: the 2 n volumes are never materialised -- volume 2 i is the mask (seg == labs[i]), volume 2 i + 1 its complement, both read
// straight from the label map (cupy_hd95 with precision 1: saves writing and re-reading 55 MB per label)
struct EdtLabels { int n; float lab[64]; };
template <bool SEG>
__global__ __launch_bounds__(256) void k_edt_rows(const float* __restrict__ obj, int nrows, int D, int* __restrict__ g, EdtLabels el, int rows_per_vol) {
    const int row = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (row >= nrows) return;
    const int volume = SEG ? row / rows_per_vol : 0;
    const float* src = SEG ? obj + (size_t)(row - volume * rows_per_vol) * D : obj + (size_t)row * D;
    const float lab = SEG ? el.lab[volume >> 1] : 0.0f;
    const bool inv = SEG && (volume & 1);
    // "zero voxel of the object": mask volumes are zero OUTSIDE the label, complements INSIDE it
    auto is_zero = [&](int i) { return SEG ? ((src[i] == lab) == inv) : (src[i] == 0.0f); };
    int* dst = g + (size_t)row * D;
    if (D <= 1024) {
        // Round 4: the zero voxels of the row as <= 16 wave-uniform 64-bit masks (one ballot per 64 voxels, coalesced reads); the nearest
        // zero to the left / right of a voxel is a count-leading / trailing-zeros on its own mask, else the nearest non-empty mask.
        // Replaces two lane scans + two sequential walks per row.
        const int nseg = (D + 63) >> 6;
        unsigned long long m[16];
#pragma unroll
        for (int sg = 0; sg < 16; ++sg) {
            const int i = sg * 64 + lane;
            m[sg] = sg < nseg ? __ballot(i < D && is_zero(i < D ? i : 0)) : 0ull;
        }
#pragma unroll
        for (int sg = 0; sg < 16; ++sg) {
            if (sg < nseg) {
                const int i = sg * 64 + lane;
                int l = -1;                                                          // nearest zero at or before i
                const unsigned long long ml = m[sg] & (lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull));
                if (ml) l = sg * 64 + 63 - __builtin_clzll(ml);
                else {
#pragma unroll
                    for (int t = 15; t >= 0; --t)
                        if (t < sg && l < 0 && m[t]) l = t * 64 + 63 - __builtin_clzll(m[t]);
                }
                int r = INT_MAX;                                                     // nearest zero at or after i
                const unsigned long long mr = m[sg] & ~((1ull << lane) - 1ull);
                if (mr) r = sg * 64 + __builtin_ctzll(mr);
                else {
#pragma unroll
                    for (int t = 0; t < 16; ++t)
                        if (t > sg && r == INT_MAX && m[t]) r = t * 64 + __builtin_ctzll(m[t]);
                }
                if (i < D) {
                    const int dl = l < 0 ? (int)EDT_INF : i - l, dr = r == INT_MAX ? (int)EDT_INF : r - i;
                    dst[i] = min(dl, dr);
                }
            }
        }
        return;
    }
    const int per = (D + 63) >> 6;                       // contiguous elements per lane
    const int lo = min(lane * per, D), hi = min(lo + per, D);
    // last zero at or before each position: per-lane last zero, then an inclusive max-scan across lanes
    int last = -1;
    for (int i = lo; i < hi; ++i) if (is_zero(i)) last = i;
    int incl = last;
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl = max(incl, v); }
    int carry = __shfl_up(incl, 1);
    if (lane == 0) carry = -1;
    // first zero at or after each position: per-lane first zero, then an inclusive min-scan from the right
    int first = INT_MAX;
    for (int i = hi - 1; i >= lo; --i) if (is_zero(i)) first = i;
    int incr = first;
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_down(incr, o); if (lane + o < 64) incr = min(incr, v); }
    int carry_r = __shfl_down(incr, 1);
    if (lane == 63) carry_r = INT_MAX;
    // left distances in a forward walk, right distances in a backward walk
    int l = carry;
    for (int i = lo; i < hi; ++i) {
        if (is_zero(i)) l = i;
        dst[i] = l < 0 ? (int)EDT_INF : i - l;
    }
    int r = carry_r;
    for (int i = hi - 1; i >= lo; --i) {
        if (is_zero(i)) r = i;
        const int dr = r == INT_MAX ? (int)EDT_INF : r - i;
        dst[i] = min(dst[i], dr);
    }
}

// lower envelope along one axis; SQUARE_IN: the input holds plain distances (after the row pass) and is squared on the fly
template <bool SQUARE_IN>
__global__ __launch_bounds__(128) void k_edt_envelope(int* __restrict__ vol, int len, int nlines, int inner, size_t line_stride,
                                                      size_t outer_stride, int* __restrict__ scr) {
    // line t: base = (t / inner) * outer_stride + (t % inner); consecutive elements are line_stride apart
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlines) return;
    int* p = vol + (size_t)(t / inner) * outer_stride + (size_t)(t % inner);
    auto F = [&](int i) -> long long { const long long v = p[(size_t)i * line_stride]; return SQUARE_IN ? v * v : v; };
    auto S = [&](int q) -> int& { return scr[(size_t)(2 * q) * nlines + t]; };
    auto T = [&](int q) -> int& { return scr[(size_t)(2 * q + 1) * nlines + t]; };
    auto f = [&](long long x, int i) { const long long dx = x - i; return dx * dx + F(i); };
    int q = 0;
    S(0) = 0; T(0) = 0;
    for (int u = 1; u < len; ++u) {
        while (q >= 0 && f(T(q), S(q)) > f(T(q), u)) --q;
        if (q < 0) { q = 0; S(0) = u; }
        else {
            const long long i = S(q);
            const long long num = (long long)u * u - i * i + F(u) - F((int)i), den = 2 * ((long long)u - i);
            const long long sep = num >= 0 ? num / den : -((-num + den - 1) / den);      // floor division
            const long long w = 1 + sep;
            if (w < len) { ++q; S(q) = u; T(q) = (int)w; }
        }
    }
    // results go to a second scratch plane first: the inputs of this line are still needed while the envelope is evaluated
    for (int u = len - 1; u >= 0; --u) {
        const long long v = f(u, S(q));
        scr[(size_t)(2 * len + u) * nlines + t] = v > INT_MAX ? INT_MAX : (int)v;
        if (u == T(q)) --q;
    }
    for (int u = 0; u < len; ++u) p[(size_t)u * line_stride] = scr[(size_t)(2 * len + u) * nlines + t];
}

// ---- Hausdorff-95 building blocks (reference: cupy_hd95, self_configuring/convexAdam_hyper_util.py:32-51) ----------
// inside = (nearest-resampled label map == label), outside = 1 - inside; nearest index as in ATen's upsample_nearest3d with a given
// scale factor (nearest_idx, UpSample.h): identity when the extent is unchanged, dst >> 1 when it doubles, else
// src = min(floor(dst * sc), in - 1) in float32 with sc = float32(1 / scale_factor) (:33-34); (Ho, Wo, Do) = the resampled extent.
// The identity and >> 1 shortcuts are ATen's CPU kernel (UpSampleKernel.cpp nearest_idx): that is the path the golden vectors were
// captured on (tests/golden/hd95.npz: the reference's cupy_hd95 with torch on the CPU).  ATen's CUDA kernel has no shortcut and
// evaluates floor(dst * sc) always; the two agree for every integer `precision` and can differ only for a non-integer scale whose
// resampled extent happens to equal n_in or 2 n_in -- this library follows the CPU convention there, like its goldens.
__device__ __forceinline__ int nearest_src(int dst, int n_in, int n_out, float sc) {
    return n_out == n_in ? dst : n_out == 2 * n_in ? dst >> 1 : min((int)floorf((float)dst * sc), n_in - 1);
}
__global__ __launch_bounds__(256) void k_label_mask(const float* __restrict__ seg, int H, int W, int D, float label, int Ho, int Wo, int Do, float sc,
                                                    float* __restrict__ inside, float* __restrict__ outside,
                                                    unsigned long long* __restrict__ count) {
    const size_t Vo = (size_t)Ho * Wo * Do;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool in = false;
    if (i < Vo) {
        const int x = (int)(i % Do), y = (int)((i / Do) % Wo), z = (int)(i / ((size_t)Do * Wo));
        const int sz = nearest_src(z, H, Ho, sc), sy = nearest_src(y, W, Wo, sc), sx = nearest_src(x, D, Do, sc);
        in = seg[((size_t)sz * W + sy) * D + sx] == label;
        inside[i] = in ? 1.0f : 0.0f;
        outside[i] = in ? 0.0f : 1.0f;
    }
    if (count) {                                      // one atomic per workgroup (a single hot address serialises them)
        __shared__ unsigned int wsum[4];
        const unsigned long long b = __ballot(in);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (unsigned)__popcll(b);
        cvx_barrier();
        if (threadIdx.x == 0) {
            const unsigned t = wsum[0] + wsum[1] + wsum[2] + wsum[3];
            if (t) atomicAdd(count, (unsigned long long)t);
        }
    }
}

// squared Euclidean distance to the nearest zero voxel of obj (0 on the zero voxels themselves), from the feature transform
__global__ __launch_bounds__(256) void k_edt_sqdist(const float* __restrict__ obj, const int* __restrict__ feat, int H, int W, int D,
                                                    int* __restrict__ d2) {
    const size_t V = (size_t)H * W * D;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    int r = 0;
    if (obj[i] != 0.0f) {
        const int x = (int)(i % D), y = (int)((i / D) % W), z = (int)(i / ((size_t)D * W));
        const int dz = feat[i] - z, dy = feat[V + i] - y, dx = feat[2 * V + i] - x;
        r = dz * dz + dy * dy + dx * dx;
    }
    d2[i] = r;
}

// histogram of the squared distances (a_in2 + a_out2: one of the two is 0 at every voxel) over the surface of b (b_in2 == 1)
__global__ __launch_bounds__(256) void k_surface_hist(const int* __restrict__ a_in2, const int* __restrict__ a_out2,
                                                      const int* __restrict__ b_in2, size_t n, int nbins,
                                                      unsigned long long* __restrict__ hist, int* __restrict__ overflow) {
    // surface voxels are close to the other surface: almost every count lands in a few low bins, which are accumulated per
    // workgroup in LDS and flushed once (global atomics on those few addresses would serialise)
    constexpr int LB = 2048;
    __shared__ unsigned int low[LB];
    for (int i = threadIdx.x; i < LB; i += blockDim.x) low[i] = 0;
    cvx_barrier();
    auto count = [&](size_t i) {
        const int bin = a_in2[i] + a_out2[i];
        if (bin < 0 || bin >= nbins) { *overflow = 1; return; }
        if (bin < LB) atomicAdd(&low[bin], 1u);
        else atomicAdd(&hist[bin], 1ull);
    };
    // the surface test streams b_in2 once (16-byte loads: the 4-byte version ran at 0.67 TB/s); a_in2 / a_out2 are read on the surface only
    const size_t n4 = ((reinterpret_cast<uintptr_t>(b_in2) & 15) == 0) ? n / 4 : 0;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (size_t)gridDim.x * blockDim.x) {
        const int4 b = reinterpret_cast<const int4*>(b_in2)[q];
        if (b.x == 1) count(4 * q);
        if (b.y == 1) count(4 * q + 1);
        if (b.z == 1) count(4 * q + 2);
        if (b.w == 1) count(4 * q + 3);
    }
    for (size_t i = 4 * n4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        if (b_in2[i] == 1) count(i);
    cvx_barrier();
    for (int i = threadIdx.x; i < LB && i < nbins; i += blockDim.x)
        if (low[i]) atomicAdd(&hist[i], (unsigned long long)low[i]);
}

// out[0], out[1] = value (bin index) of the k0-th and k1-th smallest entry (0-based), out[2] = number of entries; -1 if out of range.
// k0 == -2: the two neighbours numpy.percentile interpolates for the quantile `quant` of float32 data are determined here, in
// numpy's float32 arithmetic: virt = float32(n-1) * quant; beyond the last index both are n-1, else floor(virt) and floor(virt)+1.
// One workgroup per histogram (blockIdx.x).  Round 4: coalesced -- wavefront w sums chunks w, w + 16, ... of 1024 bins (16 coalesced
// reads per lane), thread 0 walks the <= 4096 chunk totals to the chunks that hold the two order statistics, and two wavefronts resolve
// them inside their chunk with a lane scan (the first version gave every thread a private contiguous range: 109 uncoalesced reads per
// thread, 170 us per histogram of 111 000 bins -- 4.4 ms of every HD95 call).
__global__ __launch_bounds__(1024) void k_hist_order_stats(const unsigned long long* __restrict__ hist_all, int nbins, long long k0,
                                                           long long k1, float quant, long long* __restrict__ out_all) {
    __shared__ unsigned long long ctot[4096];
    __shared__ long long kk[2], cbase[2];
    __shared__ int cidx[2];
    const unsigned long long* hist = hist_all + (size_t)blockIdx.x * nbins;
    long long* out = out_all + 3 * (size_t)blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nchunks = (nbins + 1023) / 1024;
    for (int c = wave; c < nchunks; c += 16) {
        unsigned long long s = 0;
#pragma unroll 4
        for (int j = 0; j < 16; ++j) { const int b = c * 1024 + j * 64 + lane; if (b < nbins) s += hist[b]; }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
        if (lane == 0) ctot[c] = s;
    }
    cvx_barrier();
    if (t == 0) {
        unsigned long long run = 0;
        for (int c = 0; c < nchunks; ++c) run += ctot[c];
        out[0] = -1; out[1] = -1; out[2] = (long long)run;
        if (k0 == -2) {
            const long long n = (long long)run;
            if (n > 0) {
                const float last = (float)(n - 1);
                const float virt = last * quant;
                if (virt >= last) { k0 = k1 = n - 1; }
                else { k0 = (long long)floorf(virt); k1 = k0 + 1; }
            } else k0 = k1 = -1;
        }
        kk[0] = k0; kk[1] = k1;
        for (int q = 0; q < 2; ++q) {
            const long long k = kk[q];
            cidx[q] = -1; cbase[q] = 0;
            if (k < 0 || (unsigned long long)k >= run) continue;
            unsigned long long before = 0;
            for (int c = 0; c < nchunks; ++c) {
                if ((unsigned long long)k < before + ctot[c]) { cidx[q] = c; cbase[q] = (long long)before; break; }
                before += ctot[c];
            }
        }
    }
    cvx_barrier();
    if (wave < 2 && cidx[wave] >= 0) {
        const int c = cidx[wave];
        const unsigned long long k = (unsigned long long)kk[wave];
        unsigned long long v[16], s = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) { const int b = c * 1024 + lane * 16 + j; v[j] = b < nbins ? hist[b] : 0ull; s += v[j]; }
        unsigned long long incl = s;
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long u = __shfl_up(incl, o); if (lane >= o) incl += u; }
        unsigned long long before = (unsigned long long)cbase[wave] + incl - s;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (v[j] && k >= before && k < before + v[j]) out[wave] = c * 1024 + lane * 16 + j;
            before += v[j];
        }
    }
}

}  // namespace cvx

using namespace cvx;

// per line: 3*len coordinates + len stack entries, for the pass with the largest (lines x length) = 4 * V ints
static int* ft_layout(Carver& cv, int H, int W, int D) { return cv.take<int>(4 * (size_t)H * W * D); }
extern "C" size_t cvx_feature_transform_workspace_bytes(int H, int W, int D) { Carver m; ft_layout(m, H, W, D); return ws_query(m); }

extern "C" int cvx_feature_transform_i32(const float* obj, int H, int W, int D, int* feat, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    CVX_REQUIRE(obj && feat && workspace, "cvx_feature_transform_i32: null pointer");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_feature_transform_i32: bad extent %dx%dx%d", H, W, D);
    if (workspace_bytes < cvx_feature_transform_workspace_bytes(H, W, D))
        return fail(CVX_ERR_WORKSPACE, "cvx_feature_transform_i32: workspace too small");
    hipStream_t s = as_stream(stream);
    Carver cv(workspace);
    const size_t V = (size_t)H * W * D;
    int* scr = ft_layout(cv, H, W, D);
    hipLaunchKernelGGL(k_ft_init, dim3((unsigned)cdiv64((int64_t)V, 256)), dim3(256), 0, s, obj, H, W, D, feat);
    hipLaunchKernelGGL(k_ft_pass<0>, dim3(cdiv(W * D, 128)), dim3(128), 0, s, feat, H, W, D, scr);
    hipLaunchKernelGGL(k_ft_pass<1>, dim3(cdiv(H * D, 128)), dim3(128), 0, s, feat, H, W, D, scr);
    hipLaunchKernelGGL(k_ft_pass<2>, dim3(cdiv(H * W, 128)), dim3(128), 0, s, feat, H, W, D, scr);
    return check_last("feature_transform");
}

extern "C" int cvx_feature_flat_index_i64(const int* feat, int H, int W, int D, int W_full, int D_full, int64_t* out, void* stream) {
    CVX_REQUIRE(feat && out, "cvx_feature_flat_index_i64: null pointer");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0 && W_full > 0 && D_full > 0, "cvx_feature_flat_index_i64: bad extent");
    const size_t V = (size_t)H * W * D;
    hipLaunchKernelGGL(k_ft_flat_index, dim3((unsigned)cdiv64((int64_t)V, 256)), dim3(256), 0, as_stream(stream), feat, V, W_full, D_full, out);
    return check_last("feature_flat_index");
}

extern "C" int cvx_label_mask_f32(const float* seg, int H, int W, int D, int label, int precision, float* inside, float* outside,
                                  int64_t* count, void* stream) {
    CVX_REQUIRE(seg && inside && outside, "cvx_label_mask_f32: null pointer");     // count may be NULL
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_label_mask_f32: bad extent %dx%dx%d", H, W, D);
    CVX_REQUIRE(precision >= 1 && precision <= 8, "cvx_label_mask_f32: precision %d not in 1..8", precision);
    hipStream_t s = as_stream(stream);
    const size_t Vo = (size_t)H * W * D * precision * precision * precision;
    if (count && hipMemsetAsync(count, 0, sizeof(int64_t), s) != hipSuccess) return fail(CVX_ERR_LAUNCH, "cvx_label_mask_f32: memset failed");
    hipLaunchKernelGGL(k_label_mask, dim3((unsigned)cdiv64((int64_t)Vo, 256)), dim3(256), 0, s, seg, H, W, D, (float)label, H * precision, W * precision,
                       D * precision, 1.0f / (float)precision, inside, outside, reinterpret_cast<unsigned long long*>(count));
    return check_last("label_mask");
}

extern "C" int cvx_label_mask_scaled_f32(const float* seg, int H, int W, int D, int label, int Ho, int Wo, int Do, float scale_inv, float* inside,
                                         float* outside, int64_t* count, void* stream) {
    CVX_REQUIRE(seg && inside && outside, "cvx_label_mask_scaled_f32: null pointer");     // count may be NULL
    CVX_REQUIRE(H > 0 && W > 0 && D > 0 && Ho > 0 && Wo > 0 && Do > 0, "cvx_label_mask_scaled_f32: bad extent %dx%dx%d -> %dx%dx%d", H, W, D, Ho, Wo, Do);
    CVX_REQUIRE(scale_inv > 0.0f && scale_inv <= 1.0e6f, "cvx_label_mask_scaled_f32: scale_inv must be float32(1 / scale_factor) > 0");
    CVX_REQUIRE((double)Ho * Wo * Do < 2147483647.0 * 4.0, "cvx_label_mask_scaled_f32: resampled volume too large");
    hipStream_t s = as_stream(stream);
    const size_t Vo = (size_t)Ho * Wo * Do;
    if (count && hipMemsetAsync(count, 0, sizeof(int64_t), s) != hipSuccess) return fail(CVX_ERR_LAUNCH, "cvx_label_mask_scaled_f32: memset failed");
    hipLaunchKernelGGL(k_label_mask, dim3((unsigned)cdiv64((int64_t)Vo, 256)), dim3(256), 0, s, seg, H, W, D, (float)label, Ho, Wo, Do, scale_inv, inside, outside,
                       reinterpret_cast<unsigned long long*>(count));
    return check_last("label_mask_scaled");
}

extern "C" int cvx_edt_sqdist_i32(const float* obj, const int* feat, int H, int W, int D, int* d2, void* stream) {
    CVX_REQUIRE(obj && feat && d2, "cvx_edt_sqdist_i32: null pointer");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_edt_sqdist_i32: bad extent %dx%dx%d", H, W, D);
    CVX_REQUIRE((double)H * H + (double)W * W + (double)D * D < 2147483647.0, "cvx_edt_sqdist_i32: extent too large for int32 distances");
    const size_t V = (size_t)H * W * D;
    hipLaunchKernelGGL(k_edt_sqdist, dim3((unsigned)cdiv64((int64_t)V, 256)), dim3(256), 0, as_stream(stream), obj, feat, H, W, D, d2);
    return check_last("edt_sqdist");
}

extern "C" int cvx_surface_hist_i64(const int* a_in2, const int* a_out2, const int* b_in2, int64_t n, int nbins, int64_t* hist,
                                    int* overflow, void* stream) {
    CVX_REQUIRE(a_in2 && a_out2 && b_in2 && hist && overflow, "cvx_surface_hist_i64: null pointer");
    CVX_REQUIRE(n > 0 && nbins > 0, "cvx_surface_hist_i64: bad size");
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(hist, 0, sizeof(int64_t) * (size_t)nbins, s) != hipSuccess || hipMemsetAsync(overflow, 0, sizeof(int), s) != hipSuccess)
        return fail(CVX_ERR_LAUNCH, "cvx_surface_hist_i64: memset failed");
    const unsigned nb = (unsigned)(cdiv64(n, 256) < 2048 ? cdiv64(n, 256) : 2048);
    hipLaunchKernelGGL(k_surface_hist, dim3(nb), dim3(256), 0, s, a_in2, a_out2, b_in2, (size_t)n, nbins,
                       reinterpret_cast<unsigned long long*>(hist), overflow);
    return check_last("surface_hist");
}

// all (label, direction) histograms of one cupy_hd95 call in ONE launch: blockIdx.y = histogram h, its three volumes from a device table
// of addresses tab[3 h .. 3 h + 2] = (a_in2, a_out2, b_in2); hist [n_hist][nbins], overflow [n_hist] (26 launches of ~35 us -> one)
__global__ __launch_bounds__(256) void k_surface_hist_batch(const unsigned long long* __restrict__ tab, size_t n, int nbins,
                                                            unsigned long long* __restrict__ hist_all, int* __restrict__ overflow_all) {
    constexpr int LB = 2048;
    __shared__ unsigned int low[LB];
    const int h = blockIdx.y;
    const int* a_in2 = reinterpret_cast<const int*>(tab[3 * h]);
    const int* a_out2 = reinterpret_cast<const int*>(tab[3 * h + 1]);
    const int* b_in2 = reinterpret_cast<const int*>(tab[3 * h + 2]);
    unsigned long long* hist = hist_all + (size_t)h * nbins;
    int* overflow = overflow_all + h;
    for (int i = threadIdx.x; i < LB; i += blockDim.x) low[i] = 0;
    cvx_barrier();
    auto count = [&](size_t i) {
        const int bin = a_in2[i] + a_out2[i];
        if (bin < 0 || bin >= nbins) { *overflow = 1; return; }
        if (bin < LB) atomicAdd(&low[bin], 1u);
        else atomicAdd(&hist[bin], 1ull);
    };
    const size_t n4 = ((reinterpret_cast<uintptr_t>(b_in2) & 15) == 0) ? n / 4 : 0;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (size_t)gridDim.x * blockDim.x) {
        const int4 b = reinterpret_cast<const int4*>(b_in2)[q];
        if (b.x == 1) count(4 * q);
        if (b.y == 1) count(4 * q + 1);
        if (b.z == 1) count(4 * q + 2);
        if (b.w == 1) count(4 * q + 3);
    }
    for (size_t i = 4 * n4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        if (b_in2[i] == 1) count(i);
    cvx_barrier();
    for (int i = threadIdx.x; i < LB && i < nbins; i += blockDim.x)
        if (low[i]) atomicAdd(&hist[i], (unsigned long long)low[i]);
}
extern "C" int cvx_surface_hist_batch_i64(const void* const* volumes_dev, int n_hist, int64_t n, int nbins, int64_t* hist, int* overflow, void* stream) {
    CVX_REQUIRE(volumes_dev && hist && overflow && n_hist > 0 && n_hist <= 65535 && n > 0 && nbins > 0, "cvx_surface_hist_batch_i64: bad arguments");
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(hist, 0, sizeof(int64_t) * (size_t)nbins * n_hist, s) != hipSuccess || hipMemsetAsync(overflow, 0, sizeof(int) * n_hist, s) != hipSuccess)
        return fail(CVX_ERR_LAUNCH, "cvx_surface_hist_batch_i64: memset failed");
    const unsigned nb = (unsigned)(cdiv64(n, 4096) < 256 ? (cdiv64(n, 4096) ? cdiv64(n, 4096) : 1) : 256);
    hipLaunchKernelGGL(k_surface_hist_batch, dim3(nb, n_hist), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(volumes_dev), (size_t)n, nbins,
                       reinterpret_cast<unsigned long long*>(hist), overflow);
    return check_last("surface_hist_batch");
}
extern "C" int cvx_hist_order_stats_i64(const int64_t* hist, int nbins, int64_t k0, int64_t k1, int64_t* out3, void* stream) {
    CVX_REQUIRE(hist && out3, "cvx_hist_order_stats_i64: null pointer");
    CVX_REQUIRE(nbins > 0 && nbins <= 4096 * 1024, "cvx_hist_order_stats_i64: bad size (1 .. 4 194 304 bins: chunk totals live in LDS)");
    hipLaunchKernelGGL(k_hist_order_stats, dim3(1), dim3(1024), 0, as_stream(stream), reinterpret_cast<const unsigned long long*>(hist),
                       nbins, (long long)k0, (long long)k1, 0.0f, reinterpret_cast<long long*>(out3));
    return check_last("hist_order_stats");
}

extern "C" int cvx_hist_percentile_neighbours_i64(const int64_t* hist, int nbins, float quantile, int64_t* out3, void* stream) {
    return cvx_hist_percentile_neighbours_batch_i64(hist, nbins, 1, quantile, out3, stream);
}
extern "C" int cvx_hist_percentile_neighbours_batch_i64(const int64_t* hist, int nbins, int n_hist, float quantile, int64_t* out3, void* stream) {
    CVX_REQUIRE(hist && out3, "cvx_hist_percentile_neighbours_i64: null pointer");
    CVX_REQUIRE(nbins > 0 && nbins <= 4096 * 1024 && n_hist > 0 && quantile >= 0.0f && quantile <= 1.0f, "cvx_hist_percentile_neighbours_i64: bad arguments");
    hipLaunchKernelGGL(k_hist_order_stats, dim3(n_hist), dim3(1024), 0, as_stream(stream), reinterpret_cast<const unsigned long long*>(hist),
                       nbins, -2ll, -2ll, quantile, reinterpret_cast<long long*>(out3));
    return check_last("hist_percentile_neighbours");
}

// Tiled lower-envelope pass (round 4): a workgroup stages the lines of 64 adjacent x columns of one plane in LDS (len x 64 ints,
// squared on the fly after the row pass) and every thread evaluates its outputs by an OUTWARD search
//     out(u) = min_i (u - i)^2 + F(i):   best = F(u);  for k = 1, 2, ...  while k^2 < best:  best = min(best, k^2 + F(u -+ k))
// -- exact (integers; every i with (u - i)^2 < out(u) is visited), embarrassingly parallel, LDS reads at lane-consecutive
// addresses, no stacks in global memory.  The search radius is the distance itself: label maps with structures a few voxels wide
// stop after a few steps (the sweep's HD95: 39 -> ~5 ms per evaluation with 13 labels).  "No zero voxel" is carried as EDT_SENT
// (larger than any squared distance inside an int32 volume) and mapped to INT_MAX at the end, as the sequential pass does.
constexpr int EDT_SENT = 1 << 30;
template <bool SQUARE_IN, bool FINAL>
__global__ __launch_bounds__(256) void k_edt_envelope_tile(int* __restrict__ vol, int len, int inner, size_t line_stride, size_t outer_stride,
                                                           int ntx, size_t batch_stride) {
    extern __shared__ int edt_lds[];                       // [len][64]
    const int tx = blockIdx.x % ntx, outer = blockIdx.x / ntx;
    const int x0 = tx * 64, nx = min(64, inner - x0);
    int* base = vol + (size_t)blockIdx.y * batch_stride + (size_t)outer * outer_stride + x0;
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;          // 4 wavefronts share the lines: u = part, part + 4, ...
    for (int u = part; u < len; u += 4) {
        int v = EDT_SENT;
        if (lane < nx) {
            const long long g = base[(size_t)u * line_stride + lane];
            if (SQUARE_IN) { const long long q = g * g; v = q >= EDT_SENT ? EDT_SENT : (int)q; }
            else v = g >= EDT_SENT ? EDT_SENT : (int)g;
        }
        edt_lds[u * 64 + lane] = v;
    }
    cvx_barrier();
    if (lane >= nx) return;
    // four outputs per thread in flight (u = part + 4 (4 j + e), e = 0..3): the search loop is a chain of dependent LDS reads, four
    // independent chains hide its latency (1.93 -> ~1 ms for the y pass of 26 volumes)
    for (int u0 = part; u0 < len; u0 += 16) {
        int uu[4], best[4], kmax = 0;
        bool act[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            uu[e] = u0 + 4 * e;
            act[e] = uu[e] < len;
            best[e] = act[e] ? edt_lds[uu[e] * 64 + lane] : 0;
            if (act[e]) kmax = max(kmax, max(uu[e], len - 1 - uu[e]));
        }
        for (int k = 1; k <= kmax; ++k) {
            const int kk = k * k;
            bool any = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) any = any || (act[e] && kk < best[e]);
            if (!any) break;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (act[e] && kk < best[e]) {
                    const int a = uu[e] - k >= 0 ? edt_lds[(uu[e] - k) * 64 + lane] : EDT_SENT;
                    const int b = uu[e] + k < len ? edt_lds[(uu[e] + k) * 64 + lane] : EDT_SENT;
                    const int mm = min(a, b);
                    best[e] = min(best[e], mm >= EDT_SENT ? EDT_SENT : mm + kk);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (act[e]) base[(size_t)uu[e] * line_stride + lane] = (FINAL && best[e] >= EDT_SENT) ? INT_MAX : best[e];
    }
}

// per line: 2 stack entries + 1 result per element, for the pass with the largest (lines x length) = 3 * V ints per volume
static int* edt_layout(Carver& cv, int batch, int H, int W, int D) { return cv.take<int>(3 * (size_t)batch * H * W * D); }
extern "C" size_t cvx_edt_squared_workspace_bytes(int batch, int H, int W, int D) { Carver m; edt_layout(m, batch > 0 ? batch : 1, H, W, D); return ws_query(m); }

// `batch` independent volumes [batch][H][W][D] in one set of launches (one thread per line: a single 160 x 192 x 224 volume leaves
// most of the GPU idle in the envelope passes)
static int edt_squared_impl(const float* obj, const EdtLabels* labels, int batch, int H, int W, int D, int* d2, void* workspace, size_t workspace_bytes,
                            void* stream);
extern "C" int cvx_edt_squared_i32(const float* obj, int batch, int H, int W, int D, int* d2, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    return edt_squared_impl(obj, nullptr, batch, H, W, D, d2, workspace, workspace_bytes, stream);
}
extern "C" int cvx_edt_squared_labels_i32(const float* seg, int H, int W, int D, const int* labels_host, int n_labels, int* d2, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    CVX_REQUIRE(labels_host && n_labels >= 1 && n_labels <= 64, "cvx_edt_squared_labels_i32: 1 .. 64 labels per call");
    EdtLabels el;
    el.n = n_labels;
    for (int i = 0; i < 64; ++i) el.lab[i] = i < n_labels ? (float)labels_host[i] : 0.0f;
    return edt_squared_impl(seg, &el, 2 * n_labels, H, W, D, d2, workspace, workspace_bytes, stream);
}
static int edt_squared_impl(const float* obj, const EdtLabels* labels, int batch, int H, int W, int D, int* d2, void* workspace, size_t workspace_bytes,
                            void* stream) {
    CVX_REQUIRE(obj && d2 && workspace, "cvx_edt_squared_i32: null pointer");
    CVX_REQUIRE(batch > 0 && H > 0 && W > 0 && D > 0, "cvx_edt_squared_i32: bad extent %d x %dx%dx%d", batch, H, W, D);
    CVX_REQUIRE((double)H * H + (double)W * W + (double)D * D < 2147483647.0, "cvx_edt_squared_i32: extent too large for int32 squared distances");
    CVX_REQUIRE((double)batch * H * W * D < 2147483647.0 * 0.3, "cvx_edt_squared_i32: batch too large");
    if (workspace_bytes < cvx_edt_squared_workspace_bytes(batch, H, W, D)) return fail(CVX_ERR_WORKSPACE, "cvx_edt_squared_i32: workspace too small");
    hipStream_t s = as_stream(stream);
    Carver cv(workspace);
    int* scr = edt_layout(cv, batch, H, W, D);
    const int nrows = batch * H * W;
    if (labels) hipLaunchKernelGGL(k_edt_rows<true>, dim3((unsigned)cdiv(nrows, 4)), dim3(256), 0, s, obj, nrows, D, d2, *labels, H * W);
    else hipLaunchKernelGGL(k_edt_rows<false>, dim3((unsigned)cdiv(nrows, 4)), dim3(256), 0, s, obj, nrows, D, d2, EdtLabels{}, H * W);
    if ((size_t)max(H, W) * 64 * sizeof(int) <= 160 * 1024 && !options().edt_sequential) {
        // tiled outward-search passes: lines of 64 adjacent columns in LDS.  y: planes (volume, z), lines D apart; z: slabs (volume, y)
        const int ntx = cdiv(D, 64);
        static size_t granted_y = 0, granted_z = 0;
        ensure_dynamic_lds(&k_edt_envelope_tile<true, false>, (size_t)W * 256, granted_y);
        ensure_dynamic_lds(&k_edt_envelope_tile<false, true>, (size_t)H * 256, granted_z);
        CVX_REQUIRE(batch <= 65535, "cvx_edt_squared_i32: at most 65535 volumes per call");
        hipLaunchKernelGGL((k_edt_envelope_tile<true, false>), dim3((unsigned)(H * ntx), batch), dim3(256), (size_t)W * 256, s, d2, W, D, (size_t)D,
                           (size_t)W * D, ntx, (size_t)H * W * D);
        hipLaunchKernelGGL((k_edt_envelope_tile<false, true>), dim3((unsigned)(W * ntx), batch), dim3(256), (size_t)H * 256, s, d2, H, D,
                           (size_t)W * D, (size_t)D, ntx, (size_t)H * W * D);
        return check_last("edt_squared");
    }
    // along y: lines (volume, z, x), consecutive elements D apart; along z: lines (volume, y, x), consecutive elements W*D apart
    hipLaunchKernelGGL(k_edt_envelope<true>, dim3((unsigned)cdiv(batch * H * D, 128)), dim3(128), 0, s, d2, W, batch * H * D, D, (size_t)D,
                       (size_t)W * D, scr);
    hipLaunchKernelGGL(k_edt_envelope<false>, dim3((unsigned)cdiv(batch * W * D, 128)), dim3(128), 0, s, d2, H, batch * W * D, W * D,
                       (size_t)W * D, (size_t)H * W * D, scr);
    return check_last("edt_squared");
}
