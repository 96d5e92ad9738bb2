// ssim.hip -- 3-D structural similarity with a separable Gaussian window in ONE stencil kernel (+ a small fixed-order reduction).
//
// Reference: tests/helper_functions.py:102-145 (ssim3D / _ssim_3D, adapted there from pytorch-ssim-3D), the acceptance criterion of
// tests/test_convex_adam_mind.py:45-85.  The reference filters x, y, x*x, y*y and x*y with a dense ws^3 window (five grouped conv3d calls,
// zero padding, no renormalisation at the border); the window is the outer product of one 1-D Gaussian, so the same five moments are
// three 1-D passes.  All arithmetic float32, fused only where fmaf is written, IEEE division.
//
// Shape: a workgroup of SSIM_TW x SSIM_TD threads owns that (W, D) tile of one (n, c) volume and walks a chunk of H.  Per input plane
//   stage   the haloed tile of both images in LDS (halo R = ws / 2 on each side, zeros outside the volume); its loads were issued
//           one plane ahead and waited in registers,
//   D pass  every staged row: the five products filtered along D                       (SSIM_TW + 2 R rows, back to LDS),
//   W pass  the thread's own (w, d): the five D-filtered moments filtered along W      (lanes run along D: conflict-free reads),
//   H pass  a ring of the last ws planes' (D, W)-filtered moments in registers (5 ws values; the plane loop is unrolled ws times, so
//           every slot index is a compile-time constant and nothing moves), filtered along H for the plane R steps back, then the
//           SSIM expression and the store.
// The ring starts R planes before the chunk (recomputed by the neighbouring chunk: the price of filling the chip along H); planes
// outside the volume are zeros and cost nothing.  The tap order of every pass is fixed (lowest index first), so a voxel's bits do not
// depend on the chunking, the batch position or the outputs requested.
// Means: every thread adds its column's values in float64 in plane order, a workgroup adds its SSIM_TW rows per D column in row order and
// writes SSIM_TD float64 partials; k_ssim_finish adds the partials in index order.  No atomics: the same bits on every run.
#include "cvx_common.h"
#include "geometry_args.h"

namespace cvx {

constexpr int SSIM_TW = 16, SSIM_TD = 32;               // the (W, D) tile; convexadam_amd/ssim.py::TILE repeats these three numbers
constexpr int SSIM_MIN_HCHUNK = 16;                     // shortest H chunk (R halo planes are filtered twice per chunk boundary)
constexpr int SSIM_THREADS = SSIM_TW * SSIM_TD;
constexpr int SSIM_MAX_WS = 11;
constexpr int SSIM_WG_TARGET = 512;                     // workgroups a launch aims for before it stops cutting H: two per CU
constexpr int SSIM_FIN_THREADS = 256;

struct SsimTaps { float g[SSIM_MAX_WS]; };

// WHO computes WHAT: decided once, for the size query and the launcher
struct SsimPlan { int ntw, ntd, nch, hlen, max_ch; int64_t nwg; };
static SsimPlan ssim_plan(int64_t nc, int H, int W, int D) {
    SsimPlan p;
    p.ntw = cdiv(W, SSIM_TW);
    p.ntd = cdiv(D, SSIM_TD);
    const int64_t base = nc * p.ntw * p.ntd;
    p.max_ch = H / SSIM_MIN_HCHUNK > 1 ? H / SSIM_MIN_HCHUNK : 1;
    const int64_t want = cdiv64(SSIM_WG_TARGET, base);
    const int nch = (int)(want < p.max_ch ? want : p.max_ch);
    p.hlen = cdiv(H, nch);
    p.nch = cdiv(H, p.hlen);
    p.nwg = base * p.nch;
    return p;
}
// the workspace: SSIM_TD float64 partial sums per workgroup, sized for the finest chunking of this extent (so the query grows with n * c)
struct SsimWs { double* partial; };
static SsimWs ssim_layout(Carver& cv, int64_t nc, const SsimPlan& p) {
    return SsimWs{cv.take<double>((size_t)(nc * p.ntw * p.ntd * p.max_ch) * SSIM_TD)};
}

// what a workgroup's threads share about their tile
struct SsimTile {
    const float *X, *Y;          // the (n, c) volume
    float* map;                  // the same volume of the map, or null
    int H, W, D, w0, d0, h0;     // extent; first voxel of the tile and of the H chunk
    int tid, tx, ty;
    bool inside;                 // the thread's (w, d) lies inside the volume
};

// The five moments travel as two register pairs and a single: (x, y) -> (mu1, mu2), (x x, y y) -> (G*xx, G*yy), and x y.  A pair is one 8-byte
// LDS access and one packed instruction (v_pk_mul_f32 / v_pk_fma_f32: the same IEEE operation in both halves), so a tap costs three
// filter instructions instead of five.
struct SsimMoments { f32x2 mu, sq; float xy; };
__device__ __forceinline__ f32x2 fma2(float g, f32x2 v, f32x2 a) { return __builtin_elementwise_fma(f32x2{g, g}, v, a); }
// one ds_read_b64 (256 B per clock); left alone, the compiler pairs two of them into a ds_read2_b64, which runs at half that rate
__device__ __forceinline__ f32x2 ld2(const f32x2* p) { return lds_load2(reinterpret_cast<const float*>(p)); }

// a thread's share of the haloed plane tile: elements tid, tid + SSIM_THREADS, ... of [RW][SP]; off = w * D + d inside the plane, -1 outside
// the volume (or behind the tile's last element); xy = the values of the plane in flight
template <int R>
struct SsimStage {
    static constexpr int N = ((SSIM_TW + 2 * R) * (SSIM_TD + 2 * R) + SSIM_THREADS - 1) / SSIM_THREADS;
    int off[N];
    f32x2 xy[N];
};
// the LDS of one workgroup: the staged plane, the D-filtered rows, the final reduction
template <int R>
struct SsimLds {
    static constexpr int RW = SSIM_TW + 2 * R, SP = SSIM_TD + 2 * R;
    f32x2 in[RW * SP];                       // (x, y) of the haloed tile
    f32x2 mu[RW * SSIM_TD], sq[RW * SSIM_TD];  // filtered along D
    float xy[RW * SSIM_TD];
    double red[SSIM_THREADS];
};
template <int R>
__device__ __forceinline__ void ssim_stage_init(const SsimTile& t, SsimStage<R>& st) {
    constexpr int RW = SSIM_TW + 2 * R, SP = SSIM_TD + 2 * R;
#pragma unroll
    for (int j = 0; j < SsimStage<R>::N; ++j) {
        const int i = t.tid + j * SSIM_THREADS, r = i / SP, c = i - r * SP;
        const int w = t.w0 - R + r, d = t.d0 - R + c;
        st.off[j] = (i < RW * SP && (unsigned)w < (unsigned)t.W && (unsigned)d < (unsigned)t.D) ? w * t.D + d : -1;
        st.xy[j] = f32x2{0.0f, 0.0f};
    }
}
// plane p of both images into the thread's registers (zeros outside the volume); a plane outside [0, H) is never staged
template <int R>
__device__ __forceinline__ void ssim_load(const SsimTile& t, int p, SsimStage<R>& st) {
    if (p < 0 || p >= t.H) return;                                          // (uniform)
    const size_t plane = (size_t)p * t.W * t.D;
#pragma unroll
    for (int j = 0; j < SsimStage<R>::N; ++j) {
        const bool in = st.off[j] >= 0;
        const size_t o = plane + (in ? st.off[j] : 0);
        st.xy[j] = f32x2{in ? t.X[o] : 0.0f, in ? t.Y[o] : 0.0f};
    }
}

// one input plane p, already in the registers of `st` -> v = the five moments at the thread's (w, d), filtered along D and W (zeros for a
// plane outside the volume); the loads of plane p + 1 are issued behind the first barrier and land during the two passes
template <int R>
__device__ __forceinline__ void ssim_plane(const SsimTile& t, int p, bool more, SsimStage<R>& st, const float (&g)[2 * R + 1], SsimLds<R>& lds, SsimMoments& v) {
    constexpr int WS = 2 * R + 1, RW = SSIM_TW + 2 * R, SP = SSIM_TD + 2 * R;
    const bool live = p >= 0 && p < t.H;                                    // (uniform)
    if (live) {
#pragma unroll
        for (int j = 0; j < SsimStage<R>::N; ++j) {
            const int i = t.tid + j * SSIM_THREADS;
            if (i < RW * SP) lds.in[i] = st.xy[j];
        }
        cvx_barrier();
    }
    if (more) ssim_load<R>(t, p + 1, st);
    v.mu = v.sq = f32x2{0.0f, 0.0f};
    v.xy = 0.0f;
    if (!live) return;
    for (int i = t.tid; i < RW * SSIM_TD; i += SSIM_THREADS) {
        const int r = i / SSIM_TD, c = i % SSIM_TD;
        const f32x2* px = lds.in + r * SP + c;
        SsimMoments a = {f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, 0.0f};
#pragma unroll
        for (int k = 0; k < WS; ++k) {
            const f32x2 xy = ld2(px + k);
            a.mu = fma2(g[k], xy, a.mu);
            a.sq = fma2(g[k], xy * xy, a.sq);
            a.xy = fmaf(g[k], xy.x * xy.y, a.xy);
        }
        lds.mu[i] = a.mu; lds.sq[i] = a.sq; lds.xy[i] = a.xy;
    }
    cvx_barrier();                                                          // (the next plane's D pass writes its rows behind ITS first barrier)
#pragma unroll
    for (int k = 0; k < WS; ++k) {
        const int i = (t.ty + k) * SSIM_TD + t.tx;
        v.mu = fma2(g[k], ld2(lds.mu + i), v.mu);
        v.sq = fma2(g[k], ld2(lds.sq + i), v.sq);
        v.xy = fmaf(g[k], lds.xy[i], v.xy);
    }
}

// the SSIM expression from the five filtered moments of output plane oh; adds the value to the thread's float64 column sum
__device__ __forceinline__ void ssim_emit(const SsimTile& t, int oh, const SsimMoments& o, double& dsum) {
    if (oh < t.h0 || !t.inside) return;                                     // (planes before the chunk only fill the ring)
    const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
    const float m11 = o.mu.x * o.mu.x, m22 = o.mu.y * o.mu.y, m12 = o.mu.x * o.mu.y;
    const float s1 = o.sq.x - m11, s2 = o.sq.y - m22, s12 = o.xy - m12;
    const float num = (2.0f * m12 + C1) * (2.0f * s12 + C2);
    const float den = (m11 + m22 + C1) * (s1 + s2 + C2);
    const float val = fdiv(num, den);
    if (t.map) t.map[((size_t)oh * t.W + (t.w0 + t.ty)) * t.D + (t.d0 + t.tx)] = val;
    dsum += (double)val;
}

// WS consecutive planes with the ring slot of each a compile-time constant (no register moves): plane p goes to slot S; slots
// S+1 .. S+WS (mod WS) then hold planes p - 2R .. p, so tap k meets plane p - 2R + k and the window of plane p - R is complete.
// Returns true when the chunk ended inside the group.
template <int R, int S>
__device__ __forceinline__ bool ssim_march(const SsimTile& t, int p, int pend, SsimStage<R>& st, SsimMoments (&ring)[2 * R + 1], const float (&g)[2 * R + 1],
                                           SsimLds<R>& lds, double& dsum) {
    constexpr int WS = 2 * R + 1;
    ssim_plane<R>(t, p, p + 1 < pend, st, g, lds, ring[S]);
    SsimMoments o = {f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, 0.0f};
#pragma unroll
    for (int k = 0; k < WS; ++k) {
        const SsimMoments& r = ring[(S + 1 + k) % WS];
        o.mu = fma2(g[k], r.mu, o.mu);
        o.sq = fma2(g[k], r.sq, o.sq);
        o.xy = fmaf(g[k], r.xy, o.xy);
    }
    ssim_emit(t, p - R, o, dsum);
    if (p + 1 >= pend) return true;
    if constexpr (S + 1 < WS) return ssim_march<R, S + 1>(t, p + 1, pend, st, ring, g, lds, dsum);
    return false;
}

// X, Y [NC][H][W][D]; grid = NC x nch x ntw x ntd workgroups (D tiles fastest); map and partial may be null
template <int R>
__global__ __launch_bounds__(SSIM_THREADS) void k_ssim3d(const float* __restrict__ X, const float* __restrict__ Y, int H, int W, int D, int ntw, int ntd,
                                                         int nch, int hlen, SsimTaps taps, float* __restrict__ map, double* __restrict__ partial) {
    constexpr int WS = 2 * R + 1;
    __shared__ SsimLds<R> lds;
    SsimTile t;
    t.tid = (int)threadIdx.x; t.tx = t.tid % SSIM_TD; t.ty = t.tid / SSIM_TD;
    int b = (int)blockIdx.x;
    t.d0 = (b % ntd) * SSIM_TD; b /= ntd;
    t.w0 = (b % ntw) * SSIM_TW; b /= ntw;
    t.h0 = (b % nch) * hlen;
    const size_t vol = (size_t)(b / nch) * H * W * D;
    const int h1 = t.h0 + hlen < H ? t.h0 + hlen : H;
    t.X = X + vol; t.Y = Y + vol; t.map = map ? map + vol : nullptr;
    t.H = H; t.W = W; t.D = D;
    t.inside = t.w0 + t.ty < W && t.d0 + t.tx < D;

    float g[WS];
#pragma unroll
    for (int k = 0; k < WS; ++k) g[k] = taps.g[k];
    SsimMoments ring[WS];
#pragma unroll
    for (int k = 0; k < WS; ++k) ring[k] = SsimMoments{f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, 0.0f};
    double dsum = 0.0;
    SsimStage<R> st;
    ssim_stage_init<R>(t, st);
    ssim_load<R>(t, t.h0 - R, st);
    for (int p = t.h0 - R; !ssim_march<R, 0>(t, p, h1 + R, st, ring, g, lds, dsum); p += WS) {}

    if (partial) {                                                          // (uniform)
        lds.red[t.tid] = dsum;                                              // a thread outside the volume holds +0
        cvx_barrier();
        if (t.ty == 0) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < SSIM_TW; ++j) s += lds.red[j * SSIM_TD + t.tx];
            partial[(size_t)blockIdx.x * SSIM_TD + t.tx] = s;
        }
    }
}

// block 0 (mean != null): the sum of all partials, thread t over entries t, t + 256, ... in order, then a fixed tree; the other blocks: one thread
// per (n, d) of the slice means, adding its D column's partials over (c, chunk, W tile) in index order
__global__ __launch_bounds__(SSIM_FIN_THREADS) void k_ssim_finish(const double* __restrict__ partial, int N, int C, int D, int ntw, int ntd, int nch,
                                                                  int64_t nwg, double count_all, double count_slice, float* __restrict__ mean,
                                                                  float* __restrict__ slice_mean) {
    __shared__ double sh[SSIM_FIN_THREADS];
    const int tid = (int)threadIdx.x;
    int blk = (int)blockIdx.x;
    if (mean) {
        if (blk == 0) {
            const int64_t n = nwg * SSIM_TD;
            double s = 0.0;
            for (int64_t i = tid; i < n; i += SSIM_FIN_THREADS) s += partial[i];
            sh[tid] = s;
            cvx_barrier();
            for (int step = SSIM_FIN_THREADS / 2; step > 0; step >>= 1) {
                if (tid < step) sh[tid] += sh[tid + step];
                cvx_barrier();
            }
            if (tid == 0) *mean = (float)(sh[0] / count_all);
            return;
        }
        --blk;
    }
    const int64_t i = (int64_t)blk * SSIM_FIN_THREADS + tid;
    if (i >= (int64_t)N * D) return;
    const int n = (int)(i / D), d = (int)(i % D), td = d / SSIM_TD, tx = d % SSIM_TD;
    double s = 0.0;
    for (int c = 0; c < C; ++c)
        for (int ch = 0; ch < nch; ++ch)
            for (int tw = 0; tw < ntw; ++tw) s += partial[(((((size_t)n * C + c) * nch + ch) * ntw + tw) * ntd + td) * SSIM_TD + tx];
    slice_mean[i] = (float)(s / count_slice);
}

template <int R>
static void ssim_launch(const SsimPlan& p, const float* x, const float* y, int H, int W, int D, const SsimTaps& taps, float* map, double* partial,
                        hipStream_t s) {
    hipLaunchKernelGGL(k_ssim3d<R>, dim3((unsigned)p.nwg), dim3(SSIM_THREADS), 0, s, x, y, H, W, D, p.ntw, p.ntd, p.nch, p.hlen, taps, map, partial);
}

// the 1-D window: exp(-k^2 / (2 sigma^2)), sigma = 1.5, in float64, normalised to sum 1, rounded to float32
static SsimTaps ssim_taps(int ws) {
    double e[SSIM_MAX_WS], sum = 0.0;
    for (int k = 0; k < ws; ++k) { const double t = (double)(k - ws / 2); e[k] = exp(-(t * t) / 4.5); sum += e[k]; }
    SsimTaps taps;
    for (int k = 0; k < SSIM_MAX_WS; ++k) taps.g[k] = k < ws ? (float)(e[k] / sum) : 0.0f;
    return taps;
}

// every refusal of the two entry points (0 = acceptable); `what` names the caller in the message
static int ssim_check(const char* what, int n, int c, int h, int w, int d, int ws) {
    CVX_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && d > 0, "%s: bad extent (%d, %d, %d, %d, %d)", what, n, c, h, w, d);
    CVX_REQUIRE(ws >= 1 && ws % 2 == 1, "%s: window_size %d must be odd and positive (an even window grows the reference's output by one voxel per axis)", what, ws);
    if (ws > SSIM_MAX_WS) return fail(CVX_ERR_UNSUPPORTED, "%s: window_size %d, at most %d supported (further taps weigh less than 1e-6)", what, ws, SSIM_MAX_WS);
    if ((int64_t)w * d > 0x7fffffff) return fail(CVX_ERR_UNSUPPORTED, "%s: a plane of more than 2^31 voxels", what);
    if (ssim_plan((int64_t)n * c, h, w, d).nwg > 0x7fffffff) return fail(CVX_ERR_UNSUPPORTED, "%s: more than 2^31 tiles", what);
    return CVX_OK;
}

}  // namespace cvx

using namespace cvx;

extern "C" size_t cvx_ssim3d_workspace_bytes(int n, int c, int h, int w, int d, int window_size) {
    if (ssim_check("cvx_ssim3d_workspace_bytes", n, c, h, w, d, window_size) != CVX_OK) return 0;
    Carver m;
    ssim_layout(m, (int64_t)n * c, ssim_plan((int64_t)n * c, h, w, d));
    return ws_query(m);
}

extern "C" int cvx_ssim3d_f32(const float* img1, const float* img2, int n, int c, int h, int w, int d, int window_size, float* map, float* mean,
                              float* slice_mean, void* workspace, size_t workspace_bytes, void* stream) {
    CVX_REQUIRE(img1 && img2, "cvx_ssim3d_f32: null input");
    CVX_REQUIRE(map || mean || slice_mean, "cvx_ssim3d_f32: no output requested (map, mean and slice_mean are all NULL)");
    const int rc = ssim_check("cvx_ssim3d_f32", n, c, h, w, d, window_size);
    if (rc != CVX_OK) return rc;
    const int64_t nc = (int64_t)n * c;
    const size_t bytes = (size_t)nc * h * w * d * sizeof(float);
    CVX_REQUIRE(!overlap_any(map, bytes, img1, bytes) && !overlap_any(map, bytes, img2, bytes), "cvx_ssim3d_f32: map overlaps an input (every voxel is read by its neighbours' windows)");
    const SsimPlan p = ssim_plan(nc, h, w, d);
    double* partial = nullptr;
    if (mean || slice_mean) {                                               // the map alone needs no workspace
        const size_t need = cvx_ssim3d_workspace_bytes(n, c, h, w, d, window_size);
        if (!workspace || workspace_bytes < need) return fail(CVX_ERR_WORKSPACE, "cvx_ssim3d_f32: workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, need);
        Carver cv(workspace);
        partial = ssim_layout(cv, nc, p).partial;
    }
    hipStream_t s = as_stream(stream);
    const SsimTaps taps = ssim_taps(window_size);
    switch (window_size / 2) {
        case 0: ssim_launch<0>(p, img1, img2, h, w, d, taps, map, partial, s); break;
        case 1: ssim_launch<1>(p, img1, img2, h, w, d, taps, map, partial, s); break;
        case 2: ssim_launch<2>(p, img1, img2, h, w, d, taps, map, partial, s); break;
        case 3: ssim_launch<3>(p, img1, img2, h, w, d, taps, map, partial, s); break;
        case 4: ssim_launch<4>(p, img1, img2, h, w, d, taps, map, partial, s); break;
        default: ssim_launch<5>(p, img1, img2, h, w, d, taps, map, partial, s); break;
    }
    int st = check_last("cvx_ssim3d_f32");
    if (st != CVX_OK || !partial) return st;
    const int64_t slice_blocks = slice_mean ? cdiv64((int64_t)n * d, SSIM_FIN_THREADS) : 0;
    hipLaunchKernelGGL(k_ssim_finish, dim3((unsigned)(slice_blocks + (mean ? 1 : 0))), dim3(SSIM_FIN_THREADS), 0, s, partial, n, c, d, p.ntw, p.ntd, p.nch, p.nwg,
                       (double)nc * h * w * d, (double)c * h * w, mean, slice_mean);
    return check_last("cvx_ssim3d_f32 (means)");
}
