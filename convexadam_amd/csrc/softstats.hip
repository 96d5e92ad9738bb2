// softstats.hip -- the soft reading of a cost volume (include/convexadam_soft.h): per coarse cell the Boltzmann-weighted mean
// displacement, its covariance, the partition sum and the mean excess energy.  The arithmetic and the order of every sum are
// csrc/softstats_core.h; this file only decides who computes which D-shift plane ("chunk") of which column.
//   k_soft_min    one thread per (cell, chunk): the NaN-keeping min of the chunk's n^2 energies -> workspace [n][V].  n V threads, every
//                 load coalesced ([K][V]: consecutive lanes, consecutive cells): the pass that streams the volume from HBM.
//   k_soft_sums   one workgroup per slab of 64 cells, NW = blockDim / 64 wavefronts (up to 8).  Every wavefront folds the n chunk minima
//                 of its lanes' cells into m; in round c0 = 0, NW, .. wavefront v takes chunk c0 + v and leaves its eleven float64 chunk
//                 sums per cell in LDS; after a barrier the workgroup's threads add the round's chunk sums in dD order to the running
//                 totals in LDS (11 x 64 independent chains, one thread each: a single owner per chain, no atomics).  Wavefront 0 then
//                 turns the totals into the twelve outputs and counts the non-finite columns: one ballot, one integer atomic add.
//                 NW = ceil(n / ceil(n / 8)): the rounds are as full as n allows (hw 6: 13 chunks, 7 wavefronts, two rounds; 45 KB of
//                 LDS and ~110 VGPRs, so two workgroups share a CU and the 481 slabs of the benchmark grid are resident at once).
//                 The second read of the slab (64 cells x K entries) comes out of the caches where they hold it.
// In both kernels the loads of a chunk go out eight entries ahead of their use (soft_walk_ahead), which is what keeps a wavefront's
// HBM requests in flight.
#include <hip/hip_fp16.h>

#include "cvx_common.h"
#include "geometry_args.h"
#include "convexadam_soft.h"

namespace cvx {
CVX_HD float soft_widen(__half h) { return __half2float(h); }          // exact, as soft_widen(soft_half) of the core
}  // namespace cvx

#include "softstats_core.h"

namespace cvx {

constexpr int SS_MIN_THREADS = 256;
constexpr int SS_SLAB = 64;                          // cells per workgroup of k_soft_sums: one per lane
constexpr int SS_MAX_WAVES = 8;                      // (8 + 1) x 11 x 64 doubles of LDS: below the 64 KiB that need no opt-in
constexpr int SS_ITEMS = SOFT_SUMS * SS_SLAB;        // sums x cells: the chains of a slab
constexpr int SS_BATCH = 8;

// workspace: the chunk minima [n][V] -- ONE layout for the size query and the launcher
struct SoftWs { float* cmin; };
static SoftWs soft_layout(Carver& c, size_t V, int n) {
    SoftWs w;
    w.cmin = c.take<float>((size_t)n * V);
    return w;
}
static int soft_waves(int n) { return cdiv(n, cdiv(n, SS_MAX_WAVES)); }

template <typename T, bool FIELD>
__device__ __forceinline__ SoftColumn<T> soft_column_of(const T* ssd, const float* field, float coupling, int V, int hw, int x) {
    SoftColumn<T> col;
    col.ssd = ssd + x;
    col.V = (size_t)V;
    col.hw = hw;
    col.has_field = FIELD;
    col.coupling = coupling;
    col.u0 = FIELD ? field[x] : 0.0f;
    col.u1 = FIELD ? field[(size_t)V + x] : 0.0f;
    col.u2 = FIELD ? field[2 * (size_t)V + x] : 0.0f;
    return col;
}

// The entries of chunk c in k order, the loads SS_BATCH entries ahead of their use (two register batches): f(energy, dH, dW, dD) sees what
// the loops of soft_chunk_min / soft_chunk_sums of the core see, in the same order.  A thread that waited for every load before it asked
// for the next had one request in flight: k_soft_min then took 91 us for 270 MB.
template <typename T, typename F>
__device__ __forceinline__ void soft_walk_ahead(const SoftColumn<T>& col, int c, F&& f) {
    const int hw = col.hw, n = 2 * hw + 1, nn = n * n, dD = c - hw;
    const T* p = col.ssd + (size_t)c * nn * col.V;
    T cur[SS_BATCH], nxt[SS_BATCH];
#pragma unroll
    for (int u = 0; u < SS_BATCH; ++u)
        if (u < nn) cur[u] = p[(size_t)u * col.V];
    int dH = -hw, dW = -hw;
    for (int j = 0; j < nn; j += SS_BATCH) {
#pragma unroll
        for (int u = 0; u < SS_BATCH; ++u)
            if (j + SS_BATCH + u < nn) nxt[u] = p[(size_t)(j + SS_BATCH + u) * col.V];
#pragma unroll
        for (int u = 0; u < SS_BATCH; ++u)
            if (j + u < nn) {
                f(col.energy(cur[u], dH, dW, dD), dH, dW, dD);
                if (++dH > hw) dH = -hw, ++dW;
                __builtin_amdgcn_sched_barrier(0);   // one entry after the other: interleaving all eight exponentials costs 128 VGPRs and spills
            }
#pragma unroll
        for (int u = 0; u < SS_BATCH; ++u) cur[u] = nxt[u];
    }
}

template <typename T, bool FIELD>
__global__ __launch_bounds__(SS_MIN_THREADS) void k_soft_min(const T* __restrict__ ssd, const float* __restrict__ field, float coupling, int V, int hw,
                                                             float* __restrict__ cmin) {
    const int x = blockIdx.x * SS_MIN_THREADS + threadIdx.x, c = blockIdx.y;
    if (x >= V) return;
    const SoftColumn<T> col = soft_column_of<T, FIELD>(ssd, field, coupling, V, hw, x);
    float m = INFINITY;                              // soft_chunk_min of the core
    soft_walk_ahead(col, c, [&](float e, int, int, int) { m = soft_min(e, m); });
    cmin[(size_t)c * V + x] = m;
}

// soft_chunk_sums of the core
template <typename T>
__device__ __forceinline__ void soft_chunk_sums_ahead(const SoftColumn<T>& col, int c, float m, float beta, double (&s)[SOFT_SUMS]) {
#pragma unroll
    for (int i = 0; i < SOFT_SUMS; ++i) s[i] = 0.0;
    soft_walk_ahead(col, c, [&](float e, int dH, int dW, int dD) { soft_add(s, e, m, beta, dH, dW, dD); });
}

template <typename T, bool FIELD>
__global__ __launch_bounds__(SS_MAX_WAVES * 64) void k_soft_sums(const T* __restrict__ ssd, const float* __restrict__ field, float coupling, float beta,
                                                                 int V, int hw, const float* __restrict__ cmin, float* __restrict__ out,
                                                                 unsigned long long* __restrict__ stats) {
    extern __shared__ double ss_lds[];               // part [NW][11][64], then tot [11][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, NW = nthreads >> 6;
    const int n = 2 * hw + 1;
    const int x = blockIdx.x * SS_SLAB + lane;
    const bool active = x < V;
    double* part = ss_lds;
    double* tot = ss_lds + (size_t)NW * SS_ITEMS;
    for (int i = tid; i < SS_ITEMS; i += nthreads) tot[i] = 0.0;
    float m = INFINITY;
    SoftColumn<T> col = {};
    if (active) {
        for (int c = 0; c < n; ++c) m = soft_min(cmin[(size_t)c * V + x], m);
        col = soft_column_of<T, FIELD>(ssd, field, coupling, V, hw, x);
    }
    for (int c0 = 0; c0 < n; c0 += NW) {
        const int c = c0 + wave;
        if (c < n) {
            double s[SOFT_SUMS];
            if (active) soft_chunk_sums_ahead(col, c, m, beta, s);
            else {
#pragma unroll
                for (int i = 0; i < SOFT_SUMS; ++i) s[i] = 0.0;
            }
#pragma unroll
            for (int i = 0; i < SOFT_SUMS; ++i) part[(wave * SOFT_SUMS + i) * SS_SLAB + lane] = s[i];
        }
        cvx_barrier();
        const int live = min(NW, n - c0);            // the round's chunks, in dD order
        for (int item = tid; item < SS_ITEMS; item += nthreads) {
            double a = tot[item];
            for (int v = 0; v < live; ++v) a += part[v * SS_ITEMS + item];
            tot[item] = a;
        }
        cvx_barrier();
    }
    if (wave != 0) return;
    double s[SOFT_SUMS];
#pragma unroll
    for (int i = 0; i < SOFT_SUMS; ++i) s[i] = tot[i * SS_SLAB + lane];
    float o[SOFT_CHANNELS];
    const bool bad = soft_finish(s, m, o) && active;
    if (active) {
#pragma unroll
        for (int i = 0; i < SOFT_CHANNELS; ++i) out[(size_t)i * V + x] = o[i];
    }
    const unsigned long long votes = __ballot(bad);
    if (lane == 0 && votes) atomicAdd(stats, (unsigned long long)__popcll(votes));
}

template <typename T, bool FIELD>
static void launch_soft(const void* ssd, const float* field, float coupling, float beta, int V, int hw, const SoftWs& ws, float* out, int64_t* stats,
                        hipStream_t s) {
    const int n = 2 * hw + 1, NW = soft_waves(n);
    const size_t lds = (size_t)(NW + 1) * SS_ITEMS * sizeof(double);
    static_assert((SS_MAX_WAVES + 1) * SS_ITEMS * sizeof(double) <= 64 * 1024, "k_soft_sums: dynamic LDS beyond 64 KiB needs an opt-in");
    k_soft_min<T, FIELD><<<dim3(cdiv(V, SS_MIN_THREADS), n), SS_MIN_THREADS, 0, s>>>((const T*)ssd, field, coupling, V, hw, ws.cmin);
    k_soft_sums<T, FIELD><<<cdiv(V, SS_SLAB), NW * 64, lds, s>>>((const T*)ssd, field, coupling, beta, V, hw, ws.cmin, out,
                                                                 reinterpret_cast<unsigned long long*>(stats));
}

}  // namespace cvx

using namespace cvx;

extern "C" size_t cvx_soft_stats_workspace_bytes(int h, int w, int d, int hw) {
    const size_t V = voxels(h, w, d);
    if (!V || hw < 0 || hw > 15) return 0;
    const int n = 2 * hw + 1;
    if ((uint64_t)n * n * n * V >= ((uint64_t)1 << 31)) return 0;
    Carver measure;
    soft_layout(measure, V, n);
    return ws_query(measure);
}

extern "C" int cvx_soft_stats_f32(const void* ssd, int ssd_is_half, const float* field, float coupling, float beta, int h, int w, int d, int hw,
                                  float* out, int64_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
    CVX_REQUIRE(ssd && out && stats, "cvx_soft_stats_f32: null pointer");
    CVX_REQUIRE(h > 0 && w > 0 && d > 0, "cvx_soft_stats_f32: bad extent (%dx%dx%d)", h, w, d);
    CVX_REQUIRE(hw >= 0 && hw <= 15, "cvx_soft_stats_f32: hw %d outside 0 .. 15", hw);
    const size_t V = voxels(h, w, d);
    const int n = 2 * hw + 1;
    const uint64_t K = (uint64_t)n * n * n;
    CVX_REQUIRE(V && K * V < ((uint64_t)1 << 31), "cvx_soft_stats_f32: K * V = %d x (%dx%dx%d) reaches 2^31", (int)K, h, w, d);
    CVX_REQUIRE(isfinite(beta) && beta > 0.0f, "cvx_soft_stats_f32: beta must be finite and > 0 (got %g)", (double)beta);
    CVX_REQUIRE(isfinite(coupling) && coupling >= 0.0f, "cvx_soft_stats_f32: coupling must be finite and >= 0 (got %g)", (double)coupling);
    CVX_REQUIRE(field || coupling == 0.0f, "cvx_soft_stats_f32: a coupling of %g needs a field", (double)coupling);
    const size_t esz = ssd_is_half ? 2 : 4;
    CVX_REQUIRE(((uintptr_t)ssd & (esz - 1)) == 0 && ((uintptr_t)field & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)stats & 7) == 0 &&
                    ((uintptr_t)workspace & 7) == 0,
                "cvx_soft_stats_f32: a buffer is not aligned to its element");
    const size_t need = cvx_soft_stats_workspace_bytes(h, w, d, hw);
    const Span ins[2] = {{ssd, (size_t)K * V * esz}, {field, field ? 3 * V * 4 : 0}};
    const Span outs[3] = {{out, (size_t)SOFT_CHANNELS * V * 4}, {stats, 8}, {workspace, need}};
    static const char* const names[3] = {"out", "stats", "the workspace"};
    const Overlaps ov = find_overlaps(outs, ins);
    CVX_REQUIRE(ov.out < 0, "cvx_soft_stats_f32: %s overlaps an input", names[ov.out < 0 ? 0 : ov.out]);
    CVX_REQUIRE(ov.a < 0, "cvx_soft_stats_f32: %s overlaps %s", names[ov.a < 0 ? 0 : ov.a], names[ov.b < 0 ? 0 : ov.b]);
    CVX_REQUIRE(workspace && workspace_bytes >= need, "cvx_soft_stats_f32: workspace too small (%zu bytes, %zu needed)", workspace ? workspace_bytes : (size_t)0,
                need);
    hipStream_t s = as_stream(stream);
    Carver carve(workspace);
    const SoftWs ws = soft_layout(carve, V, n);
    if (hipMemsetAsync(stats, 0, 8, s) != hipSuccess) return check_last("soft_stats (counter)");
    if (ssd_is_half) {
        if (field) launch_soft<__half, true>(ssd, field, coupling, beta, (int)V, hw, ws, out, stats, s);
        else launch_soft<__half, false>(ssd, field, coupling, beta, (int)V, hw, ws, out, stats, s);
    } else {
        if (field) launch_soft<float, true>(ssd, field, coupling, beta, (int)V, hw, ws, out, stats, s);
        else launch_soft<float, false>(ssd, field, coupling, beta, (int)V, hw, ws, out, stats, s);
    }
    return check_last("soft_stats");
}
