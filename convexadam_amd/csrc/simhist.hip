// simhist.hip -- value range and joint histogram of an image pair, the moving image optionally warped inside the same pass
// (include/convexadam_sim.h).  The arithmetic of a voxel is csrc/simhist_core.h; this file only decides who takes which voxel
// and where a count is added.  Integer atomics only, so every split gives the same bytes.
//   k_sim_range        grid-stride pass, one voxel per lane and step: the keys of the kept values are folded per lane, per wavefront
//                      (shuffles) and per workgroup (LDS), then by at most one atomicMin per slot and workgroup into the four slots that
//                      live in range_out itself
//   k_sim_range_done   one thread turns the four slots into floats in place
//   k_joint_hist       the same pass; a kept voxel's cell goes to sim_count():
//                        LDS     bins_a bins_b 4 <= 64 KiB: uint32 copies of the histogram in LDS, wavefront w counts in copy w % copies
//                                (sim_plan: as many copies as fit 32 KiB, at most one per wavefront); after the pass the workgroup adds
//                                the copies and flushes the non-zero bins to the int64 histogram, one atomicAdd each
//                        global  otherwise: the same adds, straight into the int64 histogram
//                      Before the lanes of a wave-instruction add, the cell of the first live lane is broadcast, the lanes that hold the
//                      same cell are balloted away and ONE lane adds their number -- twice, then the rest add individually.  On a pair
//                      with a zero background (one cell holds two thirds of the voxels) almost every wave-instruction ends after the
//                      first round with a single LDS add instead of 64 serialised ones on one word.
// The grid is the resident workgroups (occupancy query x compute units), never more than the volume needs.
#include <type_traits>

#include "cvx_common.h"
#include "geometry_args.h"
#include "convexadam_sim.h"
#include "simhist_core.h"

namespace cvx {

constexpr int SIM_THREADS = 256;
constexpr int SIM_WAVES = SIM_THREADS / 64;
constexpr int SIM_LDS_LIMIT = 64 * 1024;          // the dynamic LDS a launch gets without an opt-in
constexpr int SIM_LDS_TARGET = 32 * 1024;         // copies beyond this would cost residency (160 KiB per compute unit)
constexpr int SIM_PEEL = 2;
constexpr int SIM_RED = 8;                        // words per wavefront in the workgroup's reduction of the counters (SIM_STATS of them used)

// WHERE the counts of a call go -- the one place the launcher and cvx_joint_hist_lds_bytes read
struct SimPlan { bool lds; int copies; size_t lds_bytes; };
static SimPlan sim_plan(int bins_a, int bins_b) {
    const size_t one = (size_t)bins_a * bins_b * sizeof(unsigned);
    SimPlan p = {one <= (size_t)SIM_LDS_LIMIT, 0, 0};
    if (p.lds) {
        const int fit = (int)((size_t)SIM_LDS_TARGET / one);
        p.copies = fit < 1 ? 1 : (fit > SIM_WAVES ? SIM_WAVES : fit);
        p.lds_bytes = (size_t)p.copies * one;
    }
    return p;
}

__device__ __forceinline__ void sim_add(unsigned* p, unsigned n) { atomicAdd(p, n); }
__device__ __forceinline__ void sim_add(unsigned long long* p, unsigned n) { atomicAdd(p, (unsigned long long)n); }

// one wave-instruction's cells (cell < 0: the lane has none) added to `bins`
template <typename T>
__device__ __forceinline__ void sim_count(int cell, T* bins, int lane) {
    bool live = cell >= 0;
#pragma unroll
    for (int r = 0; r < SIM_PEEL; ++r) {
        const unsigned long long act = __ballot(live);
        if (!act) return;
        const int leader = __builtin_ctzll(act);
        const int c0 = __shfl(cell, leader, 64);
        const unsigned long long same = __ballot(live && cell == c0);
        if (lane == leader) sim_add(bins + c0, (unsigned)__popcll(same));
        live = live && cell != c0;
    }
    if (live) sim_add(bins + cell, 1u);
}

__device__ __forceinline__ unsigned sim_wave_sum(unsigned x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ unsigned sim_wave_min(unsigned x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned y = __shfl_xor(x, o, 64);
        x = y < x ? y : x;
    }
    return x;
}
// The per-lane class counts of a pass -> stats: wavefront sums (shuffles), the workgroup's sum through `red` in LDS, then ONE atomicAdd per
// non-zero counter and workgroup.  Adds to one address serialise in the L2 at about 10 ns each: with one add per counter and WAVEFRONT
// the 8192 wavefronts of a full grid spent 80 us on the kept counter alone, and the range pass, with its four slots on top, 0.39 ms.
// Every thread of the workgroup arrives: the loops' trip counts are workgroup-uniform and nothing returns early.
__device__ __forceinline__ void sim_flush_stats(unsigned (&n)[SIM_STATS], unsigned long long* __restrict__ stats, unsigned* __restrict__ red, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < SIM_STATS; ++i) {
        const unsigned s = sim_wave_sum(n[i]);
        if (lane == 0) red[wave * SIM_RED + i] = s;
    }
    cvx_barrier();
    if (tid < SIM_STATS) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < SIM_WAVES; ++w) s += red[w * SIM_RED + tid];
        if (s) atomicAdd(stats + tid, (unsigned long long)s);
    }
}

template <typename TU, bool FIELD>
__global__ __launch_bounds__(SIM_THREADS) void k_sim_range(const float* __restrict__ fixed, const float* __restrict__ moving, const TU* __restrict__ u,
                                                           size_t cs, size_t vs, const unsigned char* __restrict__ mask, int H, int W, int D, int drop_outside,
                                                           unsigned* __restrict__ slots, unsigned long long* __restrict__ stats) {
    __shared__ unsigned red[SIM_WAVES * SIM_RED];    // per wavefront: the class counts, afterwards the slots
    const long long V = (long long)H * W * D, stride = (long long)gridDim.x * SIM_THREADS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned n[SIM_STATS] = {0, 0, 0, 0, 0};
    unsigned slot[4] = {SIM_SLOT_EMPTY, SIM_SLOT_EMPTY, SIM_SLOT_EMPTY, SIM_SLOT_EMPTY};
    for (long long base = (long long)blockIdx.x * SIM_THREADS; base < V; base += stride) {
        const long long q = base + threadIdx.x;
        if (q >= V) continue;
        float a, b;
        const int cls = sim_sample(fixed, moving, FIELD ? u : (const TU*)nullptr, cs, vs, mask, H, W, D, (size_t)q, drop_outside, a, b);
#pragma unroll
        for (int i = 0; i < 4; ++i) n[i] += cls == i;
        if (cls != SIM_KEPT) continue;
        const unsigned ka = sim_key(a), kb = sim_key(b);
        slot[0] = ka < slot[0] ? ka : slot[0];
        slot[1] = ~ka < slot[1] ? ~ka : slot[1];
        slot[2] = kb < slot[2] ? kb : slot[2];
        slot[3] = ~kb < slot[3] ? ~kb : slot[3];
    }
    sim_flush_stats(n, stats, red, tid);
    cvx_barrier();                                   // the counts have been read: red is free for the slots
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned m = sim_wave_min(slot[i]);
        if (lane == 0) red[wave * SIM_RED + i] = m;
    }
    cvx_barrier();
    if (tid < 4) {
        unsigned m = SIM_SLOT_EMPTY;
#pragma unroll
        for (int w = 0; w < SIM_WAVES; ++w) m = red[w * SIM_RED + tid] < m ? red[w * SIM_RED + tid] : m;
        // a slot only ever decreases, so a stale look at it can cost an atomic that changes nothing but never loses a minimum: most
        // workgroups find a smaller value there already and add no traffic to the slot's address
        if (m < __hip_atomic_load(slots + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slots + tid, m);
    }
}

__global__ void k_sim_range_done(unsigned* __restrict__ slots) {
    if (blockIdx.x || threadIdx.x) return;
    const unsigned s0 = slots[0], s1 = slots[1], s2 = slots[2], s3 = slots[3];
    float* out = reinterpret_cast<float*>(slots);
    out[0] = sim_slot_lo(s0);
    out[1] = sim_slot_hi(s1);
    out[2] = sim_slot_lo(s2);
    out[3] = sim_slot_hi(s3);
}

template <typename TU, bool FIELD, bool LDS>
__global__ __launch_bounds__(SIM_THREADS) void k_joint_hist(const float* __restrict__ fixed, const float* __restrict__ moving, const TU* __restrict__ u,
                                                            size_t cs, size_t vs, const unsigned char* __restrict__ mask, int H, int W, int D, int bins_a,
                                                            int bins_b, const float* __restrict__ range, int drop_outside, int copies,
                                                            unsigned long long* __restrict__ hist, unsigned long long* __restrict__ stats) {
    extern __shared__ unsigned sim_lds[];             // [copies][bins_a * bins_b]; at the end, SIM_WAVES * SIM_RED words for the counters
    const int nb = bins_a * bins_b, tid = threadIdx.x, lane = tid & 63;
    if (LDS) {
        for (int i = tid; i < copies * nb; i += SIM_THREADS) sim_lds[i] = 0u;
        cvx_barrier();
    }
    unsigned* mine = sim_lds + (size_t)((tid >> 6) % (LDS ? copies : 1)) * nb;
    const SimBins g = sim_bins(range, bins_a, bins_b);
    const long long V = (long long)H * W * D, stride = (long long)gridDim.x * SIM_THREADS;
    unsigned n[SIM_STATS] = {0, 0, 0, 0, 0};
    for (long long base = (long long)blockIdx.x * SIM_THREADS; base < V; base += stride) {
        const long long q = base + tid;
        int cell = -1;
        if (q < V) {
            float a, b;
            const int cls = sim_sample(fixed, moving, FIELD ? u : (const TU*)nullptr, cs, vs, mask, H, W, D, (size_t)q, drop_outside, a, b);
#pragma unroll
            for (int i = 0; i < 4; ++i) n[i] += cls == i;
            if (cls == SIM_KEPT) {
                bool clamped;
                cell = sim_cell(g, a, b, clamped);
                n[SIM_CLAMPED] += clamped;
            }
        }
        if (LDS) sim_count(cell, mine, lane);
        else sim_count(cell, hist, lane);
    }
    if (LDS) {
        cvx_barrier();
        for (int i = tid; i < nb; i += SIM_THREADS) {
            unsigned s = 0;
            for (int c = 0; c < copies; ++c) s += sim_lds[c * nb + i];
            if (s) atomicAdd(hist + i, (unsigned long long)s);
        }
        cvx_barrier();                               // the copies have been read: their LDS is free for the counters
    }
    sim_flush_stats(n, stats, sim_lds, tid);
}

static int sim_compute_units() {
    static const int cus = [] { int dev = 0, n = 0; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); (void)hipGetLastError(); return n; }();
    return cus > 0 ? cus : 256;
}
// workgroups of `kernel` that are resident at once, capped by what the volume needs
template <typename K>
static unsigned sim_grid(K kernel, size_t lds_bytes, size_t V) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, SIM_THREADS, lds_bytes) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 2;
    }
    const size_t resident = (size_t)per_cu * sim_compute_units(), need = (V + SIM_THREADS - 1) / SIM_THREADS;
    return (unsigned)(need < resident ? need : resident);
}

struct SimArgs {
    const float *fixed, *moving; FieldArg u; const unsigned char* mask; int H, W, D, drop_outside; size_t V;
};

template <typename TU, bool FIELD>
static void launch_range(const SimArgs& a, float* range_out, int64_t* stats, hipStream_t s) {
    auto k = k_sim_range<TU, FIELD>;
    hipLaunchKernelGGL(k, dim3(sim_grid(k, 0, a.V)), dim3(SIM_THREADS), 0, s, a.fixed, a.moving, static_cast<const TU*>(a.u.p), (size_t)a.u.cs, (size_t)a.u.vs,
                       a.mask, a.H, a.W, a.D, a.drop_outside, reinterpret_cast<unsigned*>(range_out), reinterpret_cast<unsigned long long*>(stats));
    hipLaunchKernelGGL(k_sim_range_done, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned*>(range_out));
}

template <typename TU, bool FIELD, bool LDS>
static void launch_hist(const SimArgs& a, int bins_a, int bins_b, const SimPlan& plan, const float* range, int64_t* hist, int64_t* stats, hipStream_t s) {
    auto k = k_joint_hist<TU, FIELD, LDS>;
    // (a static array beside 64 KiB of dynamic LDS would need the opt-in: the counters' reduction reuses the dynamic bytes, at least its own size)
    const size_t red = SIM_WAVES * SIM_RED * sizeof(unsigned), lds = plan.lds_bytes > red ? plan.lds_bytes : red;
    static_assert(SIM_STATS <= SIM_RED, "the reduction holds every counter");
    hipLaunchKernelGGL(k, dim3(sim_grid(k, lds, a.V)), dim3(SIM_THREADS), lds, s, a.fixed, a.moving, static_cast<const TU*>(a.u.p),
                       (size_t)a.u.cs, (size_t)a.u.vs, a.mask, a.H, a.W, a.D, bins_a, bins_b, range, a.drop_outside, plan.copies,
                       reinterpret_cast<unsigned long long*>(hist), reinterpret_cast<unsigned long long*>(stats));
}

// f(element type tag, has-field tag) for the field operand of a call
template <class F>
static void with_field(const FieldArg& u, F&& f) {
    if (!u.p) f(float{}, std::false_type{});
    else with_real(u.f64, [&](auto t) { f(t, std::true_type{}); });
}

}  // namespace cvx

using namespace cvx;

// the checks both launching entry points share; the outputs' overlaps are the caller's
#define SIM_REQUIRE_COMMON(NAME)                                                                                                                      \
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, NAME ": bad extent (%dx%dx%d)", H, W, D);                                                                    \
    const size_t V = voxels(H, W, D);                                                                                                                 \
    CVX_REQUIRE(V, NAME ": H W D = %dx%dx%d reaches 2^31", H, W, D);                                                                                  \
    const FieldArg fu = {field, field_f64 != 0, field ? field_comp_stride : 1, field ? field_voxel_stride : 3};                                        \
    CVX_REQUIRE(fu.strides_ok(V), NAME ": bad field strides (component %lld, voxel %lld)", (long long)field_comp_stride, (long long)field_voxel_stride)

extern "C" int cvx_joint_hist_lds_bytes(int bins_a, int bins_b) {
    if (bins_a < SIM_MIN_BINS || bins_a > SIM_MAX_BINS || bins_b < SIM_MIN_BINS || bins_b > SIM_MAX_BINS) return -1;
    return (int)sim_plan(bins_a, bins_b).lds_bytes;
}

extern "C" int cvx_sim_range_f32(const float* fixed, const float* moving, const void* field, int field_f64, int64_t field_comp_stride,
                                 int64_t field_voxel_stride, const unsigned char* mask, int H, int W, int D, int drop_outside, float* range_out,
                                 int64_t* stats, void* stream) {
    CVX_REQUIRE(fixed && moving && range_out && stats, "cvx_sim_range_f32: null pointer");
    SIM_REQUIRE_COMMON("cvx_sim_range_f32");
    CVX_REQUIRE(((uintptr_t)fixed & 3) == 0 && ((uintptr_t)moving & 3) == 0 && fu.aligned() && ((uintptr_t)range_out & 3) == 0 && ((uintptr_t)stats & 7) == 0,
                "cvx_sim_range_f32: a buffer is not aligned to its element");
    const Span ins[4] = {{fixed, V * 4}, {moving, V * 4}, fu.span(V), {mask, mask ? V : 0}};
    const Span outs[2] = {{range_out, 16}, {stats, SIM_STATS * 8}};
    static const char* const names[2] = {"range_out", "stats"};
    const Overlaps ov = find_overlaps(outs, ins);
    CVX_REQUIRE(ov.out < 0, "cvx_sim_range_f32: %s overlaps an input", names[ov.out < 0 ? 0 : ov.out]);
    CVX_REQUIRE(ov.a < 0, "cvx_sim_range_f32: %s overlaps %s", names[ov.a < 0 ? 0 : ov.a], names[ov.b < 0 ? 0 : ov.b]);
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(range_out, 0xff, 16, s) != hipSuccess || hipMemsetAsync(stats, 0, SIM_STATS * 8, s) != hipSuccess) return check_last("sim_range (reset)");
    const SimArgs a = {fixed, moving, fu, mask, H, W, D, drop_outside != 0, V};
    with_field(fu, [&](auto t, auto has) { launch_range<decltype(t), decltype(has)::value>(a, range_out, stats, s); });
    return check_last("sim_range");
}

extern "C" int cvx_joint_hist_f32(const float* fixed, const float* moving, const void* field, int field_f64, int64_t field_comp_stride,
                                  int64_t field_voxel_stride, const unsigned char* mask, int H, int W, int D, int bins_a, int bins_b, const float* range,
                                  int drop_outside, int64_t* hist, int64_t* stats, void* stream) {
    CVX_REQUIRE(fixed && moving && range && hist && stats, "cvx_joint_hist_f32: null pointer");
    SIM_REQUIRE_COMMON("cvx_joint_hist_f32");
    CVX_REQUIRE(bins_a >= SIM_MIN_BINS && bins_a <= SIM_MAX_BINS && bins_b >= SIM_MIN_BINS && bins_b <= SIM_MAX_BINS,
                "cvx_joint_hist_f32: bins %d x %d outside %d .. %d", bins_a, bins_b, (int)SIM_MIN_BINS, (int)SIM_MAX_BINS);
    CVX_REQUIRE(((uintptr_t)fixed & 3) == 0 && ((uintptr_t)moving & 3) == 0 && fu.aligned() && ((uintptr_t)range & 3) == 0 && ((uintptr_t)hist & 7) == 0 &&
                    ((uintptr_t)stats & 7) == 0,
                "cvx_joint_hist_f32: a buffer is not aligned to its element");
    const size_t hist_bytes = (size_t)bins_a * bins_b * 8;
    const Span ins[5] = {{fixed, V * 4}, {moving, V * 4}, fu.span(V), {mask, mask ? V : 0}, {range, 16}};
    const Span outs[2] = {{hist, hist_bytes}, {stats, SIM_STATS * 8}};
    static const char* const names[2] = {"hist", "stats"};
    const Overlaps ov = find_overlaps(outs, ins);
    CVX_REQUIRE(ov.out < 0, "cvx_joint_hist_f32: %s overlaps an input", names[ov.out < 0 ? 0 : ov.out]);
    CVX_REQUIRE(ov.a < 0, "cvx_joint_hist_f32: %s overlaps %s", names[ov.a < 0 ? 0 : ov.a], names[ov.b < 0 ? 0 : ov.b]);
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(hist, 0, hist_bytes, s) != hipSuccess || hipMemsetAsync(stats, 0, SIM_STATS * 8, s) != hipSuccess) return check_last("joint_hist (reset)");
    const SimArgs a = {fixed, moving, fu, mask, H, W, D, drop_outside != 0, V};
    const SimPlan plan = sim_plan(bins_a, bins_b);
    with_field(fu, [&](auto t, auto has) {
        if (plan.lds) launch_hist<decltype(t), decltype(has)::value, true>(a, bins_a, bins_b, plan, range, hist, stats, s);
        else launch_hist<decltype(t), decltype(has)::value, false>(a, bins_a, bins_b, plan, range, hist, stats, s);
    });
    return check_last("joint_hist");
}
