// pipeline.hip -- one registration of an image pair, end to end on one stream
// (reference: convex_adam_pt, src/convexAdam/convex_adam_MIND.py:64-202; multi-channel variant
// convex_adam_nnUNet.py:41-159).  Every stage is one of the C-ABI operators; nothing touches the host
// between the upload of the two images and the finished displacement field.
#include <vector>

#include "cvx_common.h"
#include "mind_common.h"

namespace cvx {

// identity coordinate of F.affine_grid(align_corners=False) and the search mesh of
// convex_adam_MIND.py:127, built on the device with the same float ops as the host helpers
// (torch.linspace restated: start + step*i / end - step*(S-1-i), each a single fused rounding).
__device__ __forceinline__ float linspace_pm1_at(int S, int i) {
    if (S == 1) return -1.0f;
    const float step = fdiv(1.0f - (-1.0f), (float)(S - 1));
    return (i < S / 2) ? __builtin_fmaf(step, (float)i, -1.0f) : __builtin_fmaf(-step, (float)(S - 1 - i), 1.0f);
}
// all six identity tables of a pair in one launch: (extent, destination) x 6, one workgroup row per table
struct BaseTables { int S[6]; float* out[6]; };
__global__ void k_affine_bases(BaseTables t) {
    const int S = t.S[blockIdx.y];
    float* out = t.out[blockIdx.y];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; out && i < S; i += gridDim.x * blockDim.x)
        out[i] = fdiv(linspace_pm1_at(S, i) * (float)(S - 1), (float)S);
}
__global__ void k_disp_mesh(int hw, float* out) {
    const int n = 2 * hw + 1, K = n * n * n;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int c = k % n, b = (k / n) % n, a = k / (n * n);
    const float la = n == 1 ? 0.f : linspace_pm1_at(n, a), lb = n == 1 ? 0.f : linspace_pm1_at(n, b),
                lc = n == 1 ? 0.f : linspace_pm1_at(n, c);
    out[k] = lc * (float)hw;
    out[K + k] = lb * (float)hw;
    out[2 * K + k] = la * (float)hw;
}

// Everything of a pair that depends on nothing but its geometry, in ONE launch instead of seven (two table kernels, the two all-ones fills
// of the plain argmins' key buffers, the list counters of both coupled-convex solves, the zero Adam state): the identity tables, the
// search mesh, keys = ~0, counts = 0, m = v = 0.
struct PairSetup {
    BaseTables t;
    int hw; float* mesh;
    unsigned long long* keys[2]; size_t v;
    int* counts[2];
    float4* zero[2]; size_t nzero4;
};
__global__ __launch_bounds__(256) void k_pair_setup(PairSetup a) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (size_t)gridDim.x * blockDim.x;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int S = a.t.S[t];
        float* out = a.t.out[t];
        for (size_t i = gid; out && i < (size_t)S; i += gsz) out[i] = fdiv(linspace_pm1_at(S, (int)i) * (float)(S - 1), (float)S);
    }
    const int n = 2 * a.hw + 1, K = n * n * n;
    for (size_t k = gid; k < (size_t)K; k += gsz) {
        const int c = (int)k % n, b = ((int)k / n) % n, aa = (int)k / (n * n);
        const float la = n == 1 ? 0.f : linspace_pm1_at(n, aa), lb = n == 1 ? 0.f : linspace_pm1_at(n, b), lc = n == 1 ? 0.f : linspace_pm1_at(n, c);
        a.mesh[k] = lc * (float)a.hw;
        a.mesh[K + k] = lb * (float)a.hw;
        a.mesh[2 * K + k] = la * (float)a.hw;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (a.keys[q]) for (size_t x = gid; x < a.v; x += gsz) a.keys[q][x] = ~0ull;
        if (a.counts[q] && gid < 2) a.counts[q][gid] = 0;
        if (a.zero[q]) for (size_t i = gid; i < a.nzero4; i += gsz) a.zero[q][i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// (disp_soft / scale).flip(1)                                             convex_adam_MIND.py:134,139
// (both directions of a pair in one launch: blockIdx.y selects the field)
__global__ __launch_bounds__(256) void k_ic_prepare(const float* __restrict__ soft, const float* __restrict__ soft_rev, int h, int w, int d,
                                                    float* __restrict__ out, float* __restrict__ out_rev) {
    const size_t v = (size_t)h * w * d;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= v) return;
    if (blockIdx.y) { soft = soft_rev; out = out_rev; }
    const float sc[3] = {(float)(h - 1) / 2.0f, (float)(w - 1) / 2.0f, (float)(d - 1) / 2.0f};
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(size_t)c * v + p] = fdiv(soft[(size_t)(2 - c) * v + p], sc[2 - c]);
}
// disp_ice.flip(1) * scale * grid_sp                                        convex_adam_MIND.py:141
__global__ __launch_bounds__(256) void k_ic_finish(const float* __restrict__ ice, int h, int w, int d, float gs, float* __restrict__ out) {
    const size_t v = (size_t)h * w * d;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= v) return;
    const float sc[3] = {(float)(h - 1) / 2.0f, (float)(w - 1) / 2.0f, (float)(d - 1) / 2.0f};
#pragma unroll
    for (int a = 0; a < 3; ++a) out[(size_t)a * v + p] = (ice[(size_t)(2 - a) * v + p] * sc[a]) * gs;
}

struct PairLayout {
    // extents
    int H, W, D, h, w, d, h2, w2, d2, C, K;
    size_t V, v, V2;
    // byte offsets into the workspace (0 = not used)
    size_t featF, featM, mind_ws, mind_ws2, fs, ms, corr_ws, corr_ws2, ssd, argmin, mesh, conv_ws, ssd2, argmin2, conv_ws2, cert_ws, cert_ws2, soft, soft2, in1, in2, ic1, ic2, ic_ws,
        upin, disp_hr, F2, M2, P, m, v_, U, adam_ws, smooth_ws, smooth_ws2, snaps, bh, bw, bd, bh2, bw2, bd2, total;
};

static PairLayout pair_layout(const cvx_pair_params& p, int n_snap = 0, int max_smooth = 0) {
    PairLayout L{};
    L.H = p.H; L.W = p.W; L.D = p.D;
    L.h = p.H / p.grid_sp; L.w = p.W / p.grid_sp; L.d = p.D / p.grid_sp;
    L.h2 = p.H / p.grid_sp_adam; L.w2 = p.W / p.grid_sp_adam; L.d2 = p.D / p.grid_sp_adam;
    L.C = p.n_feat > 0 ? p.n_feat : 12;
    const int n = 2 * p.disp_hw + 1;
    L.K = n * n * n;
    L.V = (size_t)p.H * p.W * p.D; L.v = (size_t)L.h * L.w * L.d; L.V2 = (size_t)L.h2 * L.w2 * L.d2;
    Carver cv; cv.take_bytes(1);    // offset 0 is reserved as "unused"
    const size_t f = sizeof(float);
    if (p.n_feat == 0) {
        // (the pooled path's raw patch SSDs may be blocked by tiles that overhang the volume: MindPlan::raw_floats >= 12 V)
        const size_t raw_floats = mind_plan(MindUse{p.H, p.W, p.D, p.mind_r, p.mind_d, p.grid_sp, p.lambda_weight > 0 ? p.grid_sp_adam : 0, 0, true, true}).raw_floats;
        L.featF = cv.take_bytes(f * raw_floats);
        L.featM = cv.take_bytes(f * raw_floats);
        L.mind_ws = cv.take_bytes(cvx_mindssc_workspace_bytes(p.H, p.W, p.D, p.mind_r, p.mind_d));
        L.mind_ws2 = cv.take_bytes(cvx_mindssc_workspace_bytes(p.H, p.W, p.D, p.mind_r, p.mind_d));      // the moving image's pass runs beside the fixed one's
    }
    L.fs = cv.take_bytes(f * L.C * L.v);
    L.ms = cv.take_bytes(f * L.C * L.v);
    // ---- scratch of the convex stage alone: nothing in it is read once the coupled-convex solves are enqueued (PairRun::convex), so
    // the Adam loop's workspace, first touched after them on the same stream, lies over it (adam_ws below)
    const size_t convex_scratch = align_up(cv.used, 256);
    L.corr_ws = cv.take_bytes(cvx_correlate_workspace_bytes(L.C, L.h, L.w, L.d, p.disp_hw));
    // the reverse direction's padded copies (both directions in one launch): only where that path can run (option corr_dual, off by default)
    L.corr_ws2 = corr_plan(L.C, L.h, L.w, L.d, p.disp_hw, CorrUse{false, p.ic != 0, false}).pair_dual_ws ? cv.take_bytes(corr_fused_workspace_bytes(L.C, L.h, L.w, L.d, p.disp_hw)) : 0;
    // fp16 storage: the cost volumes hold __half (half the bytes written by the correlation kernel and read by every argmin pass)
    const size_t ssd_elem = p.fp16_storage ? 2 : f;
    L.ssd = cv.take_bytes(ssd_elem * (size_t)L.K * L.v);
    L.argmin = cv.take_bytes(sizeof(int64_t) * L.v);
    L.mesh = cv.take_bytes(f * 3 * (size_t)L.K);
    L.conv_ws = cv.take_bytes(cvx_coupled_convex_workspace_bytes(L.h, L.w, L.d, p.disp_hw));
    // certified decisions on the fast cost volume (certify.hip): one small workspace per direction
    L.cert_ws = cv.take_bytes(corr_certify_workspace_bytes(L.C, L.h, L.w, L.d, p.disp_hw));
    if (p.ic) {
        L.cert_ws2 = cv.take_bytes(corr_certify_workspace_bytes(L.C, L.h, L.w, L.d, p.disp_hw));
        // the reverse direction keeps its own cost volume: both coupled-convex solves share their launches
        L.ssd2 = cv.take_bytes(ssd_elem * (size_t)L.K * L.v);
        L.argmin2 = cv.take_bytes(sizeof(int64_t) * L.v);
        L.conv_ws2 = cv.take_bytes(cvx_coupled_convex_workspace_bytes(L.h, L.w, L.d, p.disp_hw));
    }
    if (p.lambda_weight > 0) {
        Carver over; over.used = convex_scratch;
        L.adam_ws = over.take_bytes(cvx_adam_workspace_bytes(L.C, L.h2, L.w2, L.d2));
        if (over.used > cv.used) cv.used = over.used;
    }
    // ---- what outlives the convex stage
    L.soft = cv.take_bytes(f * 3 * L.v);
    L.bh = cv.take_bytes(f * L.h); L.bw = cv.take_bytes(f * L.w); L.bd = cv.take_bytes(f * L.d);
    if (p.ic) {
        L.soft2 = cv.take_bytes(f * 3 * L.v);
        L.in1 = cv.take_bytes(f * 3 * L.v); L.in2 = cv.take_bytes(f * 3 * L.v);
        L.ic1 = cv.take_bytes(f * 3 * L.v); L.ic2 = cv.take_bytes(f * 3 * L.v);
        L.ic_ws = cv.take_bytes(cvx_inverse_consistency_workspace_bytes(L.h, L.w, L.d));
        L.upin = cv.take_bytes(f * 3 * L.v);
        L.disp_hr = cv.take_bytes(f * 3 * L.V);
    }
    if (p.lambda_weight > 0) {
        // planar pooled features, or (MIND path, option mind_records) the Adam loop's records: [CP/4][V2 + 1][4]
        const size_t f2_bytes = f * adam_record_floats(L.C, L.V2);
        L.F2 = cv.take_bytes(f2_bytes);
        L.M2 = cv.take_bytes(f2_bytes);
        L.P = cv.take_bytes(f * 3 * L.V2); L.m = cv.take_bytes(f * 3 * L.V2); L.v_ = cv.take_bytes(f * 3 * L.V2); L.U = cv.take_bytes(f * 3 * L.V2);
        L.bh2 = cv.take_bytes(f * L.h2); L.bw2 = cv.take_bytes(f * L.w2); L.bd2 = cv.take_bytes(f * L.d2);
        if (p.selected_smooth > 0 || max_smooth > 0) { L.smooth_ws = cv.take_bytes(f * 3 * L.V); L.smooth_ws2 = cv.take_bytes(f * 3 * L.V); }
        if (n_snap > 0) L.snaps = cv.take_bytes(f * 3 * L.V2 * (size_t)n_snap);
    }
    L.total = ws_query(cv);
    return L;
}

// ---- optional per-stage timing -------------------------------------------------------------------------
static thread_local int g_profiling = 0;       // 0 off, 1 last call only, 2 accumulate over calls, 3 = 2 + one mark per kernel of the Adam loop
struct StageMark { const char* name; hipEvent_t ev; };
static thread_local std::vector<StageMark> g_marks;
static thread_local std::vector<hipEvent_t> g_pool;
static thread_local size_t g_pool_used = 0;

static void mark(const char* name, hipStream_t s) {
    if (!g_profiling) return;
    if (g_pool_used == g_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        g_pool.push_back(e);
    }
    hipEvent_t e = g_pool[g_pool_used++];
    (void)hipEventRecord(e, s);
    g_marks.push_back({name, e});
}
// (adam.hip) one mark behind every kernel of the Adam loop when cvx_set_profiling(3) is on: per-kernel durations from events on the
// launch stream, the iteration's three launches named "adam.forward_boxes", "adam.warp_gradient", "adam.adjoint_update"
void profile_mark_kernel(const char* name, hipStream_t s) {
    if (g_profiling == 3) mark(name, s);
}

// ---- side stream for the independent half of a stage (the two images' descriptors) ---------------------------------------
// One per (thread, slot): slot = the internal stream index of cvx_register_pairs_f32 (0 for a single pair), so that concurrent pairs do
// not share a side stream.  Forks from / joins into the pair's stream with events; created once per thread and device.
struct SidePool {
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> fork, join;
    int device = -1;
};
static thread_local SidePool g_side;
static thread_local int g_side_slot = 0;
static bool side_stream(hipStream_t* side, hipEvent_t* fork, hipEvent_t* join) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    SidePool& P = g_side;
    if (P.device != dev) { P.streams.clear(); P.fork.clear(); P.join.clear(); P.device = dev; }        // leaked on device switch (rare)
    while ((int)P.streams.size() <= g_side_slot) {
        hipStream_t st; hipEvent_t a, b;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&a, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&b, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
        P.streams.push_back(st); P.fork.push_back(a); P.join.push_back(b);
    }
    *side = P.streams[g_side_slot]; *fork = P.fork[g_side_slot]; *join = P.join[g_side_slot];
    return true;
}

static int validate(const cvx_pair_params* p) {
    CVX_REQUIRE(p, "cvx_register_pair: null params");
    CVX_REQUIRE(p->H > 0 && p->W > 0 && p->D > 0, "cvx_register_pair: bad extent");
    CVX_REQUIRE(p->grid_sp >= 1 && p->grid_sp_adam >= 1, "cvx_register_pair: grid spacing must be >= 1");
    CVX_REQUIRE(p->H / p->grid_sp >= 2 && p->W / p->grid_sp >= 2 && p->D / p->grid_sp >= 2,
                "cvx_register_pair: volume too small for grid_sp %d", p->grid_sp);
    CVX_REQUIRE(p->disp_hw >= 0 && p->disp_hw <= CVX_MAX_DISP_HW, "cvx_register_pair: disp_hw %d not in 0..%d", p->disp_hw, CVX_MAX_DISP_HW);
    CVX_REQUIRE(p->n_feat >= 0 && p->n_feat < 256, "cvx_register_pair: n_feat out of range");
    CVX_REQUIRE(p->selected_smooth == 0 || (p->selected_smooth & 1), "cvx_register_pair: selected_smooth must be odd "
                "(an even kernel changes the volume size in the reference, convex_adam_MIND.py:185-191)");
    CVX_REQUIRE((p->cost == 0 || p->cost == 1) && (p->n_box == 0 || p->n_box == 1 || p->n_box == 2) &&
                (p->n_spline_pools == 0 || p->n_spline_pools == 2 || p->n_spline_pools == 3) && (p->corr_fast == 0 || p->corr_fast == 1) &&
                (p->fp16_storage == 0 || p->fp16_storage == 1), "cvx_register_pair: bad variant fields (cost, n_box, n_spline_pools, corr_fast, fp16_storage)");
    CVX_REQUIRE((p->adam_fast == 0 || p->adam_fast == 1 || p->adam_fast == 2) && p->reserved_[0] == 0 && p->reserved_[1] == 0 && p->reserved_[2] == 0,
                "cvx_register_pair: adam_fast must be 0, 1 or 2 and the reserved fields zero (struct laid out by an older header? check cvx_version())");
    CVX_REQUIRE(!p->adam_fast || p->n_spline_pools != 2, "cvx_register_pair: adam_fast needs the packaged smoother (three 3^3 boxes)");
    if (p->lambda_weight > 0) {
        CVX_REQUIRE(p->selected_niter >= 1, "cvx_register_pair: selected_niter must be >= 1 when lambda_weight > 0 "
                    "(the reference raises UnboundLocalError, convex_adam_MIND.py:181)");
        CVX_REQUIRE(p->H / p->grid_sp_adam >= 2 && p->W / p->grid_sp_adam >= 2 && p->D / p->grid_sp_adam >= 2,
                    "cvx_register_pair: volume too small for grid_sp_adam %d", p->grid_sp_adam);
    }
    return CVX_OK;
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_disp_mesh_f32(int disp_hw, float* out_device, void* stream) {
    CVX_REQUIRE(out_device && disp_hw >= 0 && disp_hw <= CVX_MAX_DISP_HW, "cvx_disp_mesh_f32: bad arguments (disp_hw 0 .. %d)", CVX_MAX_DISP_HW);
    const int n = 2 * disp_hw + 1, K = n * n * n;
    hipLaunchKernelGGL(k_disp_mesh, dim3(cdiv(K, 256)), dim3(256), 0, as_stream(stream), disp_hw, out_device);
    return check_last("disp_mesh");
}
extern "C" int cvx_affine_base_f32(int S, float* out_device, void* stream) {
    CVX_REQUIRE(out_device && S >= 1, "cvx_affine_base_f32: bad arguments");
    BaseTables t = {{S, 0, 0, 0, 0, 0}, {out_device, nullptr, nullptr, nullptr, nullptr, nullptr}};
    hipLaunchKernelGGL(k_affine_bases, dim3(cdiv(S, 64) > 4 ? cdiv(S, 64) : 4, 6), dim3(64), 0, as_stream(stream), t);
    return check_last("affine_base");
}

extern "C" void cvx_set_profiling(int enabled) {
    g_profiling = enabled < 0 ? 0 : (enabled > 3 ? 3 : enabled);
    g_marks.clear();
    g_pool_used = 0;
}

extern "C" int cvx_last_pair_profile(const char** names_host, float* ms_host, int max_stages) {
    if (g_marks.size() < 2) return 0;
    (void)hipEventSynchronize(g_marks.back().ev);
    int n = 0;
    for (size_t i = 1; i < g_marks.size() && n < max_stages; ++i) {
        if (g_marks[i].name[0] == 's' && g_marks[i].name[1] == 't' && g_marks[i].name[2] == 'a') continue;   // "start" of the next pair
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, g_marks[i - 1].ev, g_marks[i].ev);
        names_host[n] = g_marks[i].name;
        ms_host[n] = ms;
        ++n;
    }
    return n;
}

extern "C" size_t cvx_register_pair_workspace_bytes(const cvx_pair_params* p) {
    if (validate(p) != CVX_OK) return 0;
    const ContextScope scope(p->ctx);
    return pair_layout(*p).total;
}

namespace cvx {
static int smooth_max(const int* smooth_host, int n_smooth) {
    int m = 0;
    for (int i = 0; i < n_smooth; ++i) m = smooth_host[i] > m ? smooth_host[i] : m;
    return m;
}

// inverse-consistency tail of a convex stage (:133-141): (disp_soft / scale).flip(1) of both fields, `iters` iterations, disp_ice.flip(1) * scale * gs -> dst
struct IcScratch { float *in1, *in2, *ic1, *ic2; void* ws; size_t ws_bytes; };
static int ic_tail(const float* soft, const float* soft2, int h, int w, int d, int iters, const float* bh, const float* bw, const float* bd,
                   const IcScratch& t, float gs, float* dst, hipStream_t s) {
    const dim3 gv((unsigned)cdiv64((int64_t)h * w * d, 256));
    hipLaunchKernelGGL(k_ic_prepare, dim3(gv.x, 2), dim3(256), 0, s, soft, soft2, h, w, d, t.in1, t.in2);
    const int rc = cvx_inverse_consistency_f32(t.in1, t.in2, h, w, d, iters, bh, bw, bd, t.ic1, t.ic2, t.ws, t.ws_bytes, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ic_finish, gv, dim3(256), 0, s, t.ic1, h, w, d, gs, dst);
    return CVX_OK;
}

// the label entry's inputs: two label maps [H][W][D], the channels' labels and weights (device [C]), the features' multiplier
struct LabelPair { const float *fixed, *moving; const int* present; const float* weights; float mult; };

// One call of register_pair_core: what every step reads and what a step leaves for a later one; the steps are its member functions, in the order they run.
namespace {
struct PairRun {
    const cvx_pair_params* p;
    const PairLayout& L;
    char* ws;
    hipStream_t s;
    const float *featF, *featM;             // full-resolution features: the caller's, or the MIND descriptors where they are written
    const LabelPair* labels;                // label entry: the pooled one-hot features come straight from the two label maps
    const CoupledPlan cp;                   // how the coupled-convex stage runs and what setup / plain_argmin prepare for it (made once per call, under the call's context)
    bool pooled_mind = false, mind_records = false;
    CoupledWs cw1{}, cw2{};                 // coupled-convex workspaces of the two directions (the plain argmin leaves its keys in their first key buffer)

    bool pooled() const { return pooled_mind || labels != nullptr; }      // fs / ms (and F2 / M2) are written by `features`
    bool f16() const { return p->fp16_storage != 0; }
    float* F(size_t off) const { return reinterpret_cast<float*>(ws + off); }
    int64_t* am() const { return reinterpret_cast<int64_t*>(ws + L.argmin); }
    int64_t* am2() const { return p->ic ? reinterpret_cast<int64_t*>(ws + L.argmin2) : nullptr; }

    // 1. features (:106-116), 2. coarse features (:118-119)
    int features(const float* img_fixed, const float* img_moving) {
        int rc;
        // MIND path: the descriptor is consumed only through its two stride poolings, so when the window sizes tile it is never
        // written at full resolution (launch_mind_pooled: raw patch SSDs -> normalise + exp + both poolings in one pass)
        const bool adam = p->lambda_weight > 0;
        // the Adam-grid pooling of the descriptor written as the loop's feature records (no planar copy, no re-packing pass) where the plan allows
        const int g2 = adam ? p->grid_sp_adam : 0, want_records = adam && options().mind_records != 0 ? (p->fp16_storage ? 2 : 1) : 0;
        if (p->n_feat == 0) {
            auto plan_of = [&](const float* img, const float* raw) {
                return mind_plan(MindUse{p->H, p->W, p->D, p->mind_r, p->mind_d, p->grid_sp, g2, want_records, aligned16(img), aligned16(raw)});
            };
            const MindPlan plF = plan_of(img_fixed, F(L.featF)), plM = plan_of(img_moving, F(L.featM));
            pooled_mind = plF.T != 0; mind_records = plF.records != 0;
            const size_t mws = cvx_mindssc_workspace_bytes(p->H, p->W, p->D, p->mind_r, p->mind_d);
            if (pooled_mind) {
                // The two images are independent until `correlate`.  Option mind_overlap = 1 runs the moving image's pass on a side stream (one
                // image's VALU-bound stencil beside the other's memory-bound normalise + pool pass); measured on the benchmark pair: 0.52 vs
                // 0.53 ms for the stage and a SLOWER pair (7.92 vs 7.76 ms) -- every one of these kernels fills the chip on its own -- so the
                // default keeps them in order.
                hipStream_t side = s; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
                const bool overlap = options().mind_overlap != 0 && side_stream(&side, &ev_fork, &ev_join);
                if (overlap) { (void)hipEventRecord(ev_fork, s); (void)hipStreamWaitEvent(side, ev_fork, 0); }
                else side = s;
                if ((rc = launch_mind_pooled(plF, img_fixed, F(L.fs), adam ? F(L.F2) : nullptr, F(L.featF), ws + L.mind_ws, mws, s))) return rc;
                rc = launch_mind_pooled(plM, img_moving, F(L.ms), adam ? F(L.M2) : nullptr, F(L.featM), ws + (overlap ? L.mind_ws2 : L.mind_ws), mws, side);
                if (overlap) { (void)hipEventRecord(ev_join, side); (void)hipStreamWaitEvent(s, ev_join, 0); }      // (joined even after an error)
                if (rc) return rc;
            } else {
                if ((rc = cvx_mindssc_f32(img_fixed, p->H, p->W, p->D, p->mind_r, p->mind_d, F(L.featF), ws + L.mind_ws, mws, s))) return rc;
                if ((rc = cvx_mindssc_f32(img_moving, p->H, p->W, p->D, p->mind_r, p->mind_d, F(L.featM), ws + L.mind_ws, mws, s))) return rc;
            }
            featF = F(L.featF); featM = F(L.featM);
        }
        if (labels) {
            // label path: the weighted one-hot volumes are consumed only through the same two poolings and are never written either
            if ((rc = launch_label_pooled(labels->fixed, p->H, p->W, p->D, L.C, labels->present, labels->weights, labels->mult, p->grid_sp, F(L.fs), g2,
                                          adam ? F(L.F2) : nullptr, s))) return rc;
            if ((rc = launch_label_pooled(labels->moving, p->H, p->W, p->D, L.C, labels->present, labels->weights, labels->mult, p->grid_sp, F(L.ms), g2,
                                          adam ? F(L.M2) : nullptr, s))) return rc;
        }
        mark(labels ? "label_features" : "mind", s);
        if (!pooled()) {
            if ((rc = cvx_avgpool_f32(featF, L.C, p->H, p->W, p->D, p->grid_sp, F(L.fs), s))) return rc;
            if ((rc = cvx_avgpool_f32(featM, L.C, p->H, p->W, p->D, p->grid_sp, F(L.ms), s))) return rc;
        }
        return CVX_OK;
    }
    // everything that depends on the geometry alone, in one launch (k_pair_setup)
    void setup() {
        // the plain argmin leaves its keys in the first key buffer of the coupled-convex workspace
        Carver cv1(ws + L.conv_ws), cv2(p->ic ? ws + L.conv_ws2 : nullptr);
        cw1 = coupled_layout(cv1, L.h, L.w, L.d, p->disp_hw); cw2 = coupled_layout(cv2, L.h, L.w, L.d, p->disp_hw);
        const bool adam_tables = p->lambda_weight > 0;
        // (m, v zeroed here only if 16-byte stores fit: 3 * V2 floats from a 256-byte aligned offset)
        const bool zero_state = adam_tables && (3 * L.V2) % 4 == 0;
        const bool clear_counts = cp.prep == CoupledPrep::Keys;      // (the keys are set to all ones whatever the plan says: DESIGN.md 34.1)
        PairSetup a = {{{L.h, L.w, L.d, L.h2, L.w2, L.d2},
                        {F(L.bh), F(L.bw), F(L.bd), adam_tables ? F(L.bh2) : nullptr, adam_tables ? F(L.bw2) : nullptr, adam_tables ? F(L.bd2) : nullptr}},
                       p->disp_hw, F(L.mesh), {cw1.keys[0], cw2.keys[0]}, L.v,
                       {clear_counts ? cw1.counts : nullptr, clear_counts ? cw2.counts : nullptr},
                       {zero_state ? reinterpret_cast<float4*>(ws + L.m) : nullptr, zero_state ? reinterpret_cast<float4*>(ws + L.v_) : nullptr}, 3 * L.V2 / 4};
        hipLaunchKernelGGL(k_pair_setup, dim3(zero_state ? 1024 : 64), dim3(256), 0, s, a);
        if (adam_tables && !zero_state) {
            (void)hipMemsetAsync(F(L.m), 0, sizeof(float) * 3 * L.V2, s);
            (void)hipMemsetAsync(F(L.v_), 0, sizeof(float) * 3 * L.V2, s);
        }
    }
    int plain_argmin(const float* ssd, unsigned long long* keys, int64_t* argmin, const char* done) {     // keys stay in the coupled workspace's first buffer
        const int rc = cp.prep == CoupledPrep::Winners64 ? launch_argmin(ssd, f16(), nullptr, nullptr, 0.0f, false, L.K, L.v, keys, argmin, s)
                                                         : launch_argmin_keys(ssd, f16(), L.K, L.v, keys, s);     // prep Keys: `setup` armed them
        if (rc == CVX_OK) mark(done, s);
        return rc;
    }
    // one direction of the exact convex stage: cost volume, plain argmin, a profile mark behind each
    int exact_direction(const float* fix, const float* mov, const cvx_corr_opts* copt, float* ssd, unsigned long long* keys, int64_t* argmin,
                        const char* correlated, const char* done) {
        const int rc = cvx_correlate_ex_f32(fix, mov, L.C, L.h, L.w, L.d, p->disp_hw, copt, ssd, nullptr, ws + L.corr_ws,
                                            cvx_correlate_workspace_bytes(L.C, L.h, L.w, L.d, p->disp_hw), s);
        if (rc) return rc;
        mark(correlated, s);
        return plain_argmin(ssd, keys, argmin, done);
    }
    // 3. forward (and reverse) correlation + coupled convex                      (:124-130)
    int convex() {
        int rc;
        const cvx_corr_opts copt = {p->cost, p->n_box == 1 ? 1 : 2, p->corr_fast, f16() ? 2 : 0};
        const bool variant = copt.cost || copt.n_box == 1 || copt.fast || copt.f16;
        if (p->fp16_storage) {                      // features are stored in half precision by the reference's GPU default (MIND:79)
            if ((rc = cvx_round_f16_f32(F(L.fs), (int64_t)L.C * L.v, s)) || (rc = cvx_round_f16_f32(F(L.ms), (int64_t)L.C * L.v, s))) return rc;
        }
        // Certified-fast path (option corr_cert, default): the cost volumes in the fast arithmetic (unscaled, 2^-16 relative to ATen's), every
        // argmin decision certified against the exact arithmetic or evaluated exactly (certify.hip) -- the SAME winners, hence the same field bits,
        // as the exact kernels below; packaged operator only (SSD, two boxes, float32, pruned passes).
        // (which geometries take it, and with which kernel: corr_plan, correlate.hip)
        const CorrPlan plan = corr_plan(L.C, L.h, L.w, L.d, p->disp_hw, CorrUse{variant, p->ic != 0, cp.passes == CoupledPasses::Streamed});
        if (plan.pair_cert) {
            const size_t fws = corr_certfast_workspace_bytes(L.C, L.h, L.w, L.d, p->disp_hw), qws = corr_certify_workspace_bytes(L.C, L.h, L.w, L.d, p->disp_hw);
            auto cert_stage = [&](int stage) {
                return coupled_convex_cert_impl(F(L.ssd), F(L.fs), F(L.ms), F(L.soft), ws + L.cert_ws, p->ic ? F(L.ssd2) : nullptr, F(L.ms), F(L.fs),
                                                p->ic ? F(L.soft2) : nullptr, p->ic ? ws + L.cert_ws2 : nullptr, F(L.mesh), L.C, L.h, L.w, L.d, p->disp_hw, qws, cp.refine, s, stage);
            };
            if ((rc = cert_stage(1))) return rc;                                    // keys, counters, tail values
            if ((rc = launch_corr_certfast(F(L.fs), F(L.ms), L.C, L.h, L.w, L.d, p->disp_hw, F(L.ssd), ws + L.corr_ws, fws, s))) return rc;
            mark("correlate", s);
            if ((rc = cert_stage(2))) return rc;                                    // the plain argmin streams the volume while the Infinity Cache holds it
            mark("argmin", s);
            if (p->ic) {
                if ((rc = launch_corr_certfast(F(L.ms), F(L.fs), L.C, L.h, L.w, L.d, p->disp_hw, F(L.ssd2), ws + L.corr_ws, fws, s))) return rc;
                mark("correlate_rev", s);
                if ((rc = cert_stage(3))) return rc;
                mark("argmin_rev", s);
            }
            if ((rc = cert_stage(4))) return rc;
            return cert_stage(5);
        }
        // Both directions' cost volumes in ONE launch of the fused kernel when the pair is inverse consistent (option corr_dual): the stage
        // interval "correlate" then covers both directions and "correlate_rev" is not recorded.
        if (plan.pair_dual) {
            const size_t fws = corr_fused_workspace_bytes(L.C, L.h, L.w, L.d, p->disp_hw);
            if ((rc = launch_corr_fused_dual(F(L.fs), F(L.ms), L.C, L.h, L.w, L.d, p->disp_hw, copt.cost, copt.n_box, copt.fast, copt.f16, F(L.ssd), F(L.ssd2),
                                             ws + L.corr_ws, fws, ws + L.corr_ws2, s))) return rc;
            mark("correlate", s);
            if ((rc = plain_argmin(F(L.ssd), cw1.keys[0], am(), "argmin"))) return rc;
            if ((rc = plain_argmin(F(L.ssd2), cw2.keys[0], am2(), "argmin_rev"))) return rc;
        } else {
            if ((rc = exact_direction(F(L.fs), F(L.ms), variant ? &copt : nullptr, F(L.ssd), cw1.keys[0], am(), "correlate", "argmin"))) return rc;
            // reverse direction (:136-138): same operators with the roles swapped
            if (p->ic && (rc = exact_direction(F(L.ms), F(L.fs), variant ? &copt : nullptr, F(L.ssd2), cw2.keys[0], am2(), "correlate_rev", "argmin_rev"))) return rc;
        }
        // both coupled-convex solves in the same launches (ic) or the forward one alone
        const bool idx = cp.seed == CoupledSeed::Indices;
        return coupled_convex_dual_impl(cp, F(L.ssd), idx ? am() : nullptr, F(L.soft), ws + L.conv_ws, p->ic ? F(L.ssd2) : nullptr, idx ? am2() : nullptr,
                                        p->ic ? F(L.soft2) : nullptr, p->ic ? ws + L.conv_ws2 : nullptr, F(L.mesh),
                                        cvx_coupled_convex_workspace_bytes(L.h, L.w, L.d, p->disp_hw), s);
    }
    // dst = interpolate(src * grid_sp_adam, (H,W,D)) of an Adam-grid field (:182), then k > 0: three zero-padded k^3 box filters (:185-191)
    int upsample_smoothed(const float* src, int k, float* dst) {
        int rc;
        if (k <= 0) return launch_resize(src, 3, L.h2, L.w2, L.d2, dst, p->H, p->W, p->D, (float)p->grid_sp_adam, 1.0f, s);
        float *tmp = F(L.smooth_ws), *tmp2 = F(L.smooth_ws2);
        if ((rc = launch_resize(src, 3, L.h2, L.w2, L.d2, tmp, p->H, p->W, p->D, (float)p->grid_sp_adam, 1.0f, s))) return rc;
        if ((rc = launch_box_zero(tmp, tmp2, 3, p->H, p->W, p->D, k, false, s))) return rc;
        if ((rc = launch_box_zero(tmp2, tmp, 3, p->H, p->W, p->D, k, false, s))) return rc;
        return launch_box_zero(tmp, dst, 3, p->H, p->W, p->D, k, false, s);
    }
    // Adam instance optimisation and the full-resolution output                   (:147-191)
    int adam_and_output(const int* snap_iters_host, int n_snap, const int* smooth_host, int n_smooth, float* out_field) {
        int rc;
        if (!pooled()) {
            if ((rc = cvx_avgpool_f32(featF, L.C, p->H, p->W, p->D, p->grid_sp_adam, F(L.F2), s))) return rc;
            if ((rc = cvx_avgpool_f32(featM, L.C, p->H, p->W, p->D, p->grid_sp_adam, F(L.M2), s))) return rc;
        }
        // disp_lr = interpolate(disp_hr, (H2,W2,D2)); weight = disp_lr / grid_sp_adam       (:153,156)
        // ic=True: the up-sampling of the coarse field (L.upin) is folded into this resize; ic=False: coarse field, coarse units (:143-144)
        if (p->ic) rc = launch_resize2(F(L.upin), 3, L.h, L.w, L.d, p->H, p->W, p->D, F(L.disp_hr), F(L.P), L.h2, L.w2, L.d2, (float)p->grid_sp_adam, s);
        else rc = launch_resize(F(L.soft), 3, L.h, L.w, L.d, F(L.P), L.h2, L.w2, L.d2, 1.0f, (float)p->grid_sp_adam, s);
        if (rc) return rc;
        // (m = v = 0: k_pair_setup)
        // (fp16 storage: the Adam loop keeps its feature records in half precision -- rounded when the records are built)
        mark("adam_setup", s);
        const cvx_smoother two_pools = {0, 2, {3, 3, 0, 0}, {0.f, 0.f, 0.f, 0.f, 0.f}};            // task3_docker.py:191
        if ((rc = adam_run_impl({.F2 = F(L.F2), .M2 = F(L.M2), .C = L.C, .h = L.h2, .w = L.w2, .d = L.d2, .P = F(L.P), .m = F(L.m), .v = F(L.v_),
                                 .lambda_weight = p->lambda_weight, .niter = p->selected_niter, .step0 = 0, .cost_scale = p->cost_scale,
                                 .base_h = F(L.bh2), .base_w = F(L.bw2), .base_d = F(L.bd2), .U = F(L.U), .grad_out = nullptr,
                                 .snapshot_iters_host = snap_iters_host, .n_snap = n_snap, .snapshots = n_snap ? F(L.snaps) : nullptr,
                                 .workspace = ws + L.adam_ws, .workspace_bytes = cvx_adam_workspace_bytes(L.C, L.h2, L.w2, L.d2), .stream = s,
                                 .sm = p->n_spline_pools == 2 ? &two_pools : nullptr, .keep_state = false, .f16_features = f16(),
                                 .fast = p->adam_fast, .features_are_records = mind_records}))) return rc;
        mark("adam", s);
        // disp_hr = interpolate(fitted_grid * grid_sp_adam, (H,W,D))                            (:182)
        if (n_snap > 0) {                       // self_configuring/convex_adam_MIND.py:115-139: every snapshot x every final smoothing
            for (int i = 0; i < n_snap; ++i)
                for (int j = 0; j < n_smooth; ++j)
                    if ((rc = upsample_smoothed(F(L.snaps) + (size_t)i * 3 * L.V2, smooth_host[j], out_field + ((size_t)i * n_smooth + j) * 3 * L.V))) return rc;
        } else if ((rc = upsample_smoothed(F(L.U), p->selected_smooth, out_field))) return rc;
        mark("upsample", s);
        return CVX_OK;
    }
};
}  // namespace

// out_field: the field of the packaged pipeline ([3][H][W][D]) when n_snap == 0; otherwise [n_snap][n_smooth][3][H][W][D]: for every
// listed Adam iteration the up-sampled disp_sample of that iteration, once per listed final smoothing (0 = none, k = three k^3 boxes)
static int register_pair_core(const float* img_fixed, const float* img_moving, const float* feat_fixed, const float* feat_moving,
                              const cvx_pair_params* p, float* out_field, int* out_dims_host, const int* snap_iters_host, int n_snap,
                              const int* smooth_host, int n_smooth, void* workspace, size_t workspace_bytes, void* stream, const LabelPair* labels = nullptr) {
    int rc = validate(p);
    if (rc) return rc;
    const ContextScope scope(p->ctx);           // switches and tables of this call (cvx_pair_params.ctx; nullptr keeps the thread's)
    CVX_REQUIRE(out_field && workspace, "cvx_register_pair_f32: null pointer");
    if (labels) CVX_REQUIRE(p->n_feat >= 1 && labels->fixed && labels->moving && labels->present && labels->weights,
                            "cvx_register_label_pair_f32: label maps, channel labels or weights missing, or n_feat == 0 (n_feat = number of channels)");
    else if (p->n_feat == 0) CVX_REQUIRE(img_fixed && img_moving, "cvx_register_pair_f32: images missing");
    else CVX_REQUIRE(feat_fixed && feat_moving, "cvx_register_pair_f32: feature volumes missing");
    const PairLayout L = pair_layout(*p, n_snap, n_snap ? smooth_max(smooth_host, n_smooth) : 0);
    if (workspace_bytes < L.total) return fail(CVX_ERR_WORKSPACE, "cvx_register_pair_f32: workspace %zu < %zu", workspace_bytes, L.total);
    hipStream_t s = as_stream(stream);
    if (g_profiling < 2) { g_marks.clear(); g_pool_used = 0; }
    mark("start", s);
    // stage intervals "correlate" / "correlate_rev" = the fused kernel alone; the padded feature copies (and the certification set-up before them) are
    // "correlate_prep" (only while profiling: the hook records an event)
    corr_fused_set_prep_hook(g_profiling ? +[](hipStream_t st) { mark("correlate_prep", st); } : nullptr);
    struct HookReset { ~HookReset() { corr_fused_set_prep_hook(nullptr); } } hook_reset;

    // no winners, vouched: the run computes the plain argmin itself, as keys or as int64 winners (cp.prep); made here, under `scope`, and never kept
    PairRun run = {p, L, static_cast<char*>(workspace), s, feat_fixed, feat_moving, labels,
                   coupled_plan(CoupledUse{L.h, L.w, L.d, p->disp_hw, p->fp16_storage != 0, false, true, false, p->ic ? 2 : 1})};
    const bool adam = p->lambda_weight > 0;
    if ((rc = run.features(img_fixed, img_moving))) return rc;
    run.setup();
    mark("pool", s);
    if ((rc = run.convex())) return rc;
    mark("coupled_convex", s);
    if (p->ic) {                                // (:133-141)
        const IcScratch t = {run.F(L.in1), run.F(L.in2), run.F(L.ic1), run.F(L.ic2), run.ws + L.ic_ws, cvx_inverse_consistency_workspace_bytes(L.h, L.w, L.d)};
        if ((rc = ic_tail(run.F(L.soft), run.F(L.soft2), L.h, L.w, L.d, 15, run.F(L.bh), run.F(L.bw), run.F(L.bd), t, (float)p->grid_sp, run.F(L.upin), s))) return rc;
        // with the Adam stage following, disp_hr is only ever read by the down-sampling to the Adam grid: the two resizes are
        // folded into one there (launch_resize2) and the full-resolution field is never written
        if (!adam && (rc = launch_resize(run.F(L.upin), 3, L.h, L.w, L.d, out_field, p->H, p->W, p->D, 1.0f, 1.0f, s))) return rc;
        mark("inverse_consistency", s);
    }
    if (adam) {
        if ((rc = run.adam_and_output(snap_iters_host, n_snap, smooth_host, n_smooth, out_field))) return rc;
    } else if (!p->ic) {                        // ic=False: coarse field, coarse units (:143-144)
        (void)hipMemcpyAsync(out_field, run.F(L.soft), sizeof(float) * 3 * L.v, hipMemcpyDeviceToDevice, s);
    }
    const bool full = p->ic || adam;
    if (out_dims_host) { out_dims_host[0] = full ? p->H : L.h; out_dims_host[1] = full ? p->W : L.w; out_dims_host[2] = full ? p->D : L.d; }
    return check_last("register_pair");
}
}  // namespace cvx

extern "C" int cvx_register_pair_f32(const float* img_fixed, const float* img_moving, const float* feat_fixed,
                                     const float* feat_moving, const cvx_pair_params* p, float* out_field,
                                     int* out_dims_host, void* workspace, size_t workspace_bytes, void* stream) {
    return register_pair_core(img_fixed, img_moving, feat_fixed, feat_moving, p, out_field, out_dims_host, nullptr, 0, nullptr, 0, workspace,
                              workspace_bytes, stream);
}

// ---- label maps in, field out: the pair pipeline with the pooled one-hot features written straight from the maps (labelpool.hip) ----
// (the pair layout for n_feat = C holds no full-resolution feature buffer, and the label kernel needs no scratch: the same layout function)
extern "C" size_t cvx_register_label_pair_workspace_bytes(const cvx_pair_params* p) {
    if (validate(p) != CVX_OK) return 0;
    if (p->n_feat < 1) { fail(CVX_ERR_INVALID_ARG, "cvx_register_label_pair: n_feat must be the number of channels (>= 1)"); return 0; }
    const ContextScope scope(p->ctx);
    return pair_layout(*p).total;
}

extern "C" int cvx_register_label_pair_f32(const float* lab_fixed, const float* lab_moving, const int* present, const float* weights, float mult,
                                           const cvx_pair_params* p, float* out_field, int* out_dims_host, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    const LabelPair labels = {lab_fixed, lab_moving, present, weights, mult};
    return register_pair_core(nullptr, nullptr, nullptr, nullptr, p, out_field, out_dims_host, nullptr, 0, nullptr, 0, workspace, workspace_bytes, stream,
                              &labels);
}

extern "C" size_t cvx_register_pair_snapshots_workspace_bytes(const cvx_pair_params* p, int n_snap, const int* smooth_host, int n_smooth) {
    if (validate(p) != CVX_OK || n_snap < 1 || n_smooth < 1 || !smooth_host) return 0;
    const ContextScope scope(p->ctx);
    return pair_layout(*p, n_snap, smooth_max(smooth_host, n_smooth)).total;
}

extern "C" int cvx_register_pair_snapshots_f32(const float* img_fixed, const float* img_moving, const float* feat_fixed,
                                               const float* feat_moving, const cvx_pair_params* p, const int* snapshot_iters_host, int n_snap,
                                               const int* smooth_host, int n_smooth, float* out_fields, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    int rc = validate(p);
    if (rc) return rc;
    CVX_REQUIRE(snapshot_iters_host && n_snap >= 1 && smooth_host && n_smooth >= 1, "cvx_register_pair_snapshots_f32: snapshot / smoothing lists missing");
    CVX_REQUIRE(p->lambda_weight > 0, "cvx_register_pair_snapshots_f32: snapshots exist only with the Adam stage (lambda_weight > 0)");
    for (int i = 0; i < n_snap; ++i)
        CVX_REQUIRE(snapshot_iters_host[i] >= 1 && snapshot_iters_host[i] <= p->selected_niter && (i == 0 || snapshot_iters_host[i] > snapshot_iters_host[i - 1]),
                    "cvx_register_pair_snapshots_f32: snapshot iterations must be ascending and within 1..selected_niter");
    for (int i = 0; i < n_smooth; ++i)
        CVX_REQUIRE(smooth_host[i] == 0 || (smooth_host[i] & 1), "cvx_register_pair_snapshots_f32: smoothing sizes must be 0 or odd");
    return register_pair_core(img_fixed, img_moving, feat_fixed, feat_moving, p, out_fields, nullptr, snapshot_iters_host, n_snap, smooth_host,
                              n_smooth, workspace, workspace_bytes, stream);
}

// ---- several pairs at once on internal streams ------------------------------------------------------------
// The kernels of one pair are chained by data dependencies and leave issue slots idle (short grids, tails);
// independent pairs fill them.  Pairs are dealt round-robin onto `n_streams` internal non-blocking streams
// that fork from / join back into the caller's stream with events, so the call is still asynchronous and
// ordered with respect to the caller's stream.  workspace = n_streams x cvx_register_pair_workspace_bytes().
namespace cvx {
struct StreamPool {
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> done;
    hipEvent_t fork = nullptr;
    int device = -1;
};
static thread_local StreamPool g_pool_streams;
static int ensure_streams(int n) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    StreamPool& P = g_pool_streams;
    if (P.device != dev) { P.streams.clear(); P.done.clear(); P.fork = nullptr; P.device = dev; }   // leaked on device switch (rare)
    if (!P.fork && hipEventCreateWithFlags(&P.fork, hipEventDisableTiming) != hipSuccess) return fail(CVX_ERR_LAUNCH, "event create failed");
    while ((int)P.streams.size() < n) {
        hipStream_t s; hipEvent_t e;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return fail(CVX_ERR_LAUNCH, "stream create failed");
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(CVX_ERR_LAUNCH, "event create failed");
        P.streams.push_back(s); P.done.push_back(e);
    }
    return CVX_OK;
}
}  // namespace cvx

extern "C" int cvx_register_pairs_f32(int n_pairs, const float* const* img_fixed, const float* const* img_moving,
                                      const float* const* feat_fixed, const float* const* feat_moving,
                                      const cvx_pair_params* p, float* const* out_fields, int* out_dims_host, void* workspace,
                                      size_t workspace_bytes, int n_streams, void* stream) {
    CVX_REQUIRE(n_pairs >= 1 && out_fields && workspace, "cvx_register_pairs_f32: bad arguments");
    CVX_REQUIRE(n_streams >= 1 && n_streams <= 8, "cvx_register_pairs_f32: n_streams must be 1..8");
    if (n_streams > n_pairs) n_streams = n_pairs;
    const size_t per = cvx_register_pair_workspace_bytes(p);
    if (per == 0) return CVX_ERR_INVALID_ARG;
    const size_t per_al = align_up(per, 4096);
    if (workspace_bytes < per_al * (size_t)n_streams) return fail(CVX_ERR_WORKSPACE, "cvx_register_pairs_f32: workspace %zu < %zu", workspace_bytes, per_al * (size_t)n_streams);
    int rc = ensure_streams(n_streams);
    if (rc) return rc;
    StreamPool& P = g_pool_streams;
    hipStream_t user = as_stream(stream);
    const int saved_prof = g_profiling;
    g_profiling = 0;                                  // stage marks are per stream; not recorded in batch mode
    (void)hipEventRecord(P.fork, user);
    for (int s = 0; s < n_streams; ++s) (void)hipStreamWaitEvent(P.streams[s], P.fork, 0);
    for (int i = 0; i < n_pairs && rc == CVX_OK; ++i) {
        const int s = i % n_streams;
        g_side_slot = s;
        rc = cvx_register_pair_f32(img_fixed ? img_fixed[i] : nullptr, img_moving ? img_moving[i] : nullptr,
                                   feat_fixed ? feat_fixed[i] : nullptr, feat_moving ? feat_moving[i] : nullptr, p, out_fields[i],
                                   out_dims_host, static_cast<char*>(workspace) + per_al * (size_t)s, per, P.streams[s]);
    }
    for (int s = 0; s < n_streams; ++s) {
        (void)hipEventRecord(P.done[s], P.streams[s]);
        (void)hipStreamWaitEvent(user, P.done[s], 0);
    }
    g_profiling = saved_prof;
    g_side_slot = 0;
    return rc;
}

// ---- the convex stage of the CuRIOUS script in one call (l2r_2020_convexAdam_CuRIOUS.py:335-357) ------------------------------------
// correlate -> coupled convex on the masked volume, for the reverse direction too when ic_iters > 0, inverse consistency with the
// script's scale and flips, trilinear up-sampling: the operators cvx_register_pair_f32 chains with lambda_weight = 0, with the cell
// masks, the caller's iteration count and caller-supplied coarse features.  The two directions run one after the other through ONE
// cost volume (744 MB at the script's size); the exact correlation kernels, so every intermediate is the oracle's bit for bit.
namespace cvx {
struct StageWs {
    float *ssd, *mesh, *soft, *soft2, *in1, *in2, *ic1, *ic2, *upin, *bh, *bw, *bd;
    int64_t* argmin;
    char *corr_ws, *conv_ws, *ic_ws;
    size_t corr_bytes, conv_bytes, ic_bytes;
};
static StageWs stage_layout(Carver& cv, const cvx_convex_stage_params& p) {
    const int n = 2 * p.disp_hw + 1;
    const size_t v = (size_t)p.h * p.w * p.d, K = (size_t)n * n * n;
    StageWs s{};
    s.ssd = cv.take<float>(K * v);
    s.argmin = cv.take<int64_t>(v);
    s.mesh = cv.take<float>(3 * K);
    s.soft = cv.take<float>(3 * v);
    s.corr_bytes = cvx_correlate_workspace_bytes(p.C, p.h, p.w, p.d, p.disp_hw);
    s.corr_ws = cv.take<char>(s.corr_bytes);
    s.conv_bytes = cvx_coupled_convex_workspace_bytes(p.h, p.w, p.d, p.disp_hw);
    s.conv_ws = cv.take<char>(s.conv_bytes);
    if (p.ic_iters > 0) {
        s.soft2 = cv.take<float>(3 * v);
        s.in1 = cv.take<float>(3 * v); s.in2 = cv.take<float>(3 * v);
        s.ic1 = cv.take<float>(3 * v); s.ic2 = cv.take<float>(3 * v);
        s.upin = cv.take<float>(3 * v);
        s.bh = cv.take<float>(p.h); s.bw = cv.take<float>(p.w); s.bd = cv.take<float>(p.d);
        s.ic_bytes = cvx_inverse_consistency_workspace_bytes(p.h, p.w, p.d);
        s.ic_ws = cv.take<char>(s.ic_bytes);
    }
    return s;
}
static int stage_params_ok(const cvx_convex_stage_params* p) {
    CVX_REQUIRE(p, "cvx_convex_stage_f32: null parameters");
    CVX_REQUIRE(p->reserved_[0] == 0 && p->reserved_[1] == 0 && p->reserved_[2] == 0 && p->reserved_[3] == 0,
                "cvx_convex_stage_f32: reserved fields must be zero (struct laid out by a different header?)");
    CVX_REQUIRE(p->C >= 1 && p->h >= 1 && p->w >= 1 && p->d >= 1 && p->disp_hw >= 0 && p->grid_sp >= 1 && p->ic_iters >= 0,
                "cvx_convex_stage_f32: bad extent, search width, grid spacing or iteration count");
    CVX_REQUIRE((double)(2 * p->disp_hw + 1) * (2 * p->disp_hw + 1) * (2 * p->disp_hw + 1) * ((double)p->h * p->w * p->d) < 2.0e9,
                "cvx_convex_stage_f32: cost volume of more than 2e9 entries");
    return CVX_OK;
}
}  // namespace cvx

extern "C" size_t cvx_convex_stage_workspace_bytes(const cvx_convex_stage_params* p) {
    if (stage_params_ok(p) != CVX_OK) return 0;
    Carver m;
    stage_layout(m, *p);
    return ws_query(m);
}

extern "C" int cvx_convex_stage_f32(const float* feat_fix, const float* feat_mov, const unsigned char* mask_fix, const unsigned char* mask_mov,
                                    const cvx_convex_stage_params* p, float* coarse_field, float* disp_hr, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    int rc = stage_params_ok(p);
    if (rc) return rc;
    CVX_REQUIRE(feat_fix && feat_mov && workspace && (coarse_field || disp_hr), "cvx_convex_stage_f32: null pointer");
    CVX_REQUIRE(!disp_hr || (p->H >= 1 && p->W >= 1 && p->D >= 1), "cvx_convex_stage_f32: bad full-resolution extent");
    if (workspace_bytes < cvx_convex_stage_workspace_bytes(p)) return fail(CVX_ERR_WORKSPACE, "cvx_convex_stage_f32: workspace too small");
    const ContextScope scope(p->ctx);
    hipStream_t s = as_stream(stream);
    Carver cv(workspace);
    const StageWs L = stage_layout(cv, *p);
    const int h = p->h, w = p->w, d = p->d;
    if ((rc = cvx_disp_mesh_f32(p->disp_hw, L.mesh, stream))) return rc;
    // one direction: cost volume + plain argmin of the UNMASKED volume, then the six passes on the masked one (`ssd` is not written)
    auto direction = [&](const float* a, const float* b, const unsigned char* mask, float* soft) -> int {
        int r = cvx_correlate_ex_f32(a, b, p->C, h, w, d, p->disp_hw, nullptr, L.ssd, L.argmin, L.corr_ws, L.corr_bytes, stream);
        if (r) return r;
        return coupled_convex_impl(L.ssd, false, L.argmin, L.mesh, h, w, d, p->disp_hw, soft, L.conv_ws, L.conv_bytes, stream, mask);
    };
    if (p->ic_iters == 0) {                     // (:335-341) forward direction only
        float* soft = coarse_field ? coarse_field : L.soft;
        if ((rc = direction(feat_fix, feat_mov, mask_fix, soft))) return rc;
        if (disp_hr && (rc = launch_resize(soft, 3, h, w, d, disp_hr, p->H, p->W, p->D, (float)p->grid_sp, 1.0f, s))) return rc;
        return check_last("convex_stage");
    }
    if ((rc = direction(feat_fix, feat_mov, mask_fix, L.soft))) return rc;
    if ((rc = direction(feat_mov, feat_fix, mask_mov, L.soft2))) return rc;          // (:348-350)
    if ((rc = cvx_affine_base_f32(h, L.bh, stream)) || (rc = cvx_affine_base_f32(w, L.bw, stream)) || (rc = cvx_affine_base_f32(d, L.bd, stream))) return rc;
    float* up = coarse_field ? coarse_field : L.upin;
    if ((rc = ic_tail(L.soft, L.soft2, h, w, d, p->ic_iters, L.bh, L.bw, L.bd, {L.in1, L.in2, L.ic1, L.ic2, L.ic_ws, L.ic_bytes}, (float)p->grid_sp, up, s))) return rc;          // (:351-354)
    if (disp_hr && (rc = launch_resize(up, 3, h, w, d, disp_hr, p->H, p->W, p->D, 1.0f, 1.0f, s))) return rc;
    return check_last("convex_stage");
}
