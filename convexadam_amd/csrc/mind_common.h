// mind_common.h -- definitions shared by the two MIND-SSC stencil kernels (mind.hip: tiled, mindmarch.hip: z-marching)
#pragma once
#include <type_traits>
#include "cvx_common.h"

namespace cvx {

// shift pairs in the reference's PRE-permutation channel order (derived by executing convex_adam_utils.py:31-47)
struct MindOffsets {
    int o1[12][3] = {{0,0,-1},{0,-1,0},{0,-1,0},{0,0,1},{0,0,1},{1,0,0},
                     {1,0,0},{1,0,0},{0,1,0},{0,1,0},{0,1,0},{0,1,0}};
    int o2[12][3] = {{-1,0,0},{-1,0,0},{0,0,-1},{-1,0,0},{0,-1,0},{0,0,-1},
                     {0,-1,0},{0,0,1},{-1,0,0},{0,0,-1},{0,0,1},{1,0,0}};
};
// final channel j holds pre-permutation channel PERM[j], PERM = {6,8,1,11,2,10,0,7,9,4,5,3}
// (convex_adam_utils.py:66); the stores use its inverse: destination channel of pre-permutation channel c
__device__ constexpr int MIND_INV[12] = {6, 2, 4, 11, 9, 10, 0, 7, 1, 8, 5, 3};

struct MindStats {
    double m1, m2, m3;     // split grids (see oracle orc_split_make)
    double a1, a2, a3;     // exact partial sums
    float imin, imax;
    float mean_override;   // reference-bits mode (option mind_mean_threads): torch's own mean, see k_torch_sum_* in mind.hip
    int use_override;
    unsigned n_repair;     // single-pass pooled path: blocks whose pooled cells k_mind_repair recomputed
};

// Where the stencil pass puts the raw patch SSDs.  T == 0: planar [12][H][W][D].  T > 0 (pipeline, mind.hip::launch_mind_pooled): blocked by the
// tiles of k_mind_finish_pool -- [tile (z, y, x)][12][T][T][24] -- so that a tile is 12 T^2 24 contiguous floats: the second pass then reads whole
// 128-byte lines in order instead of 96-byte row pieces shared with the neighbouring tile (it runs at the depth of the L1 miss queue: half as many
// requests for the same bytes)
struct MindRawLayout {
    int T, ntx, nty;                 // tile edge (z, y), tiles along x (of 24 voxels) and y
    size_t tile_floats, chan_floats; // 12 T T 24 and T T 24 (planar: unused / H W D)
};

// The window pairs (larger, smaller) the pooled kernels are instantiated for -- k_mind_finish_pool, k_mind_repair (mind.hip), k_mind_march_pool
// (mindmarch.hip).  mind_pair_dispatch calls f(integral_constant<GA>, integral_constant<GB>) for the pair (ga, gb); false: not instantiated.
#define CVX_MIND_PAIRS(X) X(6, 2) X(6, 3) X(6, 6) X(4, 2) X(4, 4) X(2, 2)
template <typename F>
inline bool mind_pair_dispatch(int ga, int gb, F&& f) {
#define CVX_MIND_PAIR(GA, GB) if (ga == GA && gb == GB) { f(std::integral_constant<int, GA>{}, std::integral_constant<int, GB>{}); return true; }
    CVX_MIND_PAIRS(CVX_MIND_PAIR)
#undef CVX_MIND_PAIR
    return false;
}

// ---- which MIND-SSC kernels run: decided once, by mind_plan (mind.hip); the size queries, the two operators, the launchers and the
// whole-pair pipeline read the plan and combine nothing themselves.
struct MindUse {
    int H, W, D, radius, dilation;
    int g1, g2;                      // pooling windows (g2 == 0: one pooling); 0, 0: the full-resolution descriptor
    int records;                     // g2-pooled output wanted as the Adam loop's feature records: 1 float32, 2 half precision
    bool img_aligned, out_aligned;   // 16-byte alignment of the image and of what the stencil pass writes (the descriptor / the raw scratch)
};
enum class MindStencil { Unsupported, March16x32, March8x64, Tiled64, Tiled32 };    // MMGeo<16,32> / MMGeo<8,64> (mindmarch.hip), k_mind<R,64> / k_mind<R,32>
struct MindPlan {
    MindUse u;
    MindStencil stencil;             // Unsupported: the radius / dilation tile does not fit the LDS
    int nbuf; size_t lds;            // k_mind: LDS buffers of patch sums (1 or 2), dynamic LDS bytes
    int T, ga, gb; bool swap;        // pooling tile (0: not pooled), (larger, smaller) window; swap: the larger one is g2 and goes to out2
    bool single, force_repair;       // ONE pass over the image (k_mind_march_pool + k_mind_repair); option mind_single = 2: every block repaired
    bool single_unaligned;           // the single pass would apply, were the image 16-byte aligned (the scratch query assumed so)
    bool blocked; MindRawLayout lay; // two passes: raw SSDs blocked by the second pass's tiles (all zero: planar)
    bool records_ok; int records;    // feature records can be written: 0 < g2 <= g1; what out2 receives: u.records if so, else 0 (planar)
    int mean_threads; bool two_pass; // reference-bits mean (option mind_mean_threads, 0: the exactly rounded mean), at most 1024; chunked summation
    size_t raw_floats;               // floats of the two-pass `raw` scratch: max(blocked, planar) whatever the options say (callers cache it)
    bool finish4;                    // full descriptor: k_mind_finish<4> (16-byte stores), else <1>
    bool march() const { return stencil == MindStencil::March16x32 || stencil == MindStencil::March8x64; }
};
MindPlan mind_plan(const MindUse& u);
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// mindmarch.hip.  z-marching stencil (plan.march()): radius 1, dilation 2, rows of a multiple of 4 voxels, 16-byte aligned pointers
void launch_mind_march(const MindPlan& pl, const float* img, MindStats* st, float* out, hipStream_t s);
// single-pass pooled descriptor (plan.single): stencil + unclamped normalisation + both poolings, block statistics for k_mind_repair (mind.hip);
// out2 null: single pooling; plan.records: out2 receives feature records
void launch_mind_march_pool(const MindPlan& pl, const float* img, float* out1, void* out2, MindStats* st, unsigned* blk, hipStream_t s);
// mind.hip: MIND-SSC delivered only through its stride poolings (pipeline path, no full-resolution descriptor); `raw`: plan.raw_floats floats, not
// touched by the single pass.  st_out (nullable): the statistics block the launch carved from the workspace (n_repair).
int launch_mind_pooled(const MindPlan& pl, const float* img, float* out1, float* out2, float* raw, void* workspace, size_t workspace_bytes, hipStream_t s,
                       MindStats** st_out = nullptr);

}  // namespace cvx
