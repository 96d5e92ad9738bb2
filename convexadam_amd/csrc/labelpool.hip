// labelpool.hip -- label maps straight to the POOLED weighted one-hot features (no [C][H][W][D] one-hot volume).
//
// Reference call sites: the one-hot expansion convex_adam_nnUNet.py:19-38 followed by F.avg_pool3d(g, stride=g) at :101-102 and
// :117-118 (the only two readers of the full-resolution features).  Same bits as k_label_features + k_avgpool (pool.hip):
//   avg_pool3d adds the g^3 taps of a cell in raster order into a float32 sum that starts at +0 and divides once by g^3.  In channel
//   c of the weighted one-hot volume a tap is either v_c = mult * (1 * w_c) or mult * (0 * w_c) = +-0, and adding +-0 leaves the sum as
//   it is: the pooled value depends only on k, the number of voxels of the cell whose label is present[c],
//       pooled = fdiv(S_k, g^3),   S_0 = +0,   S_k = fl(S_(k-1) + v_c)          (k sequential additions, NOT k * v_c).
// A workgroup stages the channel index (one byte; C <= 255, 255 = "no channel") of every voxel of a tile in LDS once; threads then own
// (channel, cell) outputs of both grids, count their cell's bytes and write rows along D.  Algorithmic traffic: the label map read
// once, the two pooled tensors written once.
#include "cvx_common.h"

namespace cvx {

constexpr int LP_LUT = 8192;                    // labels 0 .. 8191 go through the label -> channel table (the range of cvx_label_histogram_i64)
constexpr int LP_NONE = 255;
constexpr int LP_TILE_BYTES = 32 * 1024;        // channel bytes of one tile
constexpr int LP_THREADS = 256;

struct LabelPoolGrid { int g, Ho, Wo, Do; float* out; };

// number of zero bytes of x
__device__ __forceinline__ int zero_bytes(unsigned x) {
    const unsigned y = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;              // bit 7 of a byte is clear iff the byte is zero
    return __popc(~y & 0x80808080u);
}

// the (channel, cell) outputs of one pooling grid inside the staged tile: T x T x TD voxels at (z0, y0, x0), row-major bytes in `chan`
template <int G>
__device__ __forceinline__ void label_pool_tile(const unsigned char* __restrict__ chan, const float* __restrict__ val, int C, int T, int TD, int z0,
                                                int y0, int x0, const LabelPoolGrid& q, int gr) {
    const int g = G > 0 ? G : gr;
    const int cw = T / g, cd = TD / g, row = cw * cd;                       // cells of the tile along W and D; outputs per (channel, cell plane)
    // thread t owns items t, t + 256, ... of (channel, b, e), e fastest: the item index advances in mixed radix (row, cd), no division per item
    const int sc = LP_THREADS / row, rem = LP_THREADS % row, sb = rem / cd, se = rem % cd;
    const int c0 = (int)threadIdx.x / row, r0 = (int)threadIdx.x % row, b0 = r0 / cd, e0 = r0 % cd;
    const float div = (float)(g * g * g), inv = 1.0f / div;
    const bool pow2 = (g & (g - 1)) == 0;
    const int hb = z0 / g, wb = y0 / g, db = x0 / g;
    for (int a = 0; a < cw && hb + a < q.Ho; ++a) {                          // (the tile has T / g cell planes along H as along W)
        int c = c0, b = b0, e = e0;
        while (c < C) {
            const int wo = wb + b, xo = db + e;
            if (wo < q.Wo && xo < q.Do) {                                   // a cell inside the pooled extent lies inside the volume
                const unsigned char* p = chan + ((a * g) * T + b * g) * TD + e * g;
                int k = 0;
                if (G > 0 && G % 2 == 0) {
                    // even windows: a cell's rows start at a multiple of G bytes (T, TD and the tile's LDS offset are multiples of G): 4 or 2 bytes per read
                    const unsigned cc = (unsigned)c * 0x01010101u;
#pragma unroll
                    for (int z = 0; z < G; ++z)
#pragma unroll
                        for (int y = 0; y < G; ++y) {
                            const unsigned char* r = p + (z * T + y) * TD;
                            if (G % 4 == 0) {
#pragma unroll
                                for (int x = 0; x < G / 4; ++x) k += zero_bytes(reinterpret_cast<const unsigned*>(r)[x] ^ cc);
                            } else {
#pragma unroll
                                for (int x = 0; x < G / 2; ++x) k += zero_bytes(((unsigned)reinterpret_cast<const unsigned short*>(r)[x] ^ (cc & 0xffffu)) | 0xffff0000u);
                            }
                        }
                } else if (G > 0) {
#pragma unroll
                    for (int z = 0; z < G; ++z)
#pragma unroll
                        for (int y = 0; y < G; ++y)
#pragma unroll
                            for (int x = 0; x < G; ++x) k += p[(z * T + y) * TD + x] == c ? 1 : 0;
                } else {
                    for (int z = 0; z < g; ++z)
                        for (int y = 0; y < g; ++y)
                            for (int x = 0; x < g; ++x) k += p[(z * T + y) * TD + x] == c ? 1 : 0;
                }
                const float v = val[c];
                float s = 0.0f;
                for (int j = 0; j < k; ++j) s += v;                         // S_k: the pooling's own chain of additions
                // (a power of two divides exactly: the product with its reciprocal is the correctly rounded quotient too)
                q.out[(((size_t)c * q.Ho + (hb + a)) * q.Wo + wo) * q.Do + xo] = pow2 ? s * inv : fdiv(s, div);
            }
            e += se; if (e >= cd) { e -= cd; ++b; }
            b += sb; if (b >= cw) { b -= cw; ++c; }
            c += sc;
        }
    }
}

__device__ __forceinline__ void label_pool_grid(const unsigned char* chan, const float* val, int C, int T, int TD, int z0, int y0, int x0,
                                                const LabelPoolGrid& q) {
    switch (q.g) {                                                          // (uniform) the packaged window sizes with their loops unrolled
        case 1: label_pool_tile<1>(chan, val, C, T, TD, z0, y0, x0, q, 1); break;
        case 2: label_pool_tile<2>(chan, val, C, T, TD, z0, y0, x0, q, 2); break;
        case 3: label_pool_tile<3>(chan, val, C, T, TD, z0, y0, x0, q, 3); break;
        case 4: label_pool_tile<4>(chan, val, C, T, TD, z0, y0, x0, q, 4); break;
        case 5: label_pool_tile<5>(chan, val, C, T, TD, z0, y0, x0, q, 5); break;
        case 6: label_pool_tile<6>(chan, val, C, T, TD, z0, y0, x0, q, 6); break;
        default: label_pool_tile<0>(chan, val, C, T, TD, z0, y0, x0, q, q.g); break;
    }
}

// tiles of T x T x TD voxels, T a multiple of both windows, TD a multiple of T; LDS: [LP_LUT] table, [256] channel values, [T * T * TD] bytes
__global__ __launch_bounds__(LP_THREADS) void k_label_pooled(const float* __restrict__ lab, int H, int W, int D, int C, const int* __restrict__ present,
                                                             const float* __restrict__ weights, float mult, int T, int TD, int ntw, int ntd, int ntiles,
                                                             LabelPoolGrid q1, LabelPoolGrid q2) {
    extern __shared__ __align__(16) unsigned char lp_sh[];
    unsigned char* lut = lp_sh;
    float* val = reinterpret_cast<float*>(lp_sh + LP_LUT);
    unsigned char* chan = lp_sh + LP_LUT + 256 * sizeof(float);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < LP_LUT / 4; i += LP_THREADS) reinterpret_cast<unsigned*>(lut)[i] = 0xffffffffu;
    cvx_barrier();
    for (int c = tid; c < C; c += LP_THREADS) {
        const int l = present[c];
        if (l >= 0 && l < LP_LUT) lut[l] = (unsigned char)c;
        val[c] = mult * (1.0f * weights[c]);                                // 10*(onehot*weight), convex_adam_nnUNet.py:35
    }
    cvx_barrier();
    for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
        const int x0 = (tile % ntd) * TD, y0 = ((tile / ntd) % ntw) * T, z0 = (tile / (ntd * ntw)) * T;
        for (int z = 0; z < T; ++z)
            for (int y = wave; y < T; y += LP_THREADS / 64) {
                const bool in_plane = z0 + z < H && y0 + y < W;
                const float* src = lab + ((size_t)(z0 + z) * W + (y0 + y)) * D + x0;
                unsigned char* dst = chan + (z * T + y) * TD;
                for (int x = lane; x < TD; x += 64) {
                    int ch = LP_NONE;                                       // outside the volume: no channel
                    if (in_plane && x0 + x < D) {
                        const int l = (int)src[x];
                        if (l >= 0 && l < LP_LUT) ch = lut[l];
                        else
                            for (int c = 0; c < C; ++c) ch = present[c] == l ? c : ch;     // a label outside the table's range
                    }
                    dst[x] = (unsigned char)ch;
                }
            }
        cvx_barrier();
        label_pool_grid(chan, val, C, T, TD, z0, y0, x0, q1);
        if (q2.g > 0) label_pool_grid(chan, val, C, T, TD, z0, y0, x0, q2);
        cvx_barrier();                                                      // the next tile overwrites `chan`
    }
}

// windows whose common tile does not fit the LDS budget: one thread per output, its cell's labels read from global memory
__global__ __launch_bounds__(256) void k_label_pooled_direct(const float* __restrict__ lab, int H, int W, int D, int C, const int* __restrict__ present,
                                                             const float* __restrict__ weights, float mult, LabelPoolGrid q) {
    const size_t n = (size_t)C * q.Ho * q.Wo * q.Do;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g = q.g;
    const int d = (int)(i % q.Do), w = (int)((i / q.Do) % q.Wo), h = (int)((i / ((size_t)q.Do * q.Wo)) % q.Ho);
    const int c = (int)(i / ((size_t)q.Do * q.Wo * q.Ho));
    const int pc = present[c];
    const float v = mult * (1.0f * weights[c]);
    const float* base = lab + (((size_t)h * g) * W + (size_t)w * g) * D + (size_t)d * g;
    float s = 0.0f;
    for (int z = 0; z < g; ++z)
        for (int y = 0; y < g; ++y) {
            const float* rowp = base + ((size_t)z * W + y) * D;
            for (int x = 0; x < g; ++x)
                if ((int)rowp[x] == pc) s += v;
        }
    q.out[i] = fdiv(s, (float)(g * g * g));
}

static int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

// lab [H][W][D] -> out1 [C][H/g1][W/g1][D/g1] and, g2 > 0, out2 [C][H/g2][W/g2][D/g2]; arguments checked by the callers
int launch_label_pooled(const float* lab, int H, int W, int D, int C, const int* present, const float* weights, float mult, int g1, float* out1,
                        int g2, float* out2, hipStream_t s) {
    const LabelPoolGrid q1 = {g1, H / g1, W / g1, D / g1, out1};
    const LabelPoolGrid q2 = {g2, g2 > 0 ? H / g2 : 0, g2 > 0 ? W / g2 : 0, g2 > 0 ? D / g2 : 0, out2};
    const int64_t T64 = g2 > 0 ? (int64_t)g1 / gcd64(g1, g2) * g2 : g1;
    if (T64 * T64 * T64 <= LP_TILE_BYTES) {
        const int T = (int)T64;
        const int td_max = LP_TILE_BYTES / (T * T) / T * T;                 // >= T
        const int TD = cdiv(D, T) * T < td_max ? cdiv(D, T) * T : td_max;
        // tiles up to the last voxel either grid pools (remainder voxels behind it are read by nobody)
        auto extent = [&](int n) { const int e1 = n / g1 * g1, e2 = g2 > 0 ? n / g2 * g2 : 0; return e1 > e2 ? e1 : e2; };
        const int nth = cdiv(extent(H), T), ntw = cdiv(extent(W), T), ntd = cdiv(extent(D), TD);
        const int64_t ntiles = (int64_t)nth * ntw * ntd;
        if (ntiles > 0x7fffffff) return fail(CVX_ERR_UNSUPPORTED, "label_features_pooled: more than 2^31 tiles");
        const size_t lds = LP_LUT + 256 * sizeof(float) + (size_t)T * T * TD;
        const unsigned grid = (unsigned)(ntiles < 256 * 8 ? ntiles : 256 * 8);
        hipLaunchKernelGGL(k_label_pooled, dim3(grid), dim3(LP_THREADS), lds, s, lab, H, W, D, C, present, weights, mult, T, TD, ntw, ntd, (int)ntiles, q1, q2);
    } else {
        hipLaunchKernelGGL(k_label_pooled_direct, dim3((unsigned)cdiv64((int64_t)C * q1.Ho * q1.Wo * q1.Do, 256)), dim3(256), 0, s, lab, H, W, D, C, present,
                           weights, mult, q1);
        if (g2 > 0)
            hipLaunchKernelGGL(k_label_pooled_direct, dim3((unsigned)cdiv64((int64_t)C * q2.Ho * q2.Wo * q2.Do, 256)), dim3(256), 0, s, lab, H, W, D, C, present,
                               weights, mult, q2);
    }
    return check_last("label_features_pooled");
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_label_features_pooled_f32(const float* lab, int H, int W, int D, int C, const int* present, const float* weights, float mult, int g1,
                                             float* out1, int g2, float* out2, void* stream) {
    CVX_REQUIRE(lab && present && weights && out1, "cvx_label_features_pooled_f32: null pointer");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_label_features_pooled_f32: bad extent");
    CVX_REQUIRE(C >= 1 && C <= 255, "cvx_label_features_pooled_f32: %d channels, 1 .. 255 supported (one byte per voxel)", C);
    CVX_REQUIRE(g1 >= 1 && g2 >= 0, "cvx_label_features_pooled_f32: pooling windows must be g1 >= 1, g2 >= 0 (0: no second output)");
    CVX_REQUIRE(H / g1 > 0 && W / g1 > 0 && D / g1 > 0, "cvx_label_features_pooled_f32: pooling window %d larger than the volume", g1);
    CVX_REQUIRE(g2 == 0 || (H / g2 > 0 && W / g2 > 0 && D / g2 > 0), "cvx_label_features_pooled_f32: pooling window %d larger than the volume", g2);
    CVX_REQUIRE((g2 > 0) == (out2 != nullptr), "cvx_label_features_pooled_f32: the second output goes with a second window (out2 NULL iff g2 == 0)");
    return launch_label_pooled(lab, H, W, D, C, present, weights, mult, g1, out1, g2, out2, as_stream(stream));
}
