// lts_common.h -- what the least-trimmed fits share (rigid.hip::k_rigid_lts, affine.hip::k_affine_lts): one 1024-thread workgroup, the
// fixed-order float64 workgroup sum, the float32 residual pattern, and the selection of the n/2 points with the smallest residuals (radix
// select of the n/2-th smallest bit pattern, NaN last, ties to the lowest index through an ordered ballot scan).  The two kernels differ
// in the model they solve per fit and in nothing else.
// Every global word a thread reads back (patterns, set mask) is one it wrote itself: the strided walk gives point i to thread i % 1024 in
// every pass, so the passes need nothing beyond the workgroup barriers between them.
#pragma once
#include "cvx_common.h"

namespace cvx {

constexpr int LTS_THREADS = 1024;
constexpr int LTS_WAVES = LTS_THREADS / 64;
constexpr int64_t LTS_MAX_N = (int64_t)1 << 28;

// Workgroup sum of M doubles in a fixed order; every thread gets the M totals in out[] (LDS).
template <int M>
__device__ __forceinline__ void wg_sum(double (&v)[M], double* red, double* out) {
    for (int off = 32; off >= 1; off >>= 1)
        for (int m = 0; m < M; ++m) v[m] += __shfl_xor(v[m], off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int m = 0; m < M; ++m) red[wave * M + m] = v[m];
    cvx_barrier();
    if (threadIdx.x < M) {
        double s = red[threadIdx.x];
        for (int w2 = 1; w2 < LTS_WAVES; ++w2) s += red[w2 * M + threadIdx.x];
        out[threadIdx.x] = s;
    }
    cvx_barrier();
}

// The bin b of an LDS histogram (nbins = LTS_THREADS * PER) with cum(< b) < k <= cum(<= b), 1 <= k <= total: res[0] = b,
// res[1] = cum(< b).  Ends with a barrier.
template <int PER>
__device__ __forceinline__ void find_bin(const unsigned* hist, unsigned k, unsigned* wsum, unsigned* res) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned c[PER], local = 0;
    for (int j = 0; j < PER; ++j) { c[j] = hist[tid * PER + j]; local += c[j]; }
    unsigned x = local;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    cvx_barrier();
    unsigned cum = x - local;
    for (int w2 = 0; w2 < wave; ++w2) cum += wsum[w2];
    for (int j = 0; j < PER; ++j) {
        if (cum < k && k <= cum + c[j]) { res[0] = (unsigned)(tid * PER + j); res[1] = cum; }
        cum += c[j];
    }
    cvx_barrier();
}

// Bit pattern of the float32 residual || m - f X || over all four columns, X given by its columns: column a of X is Xc[4 a .. 4 a + 3]
// (for the rigid fit the rows of T).  LAST_IS_E3: column 3 of X is (0, 0, 0, 1), its term is m[3] - f[3].  Non-negative floats order like
// their bits; NaN is mapped to 0x7fffffff so that it sorts last, as in torch.topk.
template <bool LAST_IS_E3>
__device__ __forceinline__ unsigned residual_bits(const float* __restrict__ f, const float* __restrict__ m, const float* Xc) {
    const float f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
    float s = 0.0f;
    for (int a = 0; a < (LAST_IS_E3 ? 3 : 4); ++a) {
        float p = f0 * Xc[4 * a];
        p = fmaf(f1, Xc[4 * a + 1], p);
        p = fmaf(f2, Xc[4 * a + 2], p);
        p = fmaf(f3, Xc[4 * a + 3], p);
        const float e = m[a] - p;
        s = s + e * e;
    }
    if (LAST_IS_E3) {
        const float e3 = m[3] - f3;
        s = s + e3 * e3;
    }
    const float r = sqrtf(s);
    return r != r ? 0x7fffffffu : __float_as_uint(r);
}

// mode 0: every point; 1: pattern <= thr; 2: the byte mask
__device__ __forceinline__ bool in_set(int mode, int i, const unsigned* rbits, const unsigned char* sel, unsigned thr) {
    return mode == 0 ? true : (mode == 1 ? rbits[i] <= thr : sel[i] != 0);
}

// LDS of the selection
struct LtsSelectLds { unsigned hist[2048], wsum[LTS_WAVES], res[2]; };

// The K = n / 2 points with the smallest patterns pattern(i), i < n: writes rbits[i] = pattern(i), finds the K-th smallest pattern thr by a
// three-pass radix select (11 + 11 + 10 bits, LDS histograms) and returns the mode of in_set for the next fit: 1 when the set is simply
// {r <= thr} (every r == thr point is needed; no pass is spent), else 2 after an ordered ballot scan over chunks of LTS_THREADS points has
// written the set -- {r < thr} plus the LOWEST-INDEX points with r == thr until K are chosen -- as the byte mask sel.  Called by every
// thread of the workgroup; starts and ends with a barrier.
template <typename Pattern>
__device__ __forceinline__ int lts_select(int n, int K, unsigned* rbits, unsigned char* sel, LtsSelectLds& L, unsigned& thr, Pattern pattern) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* hist = L.hist;
    unsigned* wsum = L.wsum;
    unsigned* res = L.res;
    for (int j = tid; j < 2048; j += LTS_THREADS) hist[j] = 0u;
    cvx_barrier();
    for (int i = tid; i < n; i += LTS_THREADS) {
        const unsigned b = pattern(i);
        rbits[i] = b;
        atomicAdd(&hist[b >> 21], 1u);
    }
    cvx_barrier();
    find_bin<2>(hist, (unsigned)K, wsum, res);
    const unsigned b1 = res[0], below1 = res[1];
    for (int j = tid; j < 2048; j += LTS_THREADS) hist[j] = 0u;
    cvx_barrier();
    for (int i = tid; i < n; i += LTS_THREADS) {
        const unsigned b = rbits[i];
        if ((b >> 21) == b1) atomicAdd(&hist[(b >> 10) & 0x7ffu], 1u);
    }
    cvx_barrier();
    find_bin<2>(hist, (unsigned)K - below1, wsum, res);
    const unsigned pre = (b1 << 11) | res[0], below2 = res[1];
    for (int j = tid; j < 1024; j += LTS_THREADS) hist[j] = 0u;
    cvx_barrier();
    for (int i = tid; i < n; i += LTS_THREADS) {
        const unsigned b = rbits[i];
        if ((b >> 10) == pre) atomicAdd(&hist[b & 0x3ffu], 1u);
    }
    cvx_barrier();
    find_bin<1>(hist, (unsigned)K - below1 - below2, wsum, res);
    thr = (pre << 10) | res[0];
    const unsigned need = (unsigned)K - below1 - below2 - res[1], eq = hist[res[0]];
    cvx_barrier();                                                          // hist / res are rewritten by the next fit
    if (eq == need) return 1;
    // ties at the threshold: the lowest-index `need` of them, by an ordered scan over chunks of LTS_THREADS points
    unsigned run = 0;
    for (int base = 0; base < n; base += LTS_THREADS) {
        const int i = base + tid;
        const unsigned b = i < n ? rbits[i] : 0xffffffffu;
        const bool e = b == thr;
        const unsigned long long bal = __ballot(e);
        const unsigned before = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = (unsigned)__popcll(bal);
        cvx_barrier();
        unsigned wb = 0, all = 0;
        for (int w2 = 0; w2 < LTS_WAVES; ++w2) {
            if (w2 < wave) wb += wsum[w2];
            all += wsum[w2];
        }
        if (i < n) sel[i] = (unsigned char)(b < thr || (e && run + wb + before < need));
        run += all;
        cvx_barrier();
    }
    return 2;
}

// residual bits, inlier selection, the status word: the workspace of both fits
struct LtsWs { unsigned* rbits; unsigned char* sel; int* status; };
static inline LtsWs lts_layout(Carver& cv, int64_t n) { return LtsWs{cv.take<unsigned>((size_t)n), cv.take<unsigned char>((size_t)n), cv.take<int>(1)}; }

}  // namespace cvx
