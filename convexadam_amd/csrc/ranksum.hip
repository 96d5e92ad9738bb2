// ranksum.hip -- the rank-sum tests that end the L2R-2022 self-configuration: self_configuring/l2r3.py:262-271 calls
// scipy.stats.ranksums on every ordered pair of N "teams" with S noisy samples each and keeps (statistic > 0) & (pvalue < 0.05), 50 times
// per metric.  With equal sample sizes and no tie correction that decision is U2 >= u2_crit(S) for the integer
//     U2(i, j) = 2 #{a > b} + #{a == b} = #{a > b} + #{a >= b}        a in x_i, b in x_j, IEEE comparisons
// so the kernel counts comparisons and nothing else; the only floating point is the statement of the samples themselves.
//   cvx_ranksum_critical_u2   host: the threshold of one S, from scipy's own formula of z in float64 and libm's erfc
//   k_ranksum_better          one work-group per (repeat r, team j): x_j in LDS, the N rows x_i dealt to its four wavefronts straight from
//                             global memory (one repeat's N x S doubles stay in the L2), each lane holding KC values a_k in registers and
//                             walking x_j with broadcast 16-byte LDS reads; a wavefront reduction gives U2(r, i, j), lane 0 counts the
//                             decisions, and scores[r][j] is stored once.  No atomics, no workspace.
// x_j is padded to a multiple of four and a row's overhanging lanes are filled with NaN: a NaN compares false both ways and adds nothing,
// which is also what the contract asks of a NaN sample.
#include <limits.h>
#include <math.h>

#include "cvx_common.h"
#include "interp_f64.h"
#include "geometry_args.h"

namespace cvx {

enum { RS_THREADS = 256, RS_WAVES = RS_THREADS / 64, RS_MAX = 4096 };

// z of scipy.stats.ranksums for n1 = n2 = S and the rank sum s = U2 / 2 + S (S + 1) / 2 of the first sample, in scipy's order
static double ranksum_z(int S, long long u2) {
    const double s = (double)u2 / 2.0 + (double)((long long)S * (S + 1) / 2);
    const double expected = (double)((long long)S * (2 * S + 1)) / 2.0;
    return (s - expected) / sqrt((double)((long long)S * S * (2 * S + 1)) / 12.0);
}
static bool ranksum_significant(int S, long long u2, double p_threshold) {
    const double z = ranksum_z(S, u2);
    return z > 0.0 && erfc(fabs(z) / sqrt(2.0)) < p_threshold;
}

// the sample k of team i in repeat r as the tests compare it: sign * ((double) mean_i + scale * samples), every operation rounded
template <bool MEANS>
__device__ __forceinline__ double rs_value(const double* __restrict__ row, int k, int S, double mean, double scale, double sign) {
    if (k >= S) return __builtin_nan("");
    const double v = row[k];
    if (!MEANS) return v;
    const double p = scale * v;
    const double q = mean + p;
    return sign * q;
}

// samples [R][N][S]; scores [R][N]; u2 [R][N][N] or null; block = (r, j), 4 wavefronts, dynamic LDS: S rounded up to 4 doubles
template <int KC, bool MEANS>
__global__ __launch_bounds__(RS_THREADS) void k_ranksum_better(const double* __restrict__ samples, const float* __restrict__ means, double scale,
                                                               double sign, int N, int S, int u2_crit, int* __restrict__ scores,
                                                               int* __restrict__ u2) {
    extern __shared__ double rs_b[];
    __shared__ int rs_part[RS_WAVES];
    const int r = blockIdx.x / N, j = blockIdx.x - r * N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S4 = (S + 3) & ~3;
    const double* __restrict__ rep = samples + (size_t)r * N * S;
    {
        const double mj = MEANS ? (double)means[j] : 0.0;
        for (int k = threadIdx.x; k < S4; k += RS_THREADS) rs_b[k] = rs_value<MEANS>(rep + (size_t)j * S, k, S, mj, scale, sign);
    }
    __syncthreads();
    int better = 0;                                             // lane 0 of each wavefront: decisions of the rows it was dealt
    for (int i = wave; i < N; i += RS_WAVES) {
        const double* __restrict__ row = rep + (size_t)i * S;
        const double mi = MEANS ? (double)means[i] : 0.0;
        int cnt = 0;
        for (int k0 = 0; k0 < S; k0 += 64 * KC) {
            double a[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) a[c] = rs_value<MEANS>(row, k0 + c * 64 + lane, S, mi, scale, sign);
            int gt[KC] = {}, ge[KC] = {};
            for (int q = 0; q < S4; q += 4) {
                const double2 b01 = *reinterpret_cast<const double2*>(rs_b + q);          // every lane the same address: a broadcast
                const double2 b23 = *reinterpret_cast<const double2*>(rs_b + q + 2);
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    gt[c] += (a[c] > b01.x) + (a[c] > b01.y) + (a[c] > b23.x) + (a[c] > b23.y);
                    ge[c] += (a[c] >= b01.x) + (a[c] >= b01.y) + (a[c] >= b23.x) + (a[c] >= b23.y);
                }
            }
#pragma unroll
            for (int c = 0; c < KC; ++c) cnt += gt[c] + ge[c];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);      // at most 2 S^2 = 2^25: an int holds it
        if (lane == 0) {
            better += cnt >= u2_crit;
            if (u2) u2[((size_t)r * N + i) * N + j] = cnt;
        }
    }
    if (lane == 0) rs_part[wave] = better;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) s += rs_part[w];
        scores[(size_t)r * N + j] = s;
    }
}

template <int KC>
static void launch_ranksum(const double* samples, const float* means, double scale, double sign, int R, int N, int S, int u2_crit, int* scores,
                           int* u2, hipStream_t s) {
    const size_t lds = (size_t)((S + 3) & ~3) * sizeof(double);              // at most 32 KiB
    const dim3 grid((unsigned)(R * N)), block(RS_THREADS);
    if (means) hipLaunchKernelGGL((k_ranksum_better<KC, true>), grid, block, lds, s, samples, means, scale, sign, N, S, u2_crit, scores, u2);
    else hipLaunchKernelGGL((k_ranksum_better<KC, false>), grid, block, lds, s, samples, means, scale, sign, N, S, u2_crit, scores, u2);
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_ranksum_critical_u2(int S, double p_threshold, int* u2_crit) {
    CVX_REQUIRE(u2_crit, "cvx_ranksum_critical_u2: null pointer");
    CVX_REQUIRE(S >= 1 && S <= RS_MAX, "cvx_ranksum_critical_u2: bad sample count %d (1..%d)", S, (int)RS_MAX);
    CVX_REQUIRE(p_threshold > 0.0 && p_threshold < 1.0, "cvx_ranksum_critical_u2: bad p threshold %g (inside (0, 1))", p_threshold);
    // z grows with U2 and erfc falls with |z|: the significant values are an upper stretch of (S^2, 2 S^2], found by bisection
    const long long top = 2LL * S * S;
    if (!ranksum_significant(S, top, p_threshold)) {
        *u2_crit = (int)(top + 1);                               // "never": S = 1 and S = 2 at 0.05
        return CVX_OK;
    }
    long long lo = (long long)S * S, hi = top;                   // lo: not significant (z = 0); hi: significant
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (ranksum_significant(S, mid, p_threshold)) hi = mid;
        else lo = mid;
    }
    *u2_crit = (int)hi;
    return CVX_OK;
}

extern "C" int cvx_ranksum_better_f64(const double* samples, const float* means, double scale, double sign, int R, int N, int S, int u2_crit,
                                      int* scores, int* u2, void* stream) {
    CVX_REQUIRE(samples && scores, "cvx_ranksum_better_f64: null pointer");
    CVX_REQUIRE(R >= 1 && N >= 1 && S >= 1, "cvx_ranksum_better_f64: bad extent (R %d, N %d, S %d)", R, N, S);
    CVX_REQUIRE(N <= RS_MAX && S <= RS_MAX, "cvx_ranksum_better_f64: bad extent (N %d, S %d: at most %d each)", N, S, (int)RS_MAX);
    const uint64_t n_samples = (uint64_t)R * N * S, n_u2 = (uint64_t)R * N * N;
    CVX_REQUIRE(n_samples <= (uint64_t)INT_MAX && (!u2 || n_u2 <= (uint64_t)INT_MAX),
                "cvx_ranksum_better_f64: more than 2^31 - 1 elements (R %d, N %d, S %d)", R, N, S);
    CVX_REQUIRE(u2_crit >= 0 && (long long)u2_crit <= 2LL * S * S + 1, "cvx_ranksum_better_f64: bad threshold %d (0..2 S^2 + 1 = %lld)", u2_crit,
                2LL * S * S + 1);
    CVX_REQUIRE(!means || (isfinite(scale) && isfinite(sign)), "cvx_ranksum_better_f64: non-finite scale or sign");
    CVX_REQUIRE(((uintptr_t)samples & 7) == 0 && ((uintptr_t)means & 3) == 0 && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)u2 & 3) == 0,
                "cvx_ranksum_better_f64: a buffer is not aligned to its element");
    const size_t sbytes = (size_t)n_samples * 8, obytes = (size_t)R * N * 4, ubytes = (size_t)n_u2 * 4, mbytes = (size_t)N * 4;
    const Span outs[2] = {{scores, obytes}, {u2, ubytes}}, in_samples[1] = {{samples, sbytes}}, in_means[1] = {{means, mbytes}};
    const Overlaps ov = find_overlaps(outs, in_samples);
    CVX_REQUIRE(ov.out < 0 && ov.a < 0, "cvx_ranksum_better_f64: scores, u2 and samples overlap");
    CVX_REQUIRE(find_overlaps(outs, in_means).out < 0, "cvx_ranksum_better_f64: an output overlaps means");
    hipStream_t s = as_stream(stream);
    if (S <= 64) launch_ranksum<1>(samples, means, scale, sign, R, N, S, u2_crit, scores, u2, s);
    else if (S <= 128) launch_ranksum<2>(samples, means, scale, sign, R, N, S, u2_crit, scores, u2, s);
    else launch_ranksum<4>(samples, means, scale, sign, R, N, S, u2_crit, scores, u2, s);
    return check_last("ranksum_better");
}
