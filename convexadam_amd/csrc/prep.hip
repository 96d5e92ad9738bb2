// prep.hip -- the nnU-Net preprocessing helpers (convex_adam_utils.py:142-170, 240-259; include/convexadam_prep.h):
//   k_prep_pass<1|2|3>     one read of the volume each: float64 moments in a fixed order and / or one histogram pass of the radix select
//   k_prep_finish<1|2|3>   one workgroup between the passes: adds the span partials, turns counts into the next key prefix and the residual
//                          rank of every requested order statistic, and at the end writes the parameter block { mean, std, lo, hi }
//   k_prep_normalise*      (clamp(x, lo, hi) - mean) / std with the block read from the device (or from launch arguments)
//   k_mask_init / k_mask_sweep(_row) / k_mask_final   the non-zero mask, its hole filling by line sweeps (along D in 8- or 4-byte words where
//                          the row length allows) and its box
// The ORDER of the float64 additions is the contract, and it is cvx_field_mean_f64's (fieldmean.hip), for one accumulator:
//   span b owns elements [b S, (b + 1) S), S = 256 K, K = 16; thread t adds its elements b S + k 256 + t, k = 0 .. K - 1, in that order into
//   an accumulator started at 0.0 (an element that does not count adds nothing); the 256 accumulators are combined by the stride-halving tree
//   (s = 128, 64, .., 1: acc[t] += acc[t + s] for t < s; LDS across wavefronts, __shfl_down inside one); the finish lets thread t add
//   partials t, t + 256, .. in order from 0.0 and runs the same tree.  Pass 1 adds (double)x, pass 2 d * d with d = (double)x - mean.
//   A workgroup walks PR_G consecutive spans (one tree each) so that it zeroes and merges its LDS histograms once per 16 384 elements.
// Radix select: key = the monotone 32-bit image of a float (-0.0 on +0.0's key), 11 + 11 + 10 bits.  The requested ranks have reached up to
//   four DISTINCT prefixes, one histogram each; a key shares at most one of them, so a pass takes one voting step per element -- bins
//   privatised in LDS, merged with integer atomics (sums of integers do not depend on the arrival order).  A clamped CT puts most of its
//   voxels on ONE key: when more than eight lanes of a wavefront vote, the bin of the first pending lane is peeled twice (one lane adds the
//   population count of the ballot), so the common bin costs one atomic per wavefront, not 64 serialised ones; what is left goes lane by lane.
#include <limits.h>
#include <math.h>

#include "cvx_common.h"
#include "interp_f64.h"
#include "geometry_args.h"
#include "convexadam_prep.h"

namespace cvx {

constexpr int PR_THREADS = 256;                     // the tree below is written for 256 threads = 4 wavefronts of 64
constexpr int PR_K = 16;                            // elements per thread and span
constexpr int PR_SPAN = PR_THREADS * PR_K;          // S
constexpr int PR_G = 4;                             // spans per workgroup
constexpr int PR_BITS1 = 11, PR_BITS2 = 11, PR_BITS3 = 10;
constexpr int PR_BINS1 = 1 << PR_BITS1, PR_BINS2 = 1 << PR_BITS2, PR_BINS3 = 1 << PR_BITS3;
constexpr int PR_RANKS = 4;                         // below / above of two quantiles

// what the passes hand to each other, on the device
struct PrepState {
    unsigned prefix[PR_RANKS];        // key bits decided so far, per rank
    unsigned resid[PR_RANKS];         // rank among the keys that share that prefix
    int slot[PR_RANKS];               // which histogram of the next pass serves the rank
    unsigned slot_prefix[PR_RANKS];   // the distinct prefixes, one histogram each
    int nslots;
    unsigned has_nan;
    long long count;
    double mean, ss;
};
struct PrepRanks { unsigned k[PR_RANKS]; float w[2]; };

// workspace: ONE layout for the size query and the launcher.  `zeroed` (state + histograms) is cleared at the start of every call
struct PrepWs { PrepState* st; unsigned *h1, *h2, *h3; double *psum, *pss; long long* pcnt; size_t zeroed_bytes; };
static PrepWs prep_layout(Carver& c, size_t nspans) {
    PrepWs w;
    w.st = c.take<PrepState>(1);
    w.h1 = c.take<unsigned>(PR_BINS1);
    w.h2 = c.take<unsigned>((size_t)PR_RANKS * PR_BINS2);
    w.h3 = c.take<unsigned>((size_t)PR_RANKS * PR_BINS3);
    w.zeroed_bytes = c.used;
    w.psum = c.take<double>(nspans);
    w.pss = c.take<double>(nspans);
    w.pcnt = c.take<long long>(nspans);
    return w;
}

__device__ __forceinline__ unsigned pr_key(float x) {
    unsigned b = __float_as_uint(x);
    if (x == 0.0f) b = 0u;                                   // -0.0 sorts with +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float pr_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// acc[t] += acc[t + s] for s = 128 .. 1, t < s; thread 0 ends with the totals.  The caller puts a barrier before it reuses sm / sn
__device__ __forceinline__ void pr_tree(double& a, long long& n, double* sm, long long* sn) {
    const int t = threadIdx.x;
    sm[t] = a;
    sn[t] = n;
    cvx_barrier();
    if (t < 128) {
        a += sm[t + 128];
        sm[t] = a;
        n += sn[t + 128];
        sn[t] = n;
    }
    cvx_barrier();
    if (t < 64) {                                   // wavefront 0, whole
        a += sm[t + 64];
        n += sn[t + 64];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {         // lane t < s reads lane t + s < 2 s, which the step before left valid
            a += __shfl_down(a, s, 64);
            n += __shfl_down(n, s, 64);
        }
    }
}

// one count into h[bin] for every lane with `on`; every lane of the wavefront calls it.  More than eight lanes voting: the bin of the first
// pending lane is peeled (twice) before the rest goes lane by lane; eight or fewer go straight to the atomics
__device__ __forceinline__ void pr_hist_add(unsigned* h, unsigned bin, bool on) {
    unsigned long long todo = __builtin_amdgcn_ballot_w64(on);
    if (!todo) return;
    const int lane = threadIdx.x & 63;
    const int peels = __builtin_popcountll(todo) > 8 ? 2 : 0;       // a few scattered lanes: straight to the atomics
    for (int it = 0; it < peels; ++it) {
        if (!todo) break;
        const int leader = __builtin_ctzll(todo);
        const unsigned b0 = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);     // leader is wave-uniform
        const unsigned long long m = __builtin_amdgcn_ballot_w64(on && bin == b0) & todo;
        if (lane == leader) atomicAdd(&h[b0], (unsigned)__builtin_popcountll(m));
        todo &= ~m;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&h[bin], 1u);
}

template <int PASS>
__global__ __launch_bounds__(PR_THREADS) void k_prep_pass(const float* __restrict__ x, size_t n, int flags, float lo, float hi, int nq,
                                                          PrepState* __restrict__ st, double* __restrict__ part, long long* __restrict__ pcnt,
                                                          unsigned* __restrict__ hist, size_t nspans) {
    constexpr int BINS = PASS == 1 ? PR_BINS1 : (PASS == 2 ? PR_BINS2 : PR_BINS3);
    constexpr int SLOTS = PASS == 1 ? 1 : PR_RANKS;
    __shared__ double sm[PR_THREADS];
    __shared__ long long sn[PR_THREADS];
    __shared__ unsigned lh[SLOTS * BINS];
    const int t = threadIdx.x;
    const bool clamp = flags & CVX_PREP_CLAMP, positive = flags & CVX_PREP_POSITIVE;
    __shared__ unsigned sp[PR_RANKS];
    const int nslots = nq ? (PASS == 1 ? 1 : st->nslots) : 0;
    if (t < PR_RANKS) sp[t] = (PASS > 1 && t < nslots) ? st->slot_prefix[t] : 0u;
    for (int i = t; i < nslots * BINS; i += PR_THREADS) lh[i] = 0u;
    const double mean = PASS == 2 ? st->mean : 0.0;
    cvx_barrier();
    for (int g = 0; g < PR_G; ++g) {
        const size_t span = (size_t)blockIdx.x * PR_G + g;
        if (span >= nspans) break;                  // the same for every thread of the workgroup
        double a = 0.0;
        long long c = 0;
        const size_t v0 = span * PR_SPAN + t;
        float ys[PR_K];                             // the span's 16 loads are in flight together; the additions below keep their order
#pragma unroll
        for (int k = 0; k < PR_K; ++k) {
            const size_t v = v0 + (size_t)k * PR_THREADS;
            ys[k] = v < n ? x[v] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < PR_K; ++k) {            // no early exit: the histogram step votes across the whole wavefront
            const bool valid = v0 + (size_t)k * PR_THREADS < n;
            float y = ys[k];
            if (clamp) {
                y = y < lo ? lo : y;
                y = y > hi ? hi : y;
            }
            const bool in = valid && (!positive || y > 0.0f);
            if (PASS == 1 && in) {
                a += (double)y;
                c += 1;
            }
            if (PASS == 2 && in) {
                const double d = (double)y - mean;
                a += d * d;
            }
            if (nslots) {
                const unsigned key = pr_key(y);
                if (PASS == 1) {
                    if (valid && y != y) atomicOr(&st->has_nan, 1u);
                    pr_hist_add(lh, key >> (32 - PR_BITS1), valid);
                } else {
                    const unsigned pre = PASS == 2 ? key >> (32 - PR_BITS1) : key >> PR_BITS3;
                    const unsigned bin = PASS == 2 ? (key >> PR_BITS3) & (PR_BINS2 - 1) : key & (PR_BINS3 - 1);
                    int slot = -1;                   // the prefixes are distinct: a key counts in at most one histogram
                    for (int u = 0; u < nslots; ++u) slot = pre == sp[u] ? u : slot;
                    pr_hist_add(lh, (unsigned)(slot < 0 ? 0 : slot) * BINS + bin, valid && slot >= 0);
                }
            }
        }
        if (PASS < 3) {
            pr_tree(a, c, sm, sn);
            if (t == 0) {
                part[span] = a;
                if (PASS == 1) pcnt[span] = c;
            }
            cvx_barrier();                          // sm / sn are free again
        }
    }
    cvx_barrier();
    for (int i = t; i < nslots * BINS; i += PR_THREADS) {
        const unsigned cnt = lh[i];
        if (cnt) atomicAdd(&hist[i], cnt);
    }
}

// wavefront `r` finds the bin that holds rank k of histogram h and the rank inside that bin.  A lane owns BINS / 64 consecutive bins and
// loads them all before it uses one (one wavefront has nothing else to hide a chain of dependent loads behind)
template <int BINS>
__device__ __forceinline__ void pr_wave_select(const unsigned* __restrict__ h, unsigned k, unsigned* bin_out, unsigned* resid_out) {
    constexpr int PER = BINS / 64;
    static_assert(PER % 4 == 0, "a lane's bins as 16-byte quads");
    const int lane = threadIdx.x & 63, base = lane * PER;
    unsigned c[PER];
#pragma unroll
    for (int i = 0; i < PER; i += 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(h + base + i);          // histograms are carved at multiples of 256 bytes
        c[i] = q.x; c[i + 1] = q.y; c[i + 2] = q.z; c[i + 3] = q.w;
    }
    unsigned s = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) s += c[i];
    unsigned incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    const unsigned excl = incl - s;
    if (k >= excl && k < incl) {                    // exactly one lane
        unsigned r = k - excl, bin = 0, res = 0;
        bool found = false;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const bool here = !found && r < c[i];
            bin = here ? (unsigned)(base + i) : bin;
            res = here ? r : res;
            found = found || here;
            r -= found ? 0u : c[i];
        }
        *bin_out = bin;
        *resid_out = res;
    }
}

__device__ __forceinline__ void pr_write_params(const PrepState* st, float qlo, float qhi, float* __restrict__ params, double* __restrict__ moments3) {
    const long long count = st->count;
    const double mean = st->mean, ss = st->ss;
    params[0] = (float)mean;
    params[1] = count > 1 ? (float)sqrt(ss / (double)(count - 1)) : __uint_as_float(0x7fc00000u);      // torch: NaN for fewer than two elements
    params[2] = qlo;
    params[3] = qhi;
    if (moments3) {
        moments3[0] = (double)count;
        moments3[1] = mean;
        moments3[2] = ss;
    }
}

template <int PASS>
__global__ __launch_bounds__(PR_THREADS) void k_prep_finish(const double* __restrict__ part, const long long* __restrict__ pcnt, size_t nspans,
                                                            long long n, int flags, int nq, PrepRanks rk, PrepState* __restrict__ st,
                                                            const unsigned* __restrict__ hist, float* __restrict__ params,
                                                            double* __restrict__ moments3) {
    constexpr int BINS = PASS == 1 ? PR_BINS1 : (PASS == 2 ? PR_BINS2 : PR_BINS3);
    constexpr int BITS = PASS == 1 ? PR_BITS1 : (PASS == 2 ? PR_BITS2 : PR_BITS3);
    __shared__ double sm[PR_THREADS];
    __shared__ long long sn[PR_THREADS];
    __shared__ unsigned sbin[PR_RANKS], sres[PR_RANKS];
    const int t = threadIdx.x;
    if (PASS < 3) {
        double a = 0.0;
        long long c = 0;
        for (size_t i0 = t; i0 < nspans; i0 += 8 * PR_THREADS) {      // eight loads in flight, added in the order t, t + 256, ..
            double pa[8];
            long long pc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const size_t i = i0 + (size_t)j * PR_THREADS;
                pa[j] = i < nspans ? part[i] : 0.0;                      // + 0.0 leaves an accumulator that started at + 0.0 as it is
                pc[j] = (PASS == 1 && i < nspans) ? pcnt[i] : 0;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a += pa[j];
                c += pc[j];
            }
        }
        pr_tree(a, c, sm, sn);
        if (t == 0) {
            if (PASS == 1) {
                const long long count = (flags & CVX_PREP_POSITIVE) ? c : n;
                st->count = count;
                st->mean = a / (double)count;
            } else {
                st->ss = a;
            }
        }
    }
    if (t < PR_RANKS) { sbin[t] = 0u; sres[t] = 0u; }
    cvx_barrier();
    if (nq) {
        const int r = t >> 6;                       // one wavefront per rank
        const unsigned k = PASS == 1 ? rk.k[r] : st->resid[r];
        const unsigned* h = PASS == 1 ? hist : hist + (size_t)st->slot[r] * BINS;
        pr_wave_select<BINS>(h, k, &sbin[r], &sres[r]);
    }
    cvx_barrier();
    if (t != 0) return;
    if (!nq) {
        if (PASS == 2) pr_write_params(st, -INFINITY, INFINITY, params, moments3);
        return;
    }
    unsigned key[PR_RANKS];
    for (int r = 0; r < PR_RANKS; ++r) key[r] = PASS == 1 ? sbin[r] : ((st->prefix[r] << BITS) | sbin[r]);
    if (PASS < 3) {
        int ns = 0;
        for (int r = 0; r < PR_RANKS; ++r) {
            st->prefix[r] = key[r];
            st->resid[r] = sres[r];
            int u = 0;
            while (u < ns && st->slot_prefix[u] != key[r]) ++u;
            if (u == ns) st->slot_prefix[ns++] = key[r];
            st->slot[r] = u;
        }
        st->nslots = ns;
        return;
    }
    float q[2];
    for (int j = 0; j < 2; ++j) {
        const float a = pr_unkey(key[2 * j]), b = pr_unkey(key[2 * j + 1]), w = rk.w[j];
        q[j] = w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w);        // torch's lerp
        if (st->has_nan) q[j] = __uint_as_float(0x7fc00000u);
    }
    pr_write_params(st, q[0], q[1], params, moments3);
}

// ---- the elementwise step ---------------------------------------------------------------------------------------------------------
struct NormParams { float mean, std, lo, hi; };
template <int MODE>
__device__ __forceinline__ float pr_norm(float x, const NormParams& p) {
    if (MODE == 0) {
        float t = x < p.lo ? p.lo : x;
        t = t > p.hi ? p.hi : t;
        return fdiv(t - p.mean, p.std);
    }
    return x > 0.0f ? fdiv(x - p.mean, p.std + 1e-8f) : 0.0f;
}
// VEC: both pointers 16-byte aligned -- thread i takes quad i, the last n % 4 elements go one per thread behind the quads
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void k_prep_normalise(const float* x, size_t n, const float* __restrict__ params, NormParams hostp, float* out) {
    NormParams p = hostp;
    if (params) { p.mean = params[0]; p.std = params[1]; p.lo = params[2]; p.hi = params[3]; }
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const size_t nquads = n / 4;
        if (i < nquads) {
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            float4 o;
            o.x = pr_norm<MODE>(v.x, p); o.y = pr_norm<MODE>(v.y, p); o.z = pr_norm<MODE>(v.z, p); o.w = pr_norm<MODE>(v.w, p);
            reinterpret_cast<float4*>(out)[i] = o;
        } else {
            const size_t e = nquads * 4 + (i - nquads);
            if (e < n) out[e] = pr_norm<MODE>(x[e], p);
        }
    } else if (i < n) {
        out[i] = pr_norm<MODE>(x[i], p);
    }
}

// ---- non-zero mask, hole filling, box ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mask_init(const float* __restrict__ data, int C, int H, int W, int D, int ndim, unsigned char* __restrict__ mask,
                                                   unsigned char* __restrict__ reached) {
    const size_t V = (size_t)H * W * D, v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    bool m = false;
    for (int c = 0; c < C; ++c) m = m || (data[(size_t)c * V + v] != 0.0f);
    const int xx = (int)(v % D), yy = (int)((v / D) % W), zz = (int)(v / ((size_t)D * W));
    const bool face = xx == 0 || xx == D - 1 || yy == 0 || yy == W - 1 || (ndim == 3 && (zz == 0 || zz == H - 1));
    mask[v] = m ? 1 : 0;
    reached[v] = (!m && face) ? 1 : 0;
}

// one thread per line of `len` voxels `step` apart; line l starts at (l / inner) * outer + (l % inner).  Lines of one launch are disjoint
__global__ __launch_bounds__(128) void k_mask_sweep(const unsigned char* __restrict__ mask, unsigned char* __restrict__ reached, int len, size_t step,
                                                    size_t nlines, size_t inner, size_t outer, unsigned* __restrict__ changed) {
    const size_t l = (size_t)blockIdx.x * 128 + threadIdx.x;
    if (l >= nlines) return;
    const size_t base = (l / inner) * outer + (l % inner);
    bool carry = false, any = false;
    for (int i = 0; i < len; ++i) {
        const size_t p = base + (size_t)i * step;
        const bool r = reached[p] != 0;
        carry = !mask[p] && (carry || r);
        if (carry && !r) { reached[p] = 1; any = true; }
    }
    carry = false;
    for (int i = len - 1; i >= 0; --i) {
        const size_t p = base + (size_t)i * step;
        const bool r = reached[p] != 0;
        carry = !mask[p] && (carry || r);
        if (carry && !r) { reached[p] = 1; any = true; }
    }
    if (any) atomicOr(changed, 1u);
}

// the same walks along D, where a line is contiguous: the thread reads its line in words of NB bytes (D % NB == 0, both arrays aligned to
// NB) instead of single bytes 64 cache lines apart across the wavefront, and stores a word of `reached` only when it changed
template <typename WORD>
__global__ __launch_bounds__(128) void k_mask_sweep_row(const unsigned char* __restrict__ mask, unsigned char* __restrict__ reached, int D, size_t nlines,
                                                        unsigned* __restrict__ changed) {
    constexpr int NB = (int)sizeof(WORD);
    const size_t l = (size_t)blockIdx.x * 128 + threadIdx.x;
    if (l >= nlines) return;
    const WORD* m = reinterpret_cast<const WORD*>(mask + l * (size_t)D);
    WORD* r = reinterpret_cast<WORD*>(reached + l * (size_t)D);
    const int nw = D / NB;
    bool carry = false, any = false;
    for (int i = 0; i < nw; ++i) {
        const WORD mw = m[i], rw = r[i];
        WORD out = rw;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const bool rb = ((rw >> (8 * b)) & 0xff) != 0, mb = ((mw >> (8 * b)) & 0xff) != 0;
            carry = !mb && (carry || rb);
            if (carry && !rb) out |= (WORD)1 << (8 * b);
        }
        if (out != rw) { r[i] = out; any = true; }
    }
    carry = false;
    for (int i = nw - 1; i >= 0; --i) {
        const WORD mw = m[i], rw = r[i];
        WORD out = rw;
#pragma unroll
        for (int b = NB - 1; b >= 0; --b) {
            const bool rb = ((rw >> (8 * b)) & 0xff) != 0, mb = ((mw >> (8 * b)) & 0xff) != 0;
            carry = !mb && (carry || rb);
            if (carry && !rb) out |= (WORD)1 << (8 * b);
        }
        if (out != rw) { r[i] = out; any = true; }
    }
    if (any) atomicOr(changed, 1u);
}

__global__ void k_box_init(int* __restrict__ box6, long long* __restrict__ count) {
    if (threadIdx.x < 6) box6[threadIdx.x] = (threadIdx.x & 1) ? 0 : INT_MAX;
    if (threadIdx.x == 6 && count) *count = 0;
}

constexpr int MB_PER = 16;                          // voxels per thread of k_mask_final
// FILL: mask = mask | !reached first.  Then the box and the count of the set voxels: wavefront shuffles, LDS across the four wavefronts, and
// per workgroup one atomicAdd of the count and an atomicMin / atomicMax only where the bound it read (possibly stale, which costs a
// redundant atomic and never a wrong one: the bounds move one way) is not yet as wide -- a few hundred atomics per launch, not one set per wavefront
template <bool FILL>
__global__ __launch_bounds__(256) void k_mask_final(unsigned char* mask, const unsigned char* __restrict__ reached, int H, int W, int D, int* box6,
                                                    unsigned long long* __restrict__ count) {
    __shared__ int slo[3], shi[3];
    __shared__ unsigned scnt;
    if (threadIdx.x < 3) { slo[threadIdx.x] = INT_MAX; shi[threadIdx.x] = 0; }
    if (threadIdx.x == 3) scnt = 0u;
    cvx_barrier();
    const size_t V = (size_t)H * W * D, v0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * MB_PER;
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {0, 0, 0};
    unsigned cnt = 0;
    // the coordinates of v0 by one pair of 32-bit divisions (V < 2^31), then counted up voxel by voxel
    const unsigned u0 = v0 < V ? (unsigned)v0 : 0u, row = u0 / (unsigned)D;
    int c[3] = {(int)(row / (unsigned)W), (int)(row % (unsigned)W), (int)(u0 % (unsigned)D)};
    for (int j = 0; j < MB_PER; ++j) {
        const size_t v = v0 + j;
        if (v >= V) break;
        bool m = mask[v] != 0;
        if (FILL) {
            m = m || !reached[v];
            mask[v] = m ? 1 : 0;
        }
        if (m) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = c[a] < lo[a] ? c[a] : lo[a];
                hi[a] = c[a] + 1 > hi[a] ? c[a] + 1 : hi[a];
            }
            cnt += 1;
        }
        if (++c[2] == D) {
            c[2] = 0;
            if (++c[1] == W) { c[1] = 0; ++c[0]; }
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int l2 = __shfl_xor(lo[a], s, 64), h2 = __shfl_xor(hi[a], s, 64);
            lo[a] = l2 < lo[a] ? l2 : lo[a];
            hi[a] = h2 > hi[a] ? h2 : hi[a];
        }
        cnt += __shfl_xor(cnt, s, 64);
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(&slo[a], lo[a]);
            atomicMax(&shi[a], hi[a]);
        }
        atomicAdd(&scnt, cnt);
    }
    cvx_barrier();
    if (threadIdx.x < 3 && scnt) {
        const int a = threadIdx.x;
        if (slo[a] < *(volatile int*)&box6[2 * a]) atomicMin(&box6[2 * a], slo[a]);
        if (shi[a] > *(volatile int*)&box6[2 * a + 1]) atomicMax(&box6[2 * a + 1], shi[a]);
    }
    if (threadIdx.x == 3 && scnt && count) atomicAdd(count, (unsigned long long)scnt);
}

struct MaskWs { unsigned char* reached; unsigned* changed; };
static MaskWs mask_layout(Carver& c, size_t V) {
    MaskWs w;
    w.reached = c.take<unsigned char>(V);
    w.changed = c.take<unsigned>(1);
    return w;
}

}  // namespace cvx

using namespace cvx;

extern "C" size_t cvx_prep_stats_workspace_bytes(long long n) {
    if (n < 1 || n > (long long)INT_MAX) {
        fail(CVX_ERR_INVALID_ARG, "cvx_prep_stats_workspace_bytes: n = %lld (1 .. 2^31 - 1)", n);
        return 0;
    }
    Carver m;
    prep_layout(m, (size_t)cdiv64(n, PR_SPAN));
    return ws_query(m);
}

static bool prep_rank(float q, long long n, unsigned* below, unsigned* above, float* w) {
    if (!(q >= 0.0f && q <= 1.0f)) return false;
    if (n <= (1LL << 24)) {                         // torch.quantile's own arithmetic
        const float rank = q * (float)(n - 1);
        const float fl = floorf(rank);
        *below = (unsigned)fl;
        *above = (unsigned)ceilf(rank);
        *w = rank - fl;
    } else {                                        // the one extension: torch refuses such an input
        const double rank = (double)q * (double)(n - 1);
        const double fl = floor(rank);
        *below = (unsigned)fl;
        *above = (unsigned)ceil(rank);
        *w = (float)(rank - fl);
    }
    return *above < (unsigned long long)n;
}

extern "C" int cvx_prep_stats_f32(const float* x, long long n, int flags, float clamp_lo, float clamp_hi, int n_quantiles, float q0, float q1,
                                  float* params, double* moments3, void* workspace, size_t workspace_bytes, void* stream) {
    CVX_REQUIRE(x && params, "cvx_prep_stats_f32: null pointer (x or params)");
    CVX_REQUIRE(n >= 1 && n <= (long long)INT_MAX, "cvx_prep_stats_f32: bad extent (n = %lld, 1 .. 2^31 - 1)", n);
    CVX_REQUIRE((flags & ~(CVX_PREP_CLAMP | CVX_PREP_POSITIVE)) == 0, "cvx_prep_stats_f32: unknown flag bits (%d)", flags);
    CVX_REQUIRE(n_quantiles == 0 || n_quantiles == 2, "cvx_prep_stats_f32: n_quantiles must be 0 or 2 (%d)", n_quantiles);
    CVX_REQUIRE(!(n_quantiles && (flags & CVX_PREP_POSITIVE)), "cvx_prep_stats_f32: quantiles of the positive elements only are not built");
    CVX_REQUIRE(!(flags & CVX_PREP_CLAMP) || clamp_lo <= clamp_hi, "cvx_prep_stats_f32: clamp bounds (%g, %g)", (double)clamp_lo, (double)clamp_hi);
    PrepRanks rk = {};
    if (n_quantiles) {
        CVX_REQUIRE(prep_rank(q0, n, &rk.k[0], &rk.k[1], &rk.w[0]) && prep_rank(q1, n, &rk.k[2], &rk.k[3], &rk.w[1]),
                    "cvx_prep_stats_f32: quantile fractions outside [0, 1] (%g, %g)", (double)q0, (double)q1);
    }
    const size_t need = cvx_prep_stats_workspace_bytes(n), xbytes = (size_t)n * 4;
    const Span ins[1] = {{x, xbytes}}, outs[3] = {{params, 16}, {moments3, 24}, {workspace, need}};
    const Overlaps ov = find_overlaps(outs, ins);
    CVX_REQUIRE(ov.out < 0, "cvx_prep_stats_f32: an output overlaps x");
    CVX_REQUIRE(ov.a < 0, "cvx_prep_stats_f32: outputs overlap each other");
    if (!workspace || workspace_bytes < need)
        return fail(CVX_ERR_WORKSPACE, "cvx_prep_stats_f32: workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, need);
    const size_t nspans = (size_t)cdiv64(n, PR_SPAN);
    const unsigned nblocks = (unsigned)cdiv64((int64_t)nspans, PR_G);
    Carver cv(workspace);
    const PrepWs w = prep_layout(cv, nspans);
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(workspace, 0, w.zeroed_bytes, s) != hipSuccess) return check_last("cvx_prep_stats_f32 (clear)");
    const int nq = n_quantiles;
    hipLaunchKernelGGL(k_prep_pass<1>, dim3(nblocks), dim3(PR_THREADS), 0, s, x, (size_t)n, flags, clamp_lo, clamp_hi, nq, w.st, w.psum, w.pcnt, w.h1, nspans);
    hipLaunchKernelGGL(k_prep_finish<1>, dim3(1), dim3(PR_THREADS), 0, s, w.psum, w.pcnt, nspans, n, flags, nq, rk, w.st, w.h1, params, moments3);
    int st = check_last("cvx_prep_stats_f32 (pass 1)");
    if (st != CVX_OK) return st;
    hipLaunchKernelGGL(k_prep_pass<2>, dim3(nblocks), dim3(PR_THREADS), 0, s, x, (size_t)n, flags, clamp_lo, clamp_hi, nq, w.st, w.pss, w.pcnt, w.h2, nspans);
    hipLaunchKernelGGL(k_prep_finish<2>, dim3(1), dim3(PR_THREADS), 0, s, w.pss, w.pcnt, nspans, n, flags, nq, rk, w.st, w.h2, params, moments3);
    st = check_last("cvx_prep_stats_f32 (pass 2)");
    if (st != CVX_OK || !nq) return st;
    hipLaunchKernelGGL(k_prep_pass<3>, dim3(nblocks), dim3(PR_THREADS), 0, s, x, (size_t)n, flags, clamp_lo, clamp_hi, nq, w.st, w.pss, w.pcnt, w.h3, nspans);
    hipLaunchKernelGGL(k_prep_finish<3>, dim3(1), dim3(PR_THREADS), 0, s, w.pss, w.pcnt, nspans, n, flags, nq, rk, w.st, w.h3, params, moments3);
    return check_last("cvx_prep_stats_f32 (pass 3)");
}

extern "C" int cvx_prep_normalise_f32(const float* x, long long n, const float* params, const float* params_host, int mode, float* out,
                                      void* stream) {
    CVX_REQUIRE(x && out, "cvx_prep_normalise_f32: null pointer (x or out)");
    CVX_REQUIRE((params != nullptr) != (params_host != nullptr), "cvx_prep_normalise_f32: exactly one of params (device) and params_host");
    CVX_REQUIRE(n >= 1 && n <= (long long)INT_MAX, "cvx_prep_normalise_f32: bad extent (n = %lld, 1 .. 2^31 - 1)", n);
    CVX_REQUIRE(mode == 0 || mode == 1, "cvx_prep_normalise_f32: mode %d (0 clamp + normalise, 1 positive voxels only)", mode);
    const size_t bytes = (size_t)n * 4;
    CVX_REQUIRE(out == x || !ranges_overlap(out, bytes, x, bytes), "cvx_prep_normalise_f32: out overlaps x without being x");
    CVX_REQUIRE(!overlap_any(params, 16, out, bytes), "cvx_prep_normalise_f32: params overlaps out");
    NormParams hp = {0.0f, 1.0f, 0.0f, 0.0f};
    if (params_host) hp = NormParams{params_host[0], params_host[1], params_host[2], params_host[3]};
    const bool vec = (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    const size_t threads = vec ? (size_t)n / 4 + (size_t)n % 4 : (size_t)n;
    const dim3 grid((unsigned)cdiv64((int64_t)threads, 256));
    hipStream_t s = as_stream(stream);
    if (mode == 0) {
        if (vec) hipLaunchKernelGGL((k_prep_normalise<0, true>), grid, dim3(256), 0, s, x, (size_t)n, params, hp, out);
        else hipLaunchKernelGGL((k_prep_normalise<0, false>), grid, dim3(256), 0, s, x, (size_t)n, params, hp, out);
    } else {
        if (vec) hipLaunchKernelGGL((k_prep_normalise<1, true>), grid, dim3(256), 0, s, x, (size_t)n, params, hp, out);
        else hipLaunchKernelGGL((k_prep_normalise<1, false>), grid, dim3(256), 0, s, x, (size_t)n, params, hp, out);
    }
    return check_last("cvx_prep_normalise_f32");
}

extern "C" size_t cvx_prep_nonzero_mask_workspace_bytes(int H, int W, int D) {
    const size_t V = voxels(H, W, D);
    if (!V) {
        fail(CVX_ERR_INVALID_ARG, "cvx_prep_nonzero_mask_workspace_bytes: bad extent or more than 2^31 - 1 voxels (%dx%dx%d)", H, W, D);
        return 0;
    }
    Carver m;
    mask_layout(m, V);
    return ws_query(m);
}

static void launch_box(unsigned char* mask, const unsigned char* reached, int H, int W, int D, int* box6, long long* count, hipStream_t s) {
    const size_t V = (size_t)H * W * D;
    const dim3 grid((unsigned)cdiv64((int64_t)V, 256 * MB_PER));
    hipLaunchKernelGGL(k_box_init, dim3(1), dim3(64), 0, s, box6, count);
    if (reached) hipLaunchKernelGGL(k_mask_final<true>, grid, dim3(256), 0, s, mask, reached, H, W, D, box6, reinterpret_cast<unsigned long long*>(count));
    else hipLaunchKernelGGL(k_mask_final<false>, grid, dim3(256), 0, s, mask, reached, H, W, D, box6, reinterpret_cast<unsigned long long*>(count));
}

extern "C" int cvx_prep_nonzero_mask_u8(const float* data, int C, int H, int W, int D, int ndim, unsigned char* mask_out, int* box6,
                                        long long* count, int* rounds_host, void* workspace, size_t workspace_bytes, void* stream) {
    CVX_REQUIRE(data && mask_out && box6, "cvx_prep_nonzero_mask_u8: null pointer (data, mask_out or box6)");
    CVX_REQUIRE(C >= 1, "cvx_prep_nonzero_mask_u8: C = %d channels", C);
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_prep_nonzero_mask_u8: bad extent (%dx%dx%d)", H, W, D);
    const size_t V = voxels(H, W, D);
    CVX_REQUIRE(V, "cvx_prep_nonzero_mask_u8: more than 2^31 - 1 voxels (%dx%dx%d)", H, W, D);
    CVX_REQUIRE((uint64_t)V * (uint64_t)C < ((uint64_t)1 << 40), "cvx_prep_nonzero_mask_u8: %d channels of %dx%dx%d are 2^40 elements or more", C, H, W, D);
    CVX_REQUIRE(ndim == 3 || (ndim == 2 && H == 1), "cvx_prep_nonzero_mask_u8: ndim %d (3, or 2 with H = 1)", ndim);
    const size_t need = cvx_prep_nonzero_mask_workspace_bytes(H, W, D), dbytes = (size_t)C * V * 4;
    const Span ins[1] = {{data, dbytes}}, outs[4] = {{mask_out, V}, {box6, 24}, {count, 8}, {workspace, need}};
    const Overlaps ov = find_overlaps(outs, ins);
    CVX_REQUIRE(ov.out < 0, "cvx_prep_nonzero_mask_u8: an output overlaps data");
    CVX_REQUIRE(ov.a < 0, "cvx_prep_nonzero_mask_u8: outputs overlap each other");
    if (!workspace || workspace_bytes < need)
        return fail(CVX_ERR_WORKSPACE, "cvx_prep_nonzero_mask_u8: workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, need);
    Carver cv(workspace);
    const MaskWs w = mask_layout(cv, V);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_mask_init, dim3((unsigned)cdiv64((int64_t)V, 256)), dim3(256), 0, s, data, C, H, W, D, ndim, mask_out, w.reached);
    int st = check_last("cvx_prep_nonzero_mask_u8 (init)");
    if (st != CVX_OK) return st;
    // lines along H: W D of them, a voxel every W D; along W: H D, every D, line l starts at (l / D) W D + l % D; along D: H W, contiguous
    const size_t WD = (size_t)W * D;
    const struct { int len; size_t step, nlines, inner, outer; } axis[3] = {{H, WD, WD, WD, 0}, {W, (size_t)D, (size_t)H * D, (size_t)D, WD},
                                                                            {D, 1, (size_t)H * W, 1, (size_t)D}};
    // rows in 8- or 4-byte words where D and both arrays' addresses allow, else byte by byte
    const uintptr_t row_align = (uintptr_t)mask_out | (uintptr_t)w.reached | (uintptr_t)D;
    const int row_bytes = row_align % 8 == 0 ? 8 : (row_align % 4 == 0 ? 4 : 1);
    const long long cap = (long long)V + 1;          // `reached` grows by at least one voxel in every round but the last
    long long round = 0;
    for (;;) {
        if (++round > cap) return fail(CVX_ERR_LAUNCH, "cvx_prep_nonzero_mask_u8: the sweeps did not settle in %lld rounds", cap);
        if (hipMemsetAsync(w.changed, 0, sizeof(unsigned), s) != hipSuccess) return check_last("cvx_prep_nonzero_mask_u8 (flag)");
        for (int a = (ndim == 2 ? 1 : 0); a < 3; ++a) {
            const dim3 grid((unsigned)cdiv64((int64_t)axis[a].nlines, 128));
            if (a == 2 && row_bytes == 8)
                hipLaunchKernelGGL(k_mask_sweep_row<unsigned long long>, grid, dim3(128), 0, s, mask_out, w.reached, D, axis[a].nlines, w.changed);
            else if (a == 2 && row_bytes == 4)
                hipLaunchKernelGGL(k_mask_sweep_row<unsigned>, grid, dim3(128), 0, s, mask_out, w.reached, D, axis[a].nlines, w.changed);
            else
                hipLaunchKernelGGL(k_mask_sweep, grid, dim3(128), 0, s, mask_out, w.reached, axis[a].len, axis[a].step, axis[a].nlines, axis[a].inner,
                                   axis[a].outer, w.changed);
        }
        st = check_last("cvx_prep_nonzero_mask_u8 (sweep)");
        if (st != CVX_OK) return st;
        unsigned changed = 0;
        if (hipMemcpyAsync(&changed, w.changed, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return check_last("cvx_prep_nonzero_mask_u8 (flag read)");
        if (!changed) break;
    }
    if (rounds_host) *rounds_host = (int)(round > INT_MAX ? INT_MAX : round);
    launch_box(mask_out, w.reached, H, W, D, box6, count, s);
    return check_last("cvx_prep_nonzero_mask_u8 (box)");
}

extern "C" int cvx_prep_mask_bbox_i32(const unsigned char* mask, int H, int W, int D, int* box6, long long* count, void* stream) {
    CVX_REQUIRE(mask && box6, "cvx_prep_mask_bbox_i32: null pointer (mask or box6)");
    CVX_REQUIRE(H > 0 && W > 0 && D > 0, "cvx_prep_mask_bbox_i32: bad extent (%dx%dx%d)", H, W, D);
    const size_t V = voxels(H, W, D);
    CVX_REQUIRE(V, "cvx_prep_mask_bbox_i32: more than 2^31 - 1 voxels (%dx%dx%d)", H, W, D);
    CVX_REQUIRE(!overlap_any(box6, 24, mask, V) && !overlap_any(count, 8, mask, V) && !overlap_any(box6, 24, count, 8),
                "cvx_prep_mask_bbox_i32: an output overlaps the mask or the other output");
    launch_box(const_cast<unsigned char*>(mask), nullptr, H, W, D, box6, count, as_stream(stream));
    return check_last("cvx_prep_mask_bbox_i32");
}
