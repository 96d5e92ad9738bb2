// tps.hip -- thin-plate-spline densification of a field known at sparse points (l2r_2021_convexAdam_task1_docker.py:198-262,365-387).
//
// Four pieces, each a replacement for one eager step of the reference:
//   fit     TPS.fit (task1:200-222): assemble the (n+4) x (n+4) saddle-point system  [K P; P^T 0] theta = [f; 0]  with
//           K = U(d(c_i, c_j)) + lambda I, P = [1 | c], and solve it by LU with partial pivoting (what torch.solve / linalg.solve do).
//           The right-hand sides ride along as extra columns of the matrix (A | v), so the trailing updates of the factorisation apply
//           L^-1 P to them and only the back substitution with U is left at the end.  Blocked right-looking scheme, panel width NB = 32:
//             k_lu_panel       one 1024-thread workgroup factors the N x 32 panel column by column (pivot search, row swap inside
//                              the panel, scaling, rank-1 update of the rest of the panel);
//             k_lu_swap_trsm   one thread per column right of the panel: applies the panel's 32 row swaps in order and solves
//                              U12 = L11^-1 A12 (L11 unit lower, staged in LDS);
//             k_lu_gemm        trailing update A22 -= L21 U12 as a 64 x 64-tiled fp32 VALU GEMM (K = 32, both operands through LDS);
//             k_lu_backsub     one workgroup: 64-row blocks from the bottom, the diagonal block solved by one wave from LDS, the rows
//                              above updated by the whole workgroup.
//           Columns left of a panel are never swapped: L is used only by its own panel's trailing update (the right-hand sides are
//           transformed on the way), so the row permutation of L never matters.  A zero or non-finite pivot sets `info` (1-based
//           column); every later kernel of the solve checks it and returns, so nothing downstream computes on it and theta is not
//           written.  Coincident centres with lambda = 0 are caught exactly by the assembly (see k_tps_assemble).  The host reads
//           `info` back (the fit synchronises its stream) and returns CVX_ERR_INVALID_ARG "singular system".
//   eval    TPS.z (task1:233-239): out = a0 + a1 x + a2 y + a3 z + sum_j w_j U(r_j) for m points against n centres.  Centres and
//           weights are staged through LDS in chunks of 256 (every lane reads the same centre: LDS broadcasts); two points per lane.
//   dense   the same evaluation on the F.affine_grid(eye, (1,1,s0,s1,s2), align_corners=True) lattice (thin_plate_dense, task1:247),
//           the points generated in the kernel: x = linspace(-1,1,s2)[i2], y = ..s1[i1], z = ..s0[i0] (float32 torch.linspace; an axis
//           of size 1 gives 0 as ATen's linspace_from_neg_one does); output channel-major [nrhs][s0][s1][s2].
//   resize  F.interpolate(..., mode='trilinear', align_corners=True) (task1:260): ATen's CPU coefficients for that mode
//           (scale = (in-1)/(out-1) rounded to float, src = scale * o) with the interpolation chain of k_resize (pool.hip).
//
// How r is formed.  The reference forms d(a, b) = sqrt(max(|a|^2 + |b|^2 - 2 a.b, 0)) and U = r^2 log(r + 1e-6) from that r.  Here
// r^2 is the sum of the squared DIRECT coordinate differences (no cancellation: the expanded form loses all relative accuracy of r^2
// when two points are close, and gives a non-zero r on the diagonal), r = sqrtf(r^2), and U = r^2 * logf(r + 1e-6f) with the r^2
// that was summed, not the square of the rounded root.  This is closer to the float64 restatement the tests grade against than the
// reference's own float32 arithmetic.  logf / sqrtf are the accurate library functions (the build has no fast-math).
#include "cvx_common.h"

namespace cvx {

constexpr int TPS_NB = 32;            // panel width of the LU
constexpr int TPS_MAX_N = 16384;      // centres (the matrix is (n+4) x (n+4+nrhs) floats: 1.1 GB at the limit)
constexpr int TPS_MAX_RHS = 4;

static inline int tps_lda(int n, int nrhs) { return (int)align_up((size_t)(n + 4 + nrhs), 64); }

__device__ __forceinline__ float tps_u(float r2) {
    const float r = sqrtf(r2);
    return r2 * logf(r + 1e-6f);
}

// torch.linspace(-1, 1, S)[i] in float32 (cvx_affine_base_host's formula, api.hip); S == 1 -> 0 (ATen linspace_from_neg_one)
__device__ __forceinline__ float tps_lin(int i, int S) {
    if (S <= 1) return 0.0f;
    const float step = 2.0f / (float)(S - 1);
    return (i < S / 2) ? __builtin_fmaf(step, (float)i, -1.0f) : __builtin_fmaf(-step, (float)(S - 1 - i), 1.0f);
}

// ---- system assembly: A = [K P v; P^T 0 0], N = n + 4 rows, N + nrhs columns, row-major with leading dimension lda -----------------
// Two coincident centres with lambda = 0 make two rows of K (and of A) equal: the system is exactly singular.  Elimination would turn
// the second row into rounding residue (the panel, triangular solve and GEMM round in different orders), not into an exact zero pivot,
// so the assembly detects the case itself and sets info = -(first such row + 1) before the factorisation starts.
__global__ __launch_bounds__(256) void k_tps_assemble(const float* __restrict__ c, const float* __restrict__ f, int n, int nrhs, float lambd,
                                                      float* __restrict__ A, int lda, int* __restrict__ info) {
    const int N = n + 4, ncol = N + nrhs;
    const int row = (int)blockIdx.y, col = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (col >= ncol) return;
    float v = 0.0f;
    if (row < n) {
        if (col < n) {
            const float dx = c[3 * row] - c[3 * col], dy = c[3 * row + 1] - c[3 * col + 1], dz = c[3 * row + 2] - c[3 * col + 2];
            const float r2 = dx * dx + dy * dy + dz * dz;
            v = tps_u(r2);
            if (row == col) v = v + lambd;
            else if (r2 == 0.0f && lambd == 0.0f && row < col) atomicCAS(info, 0, -(row + 1));
        } else if (col < N) {
            v = col == n ? 1.0f : c[3 * row + (col - n - 1)];
        } else {
            v = f[(size_t)row * nrhs + (col - N)];
        }
    } else if (col < n) {
        v = row == n ? 1.0f : c[3 * col + (row - n - 1)];
    }
    A[(size_t)row * lda + col] = v;
}

// ---- panel factorisation: columns k0 .. k0+nb-1, rows k0 .. N-1, one workgroup of 1024 threads --------------------------------------
__global__ __launch_bounds__(1024) void k_lu_panel(float* __restrict__ A, int lda, int N, int k0, int nb, int* __restrict__ piv,
                                                   int* __restrict__ info) {
    if (*info != 0) return;
    __shared__ float s_val[16];
    __shared__ int s_idx[16];
    __shared__ float prow[TPS_NB];
    __shared__ int s_p, s_bad;
    const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int j = k0; j < k0 + nb; ++j) {
        // pivot search: largest |a| (NaN counts as infinite so that it is found and refused), first index on ties (isamax)
        float best = -1.0f;
        int bi = N;
        for (int r = j + tid; r < N; r += 1024) {
            float a = fabsf(A[(size_t)r * lda + j]);
            if (a != a) a = INFINITY;
            if (a > best) { best = a; bi = r; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) { s_val[wid] = best; s_idx[wid] = bi; }
        __syncthreads();
        if (tid == 0) {
            float b = s_val[0];
            int p = s_idx[0];
            for (int w = 1; w < 16; ++w)
                if (s_val[w] > b || (s_val[w] == b && s_idx[w] < p)) { b = s_val[w]; p = s_idx[w]; }
            const float pv = (p < N) ? A[(size_t)p * lda + j] : 0.0f;
            const bool bad = p >= N || !(pv != 0.0f) || !isfinite(pv);
            s_bad = bad ? 1 : 0;
            s_p = p;
            if (bad) *info = j + 1;
            else piv[j] = p;
        }
        __syncthreads();
        if (s_bad) return;                                   // uniform: every thread read the same flag after the barrier
        const int p = s_p;
        if (tid < nb) {
            const int c = k0 + tid;
            const float a = A[(size_t)j * lda + c];
            float b = a;
            if (p != j) {
                b = A[(size_t)p * lda + c];
                A[(size_t)j * lda + c] = b;
                A[(size_t)p * lda + c] = a;
            }
            prow[tid] = b;
        }
        __syncthreads();
        const float pv = prow[j - k0];
        const int cend = k0 + nb;
        for (int r = j + 1 + tid; r < N; r += 1024) {
            float* Ar = A + (size_t)r * lda;
            const float l = Ar[j] / pv;
            Ar[j] = l;
            for (int c = j + 1; c < cend; ++c) Ar[c] = __builtin_fmaf(-l, prow[c - k0], Ar[c]);
        }
        __syncthreads();
    }
}

// ---- row swaps of the panel + U12 = L11^-1 A12, one thread per column c in [k0+nb, ncol) -------------------------------------------
__global__ __launch_bounds__(256) void k_lu_swap_trsm(float* __restrict__ A, int lda, int ncol, int k0, int nb, const int* __restrict__ piv,
                                                      const int* __restrict__ info) {
    if (*info != 0) return;
    __shared__ float L[TPS_NB][TPS_NB + 1];
    __shared__ int sp[TPS_NB];
    const int tid = (int)threadIdx.x;
    for (int idx = tid; idx < nb * nb; idx += 256) L[idx / nb][idx % nb] = A[(size_t)(k0 + idx / nb) * lda + k0 + idx % nb];
    if (tid < nb) sp[tid] = piv[k0 + tid];
    __syncthreads();
    const int c = k0 + nb + (int)(blockIdx.x * blockDim.x) + tid;
    if (c >= ncol) return;
    for (int i = 0; i < nb; ++i) {
        const int p = sp[i];
        if (p != k0 + i) {
            const float a = A[(size_t)(k0 + i) * lda + c];
            A[(size_t)(k0 + i) * lda + c] = A[(size_t)p * lda + c];
            A[(size_t)p * lda + c] = a;
        }
    }
    float x[TPS_NB];
#pragma unroll
    for (int i = 0; i < TPS_NB; ++i) x[i] = i < nb ? A[(size_t)(k0 + i) * lda + c] : 0.0f;
#pragma unroll
    for (int i = 1; i < TPS_NB; ++i)
#pragma unroll
        for (int t = 0; t < i; ++t)
            if (i < nb) x[i] = __builtin_fmaf(-L[i][t], x[t], x[i]);
#pragma unroll
    for (int i = 0; i < TPS_NB; ++i)
        if (i < nb) A[(size_t)(k0 + i) * lda + c] = x[i];
}

// ---- trailing update A[r0:N, c0:ncol] -= L21 U12, r0 = c0 = k0 + 32; 64 x 64 tile per workgroup, 4 x 4 outputs per thread -----------
__global__ __launch_bounds__(256) void k_lu_gemm(float* __restrict__ A, int lda, int N, int ncol, int k0, const int* __restrict__ info) {
    if (*info != 0) return;
    __shared__ float As[TPS_NB][64 + 4];                     // As[k][m] = L21[m][k]
    __shared__ float Bs[TPS_NB][64 + 4];                     // Bs[k][n] = U12[k][n]
    const int r0 = k0 + TPS_NB, tm = r0 + (int)blockIdx.y * 64, tn = r0 + (int)blockIdx.x * 64;
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int idx = tid + 256 * e;
        const int m = idx >> 5, k = idx & 31;
        const int row = tm + m;
        As[k][m] = row < N ? A[(size_t)row * lda + k0 + k] : 0.0f;
        const int kk = idx >> 6, nn = idx & 63;
        const int col = tn + nn;
        Bs[kk][nn] = col < ncol ? A[(size_t)(k0 + kk) * lda + col] : 0.0f;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    float acc[4][4] = {};
#pragma unroll 8
    for (int k = 0; k < TPS_NB; ++k) {
        float a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { a[i] = As[k][ty + 16 * i]; b[i] = Bs[k][tx + 16 * i]; }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][q] = __builtin_fmaf(a[i], b[q], acc[i][q]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = tm + ty + 16 * i;
        if (row >= N) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = tn + tx + 16 * q;
            if (col < ncol) A[(size_t)row * lda + col] -= acc[i][q];
        }
    }
}

// ---- back substitution U x = y (y = columns N .. N+nrhs-1 of A, overwritten), one workgroup of 1024 threads -----------------------
__global__ __launch_bounds__(1024) void k_lu_backsub(float* __restrict__ A, int lda, int N, int nrhs, float* __restrict__ theta,
                                                     const int* __restrict__ info) {
    if (*info != 0) return;
    __shared__ float Dg[64][65];
    __shared__ float xs[64][TPS_MAX_RHS];
    const int tid = (int)threadIdx.x;
    for (int i1 = N; i1 > 0; i1 -= 64) {
        const int i0 = i1 > 64 ? i1 - 64 : 0, bs = i1 - i0;
        for (int idx = tid; idx < bs * bs; idx += 1024) Dg[idx / bs][idx % bs] = A[(size_t)(i0 + idx / bs) * lda + i0 + idx % bs];
        if (tid < bs * nrhs) xs[tid / nrhs][tid % nrhs] = A[(size_t)(i0 + tid / nrhs) * lda + N + tid % nrhs];
        __syncthreads();
        if (tid < 64) {                                      // wave 0 solves the diagonal block
            const int lane = tid;
            float y[TPS_MAX_RHS];
#pragma unroll
            for (int k = 0; k < TPS_MAX_RHS; ++k) y[k] = (lane < bs && k < nrhs) ? xs[lane][k] : 0.0f;
            for (int i = bs - 1; i >= 0; --i) {
                const float d = Dg[i][i];
                const float u = lane < i ? Dg[lane][i] : 0.0f;
#pragma unroll
                for (int k = 0; k < TPS_MAX_RHS; ++k) {
                    const float xi = __shfl(y[k], i) / d;
                    if (lane == i) y[k] = xi;
                    else if (lane < i) y[k] = __builtin_fmaf(-u, xi, y[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < TPS_MAX_RHS; ++k)
                if (lane < bs && k < nrhs) xs[lane][k] = y[k];
        }
        __syncthreads();
        if (tid < bs * nrhs) theta[(size_t)(i0 + tid / nrhs) * nrhs + tid % nrhs] = xs[tid / nrhs][tid % nrhs];
        for (int r = tid; r < i0; r += 1024) {
            const float* Ar = A + (size_t)r * lda + i0;
            float s[TPS_MAX_RHS];
#pragma unroll
            for (int k = 0; k < TPS_MAX_RHS; ++k) s[k] = k < nrhs ? A[(size_t)r * lda + N + k] : 0.0f;
            for (int t = 0; t < bs; ++t) {
                const float u = Ar[t];
#pragma unroll
                for (int k = 0; k < TPS_MAX_RHS; ++k) s[k] = __builtin_fmaf(-u, xs[t][k], s[k]);
            }
#pragma unroll
            for (int k = 0; k < TPS_MAX_RHS; ++k)
                if (k < nrhs) A[(size_t)r * lda + N + k] = s[k];
        }
        __syncthreads();
    }
}

// ---- evaluation: out[i * sp + k * sk] = a0 + a1 x + a2 y + a3 z + sum_j w_jk U(|p_i - c_j|) -----------------------------------------
// pts != nullptr: points [m][3]; pts == nullptr: the affine_grid lattice s0 x s1 x s2 (m = s0 s1 s2, s2 fastest)
constexpr int TPS_PPL = 2;            // points per lane
template <int NR>
__global__ __launch_bounds__(256) void k_tps_eval(const float* __restrict__ pts, int64_t m, int s0, int s1, int s2, const float* __restrict__ c,
                                                  const float* __restrict__ theta, int n, float* __restrict__ out, int64_t sp, int64_t sk) {
    __shared__ float sc[3][256];
    __shared__ float sw[NR][256];
    const int tid = (int)threadIdx.x;
    float px[TPS_PPL], py[TPS_PPL], pz[TPS_PPL], acc[TPS_PPL][NR];
    int64_t idx[TPS_PPL];
#pragma unroll
    for (int p = 0; p < TPS_PPL; ++p) {
        const int64_t i = ((int64_t)blockIdx.x * TPS_PPL + p) * 256 + tid;
        idx[p] = i;
        px[p] = py[p] = pz[p] = 0.0f;
        if (i < m) {
            if (pts) {
                px[p] = pts[3 * i]; py[p] = pts[3 * i + 1]; pz[p] = pts[3 * i + 2];
            } else {
                const int i2 = (int)(i % s2);
                const int64_t t = i / s2;
                const int i1 = (int)(t % s1), i0 = (int)(t / s1);
                px[p] = tps_lin(i2, s2); py[p] = tps_lin(i1, s1); pz[p] = tps_lin(i0, s0);
            }
        }
#pragma unroll
        for (int k = 0; k < NR; ++k) acc[p][k] = 0.0f;
    }
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int cnt = n - j0 < 256 ? n - j0 : 256;
        __syncthreads();
        if (tid < cnt) {
            const int j = j0 + tid;
            sc[0][tid] = c[3 * j]; sc[1][tid] = c[3 * j + 1]; sc[2][tid] = c[3 * j + 2];
#pragma unroll
            for (int k = 0; k < NR; ++k) sw[k][tid] = theta[(size_t)j * NR + k];
        }
        __syncthreads();
        for (int jj = 0; jj < cnt; ++jj) {
            const float cx = sc[0][jj], cy = sc[1][jj], cz = sc[2][jj];
#pragma unroll
            for (int p = 0; p < TPS_PPL; ++p) {
                const float dx = px[p] - cx, dy = py[p] - cy, dz = pz[p] - cz;
                const float u = tps_u(dx * dx + dy * dy + dz * dz);
#pragma unroll
                for (int k = 0; k < NR; ++k) acc[p][k] = __builtin_fmaf(sw[k][jj], u, acc[p][k]);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < TPS_PPL; ++p) {
        if (idx[p] >= m) continue;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const float a0 = theta[(size_t)n * NR + k], a1 = theta[(size_t)(n + 1) * NR + k], a2 = theta[(size_t)(n + 2) * NR + k],
                        a3 = theta[(size_t)(n + 3) * NR + k];
            out[idx[p] * sp + k * sk] = a0 + a1 * px[p] + a2 * py[p] + a3 * pz[p] + acc[p][k];
        }
    }
}

static int launch_eval(const float* pts, int64_t m, int s0, int s1, int s2, const float* c, const float* theta, int n, int nrhs, float* out,
                       int64_t sp, int64_t sk, hipStream_t s) {
    const int64_t blocks = cdiv64(m, 256 * TPS_PPL);
    if (blocks > 0x7fffffffLL) return fail(CVX_ERR_UNSUPPORTED, "tps eval: %lld points exceed the grid limit", (long long)m);
    const dim3 g((unsigned)blocks), b(256);
    switch (nrhs) {
    case 1: hipLaunchKernelGGL(k_tps_eval<1>, g, b, 0, s, pts, m, s0, s1, s2, c, theta, n, out, sp, sk); break;
    case 2: hipLaunchKernelGGL(k_tps_eval<2>, g, b, 0, s, pts, m, s0, s1, s2, c, theta, n, out, sp, sk); break;
    case 3: hipLaunchKernelGGL(k_tps_eval<3>, g, b, 0, s, pts, m, s0, s1, s2, c, theta, n, out, sp, sk); break;
    default: hipLaunchKernelGGL(k_tps_eval<4>, g, b, 0, s, pts, m, s0, s1, s2, c, theta, n, out, sp, sk); break;
    }
    return check_last("tps_eval");
}

// ---- F.interpolate(x, size, mode='trilinear', align_corners=True), ATen CPU arithmetic -------------------------------------------------
//   scale = out > 1 ? float(in-1) / (out-1) : 0; src = scale * o; i0 = min(floor(src), in-1); l1 = clamp(src - i0, 0, 1); l0 = 1 - l1;
//   i1 = i0 + (i0 < in-1); per level (last dim first): r = fma(v0, l0, v1 * l1)   (the chain of k_resize, pool.hip)
__device__ __forceinline__ void lin_coef_ac(int o, int in, int out, int& i0, int& i1, float& l0, float& l1) {
    const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
    const float src = scale * (float)o;
    int a = (int)floorf(src);
    a = a > in - 1 ? in - 1 : a;
    float l = src - (float)a;
    l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
    i0 = a;
    i1 = a + ((a < in - 1) ? 1 : 0);
    l1 = l;
    l0 = 1.0f - l;
}
__global__ __launch_bounds__(256) void k_resize_ac(const float* __restrict__ in, int C, int h, int w, int d, float* __restrict__ out, int H,
                                                   int W, int D) {
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x), y = (int)blockIdx.y, z = (int)blockIdx.z;
    if (x >= D) return;
    int z0, z1, y0, y1, x0, x1;
    float lz0, lz1, ly0, ly1, lx0, lx1;
    lin_coef_ac(z, h, H, z0, z1, lz0, lz1);
    lin_coef_ac(y, w, W, y0, y1, ly0, ly1);
    lin_coef_ac(x, d, D, x0, x1, lx0, lx1);
    const size_t o00 = ((size_t)z0 * w + y0) * d, o01 = ((size_t)z0 * w + y1) * d, o10 = ((size_t)z1 * w + y0) * d,
                 o11 = ((size_t)z1 * w + y1) * d;
    const size_t cs = (size_t)h * w * d, n = (size_t)H * W * D, i = ((size_t)z * W + y) * D + x;
    for (int ch = 0; ch < C; ++ch) {
        const float* ic = in + (size_t)ch * cs;
        const float a0 = __builtin_fmaf(ic[o00 + x0], lx0, ic[o00 + x1] * lx1);
        const float a1 = __builtin_fmaf(ic[o01 + x0], lx0, ic[o01 + x1] * lx1);
        const float b0 = __builtin_fmaf(ic[o10 + x0], lx0, ic[o10 + x1] * lx1);
        const float b1 = __builtin_fmaf(ic[o11 + x0], lx0, ic[o11 + x1] * lx1);
        const float l0 = __builtin_fmaf(a0, ly0, a1 * ly1);
        const float l1 = __builtin_fmaf(b0, ly0, b1 * ly1);
        out[(size_t)ch * n + i] = __builtin_fmaf(l0, lz0, l1 * lz1);
    }
}

}  // namespace cvx

using namespace cvx;

// the augmented system [N][lda], its pivots, the status word
struct TpsWs { float* A; int *piv, *info; };
static TpsWs tps_layout(Carver& cv, int n, int nrhs) {
    const size_t N = (size_t)n + 4;
    TpsWs t;
    t.A = cv.take<float>(N * (size_t)tps_lda(n, nrhs));
    t.piv = cv.take<int>(N);
    t.info = cv.take<int>(1);
    return t;
}
extern "C" size_t cvx_tps_fit_workspace_bytes(int n, int nrhs) {
    if (n < 1 || n > TPS_MAX_N || nrhs < 1 || nrhs > TPS_MAX_RHS) return 0;
    Carver m; tps_layout(m, n, nrhs); return align_up(m.used, 256);    // (no slack: the status word rounded to its granule, as this query always was)
}

extern "C" int cvx_tps_fit_f32(const float* centres, const float* values, int n, int nrhs, float lambd, float* theta, void* workspace,
                               size_t workspace_bytes, void* stream) {
    CVX_REQUIRE(centres && values && theta && workspace, "cvx_tps_fit_f32: null pointer");
    CVX_REQUIRE(n >= 1 && n <= TPS_MAX_N, "cvx_tps_fit_f32: n = %d outside 1..%d", n, TPS_MAX_N);
    CVX_REQUIRE(nrhs >= 1 && nrhs <= TPS_MAX_RHS, "cvx_tps_fit_f32: nrhs = %d outside 1..%d", nrhs, TPS_MAX_RHS);
    CVX_REQUIRE(lambd - lambd == 0.0f, "cvx_tps_fit_f32: lambda is not finite");
    const size_t need = cvx_tps_fit_workspace_bytes(n, nrhs);
    if (workspace_bytes < need) return fail(CVX_ERR_WORKSPACE, "cvx_tps_fit_f32: workspace %zu < %zu bytes", workspace_bytes, need);
    const int N = n + 4, ncol = N + nrhs, lda = tps_lda(n, nrhs);
    Carver cv(workspace);
    const auto [A, piv, info] = tps_layout(cv, n, nrhs);
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(info, 0, sizeof(int), s) != hipSuccess) { (void)hipGetLastError(); return fail(CVX_ERR_LAUNCH, "cvx_tps_fit_f32: memset failed"); }
    hipLaunchKernelGGL(k_tps_assemble, dim3((unsigned)cdiv(ncol, 256), (unsigned)N), dim3(256), 0, s, centres, values, n, nrhs, lambd, A, lda, info);
    int rc = check_last("tps_assemble");
    if (rc != CVX_OK) return rc;
    for (int k0 = 0; k0 < N; k0 += TPS_NB) {
        const int nb = N - k0 < TPS_NB ? N - k0 : TPS_NB;
        hipLaunchKernelGGL(k_lu_panel, dim3(1), dim3(1024), 0, s, A, lda, N, k0, nb, piv, info);
        const int right = ncol - (k0 + nb);                  // >= nrhs > 0
        hipLaunchKernelGGL(k_lu_swap_trsm, dim3((unsigned)cdiv(right, 256)), dim3(256), 0, s, A, lda, ncol, k0, nb, piv, info);
        const int rows = N - (k0 + nb);
        if (rows > 0)                                        // only when nb == TPS_NB
            hipLaunchKernelGGL(k_lu_gemm, dim3((unsigned)cdiv(right, 64), (unsigned)cdiv(rows, 64)), dim3(256), 0, s, A, lda, N, ncol, k0, info);
        if ((rc = check_last("tps_lu")) != CVX_OK) return rc;
    }
    hipLaunchKernelGGL(k_lu_backsub, dim3(1), dim3(1024), 0, s, A, lda, N, nrhs, theta, info);
    if ((rc = check_last("tps_backsub")) != CVX_OK) return rc;
    int h_info = 0;
    if (hipMemcpyAsync(&h_info, info, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CVX_ERR_LAUNCH, "cvx_tps_fit_f32: reading the pivot status failed");
    }
    if (h_info < 0)
        return fail(CVX_ERR_INVALID_ARG, "cvx_tps_fit_f32: singular system (centre %d coincides with a later centre and lambda = 0); "
                    "theta not written", -h_info - 1);
    if (h_info > 0)
        return fail(CVX_ERR_INVALID_ARG, "cvx_tps_fit_f32: singular system (zero or non-finite pivot in column %d of %d; duplicate centres with "
                    "lambda = 0?); theta not written", h_info - 1, N);
    return CVX_OK;
}

extern "C" int cvx_tps_eval_f32(const float* points, int64_t m, const float* centres, const float* theta, int n, int nrhs, float* out,
                                void* stream) {
    CVX_REQUIRE(points && centres && theta && out, "cvx_tps_eval_f32: null pointer");
    CVX_REQUIRE(m >= 0, "cvx_tps_eval_f32: m = %lld < 0", (long long)m);
    CVX_REQUIRE(n >= 1, "cvx_tps_eval_f32: n = %d < 1", n);
    CVX_REQUIRE(nrhs >= 1 && nrhs <= TPS_MAX_RHS, "cvx_tps_eval_f32: nrhs = %d outside 1..%d", nrhs, TPS_MAX_RHS);
    if (m == 0) return CVX_OK;
    return launch_eval(points, m, 1, 1, 1, centres, theta, n, nrhs, out, nrhs, 1, as_stream(stream));
}

extern "C" int cvx_tps_dense_f32(int s0, int s1, int s2, const float* centres, const float* theta, int n, int nrhs, float* out, void* stream) {
    CVX_REQUIRE(centres && theta && out, "cvx_tps_dense_f32: null pointer");
    CVX_REQUIRE(s0 >= 1 && s1 >= 1 && s2 >= 1, "cvx_tps_dense_f32: bad lattice %d x %d x %d", s0, s1, s2);
    CVX_REQUIRE(n >= 1, "cvx_tps_dense_f32: n = %d < 1", n);
    CVX_REQUIRE(nrhs >= 1 && nrhs <= TPS_MAX_RHS, "cvx_tps_dense_f32: nrhs = %d outside 1..%d", nrhs, TPS_MAX_RHS);
    const int64_t m = (int64_t)s0 * s1 * s2;
    return launch_eval(nullptr, m, s0, s1, s2, centres, theta, n, nrhs, out, 1, m, as_stream(stream));
}

extern "C" int cvx_resize_trilinear_ac_f32(const float* in, int C, int h, int w, int d, float* out, int H, int W, int D, void* stream) {
    CVX_REQUIRE(in && out, "cvx_resize_trilinear_ac_f32: null pointer");
    CVX_REQUIRE(C > 0 && h > 0 && w > 0 && d > 0 && H > 0 && W > 0 && D > 0, "cvx_resize_trilinear_ac_f32: bad extent");
    if (H > 65535 || W > 65535) return fail(CVX_ERR_UNSUPPORTED, "cvx_resize_trilinear_ac_f32: output extent %dx%d exceeds the grid limits", H, W);
    const int bx = D > 128 ? 256 : (D > 64 ? 128 : 64);
    hipLaunchKernelGGL(k_resize_ac, dim3((unsigned)cdiv(D, bx), (unsigned)W, (unsigned)H), dim3(bx), 0, as_stream(stream), in, C, h, w, d, out, H, W, D);
    return check_last("resize_trilinear_ac");
}
