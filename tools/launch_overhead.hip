// Fixed cost of a kernel boundary on one stream (gfx950): back-to-back dependent launches of small kernels, and of an issue-bound
// writer whose output leaves as plain or as write-through stores (profiles/wt_boundary_probe.txt).
//   hipcc --offload-arch=gfx950 -O3 tools/launch_overhead.hip -o tools/launch_overhead.bin
#include <hip/hip_runtime.h>
#include <stdio.h>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
__global__ void k_empty() {}
__global__ void k_write(float4* p, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = make_float4(1.f, 2.f, 3.f, (float)i);
}
__global__ void k_copy(const float4* a, float4* b, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { float4 v = a[i]; v.x += 1.f; b[i] = v; }
}
__global__ void k_read(const float4* a, float4* b, int n) {       // reads, (practically) never writes
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { float4 v = a[i]; if (v.x == 123456.f) b[i] = v; }
}
// ---- what a boundary costs behind an ISSUE-BOUND writer, with plain and with write-through stores ------------------------------------
// The writer runs a dependent chain of `chain` FMAs before each 16 bytes it stores (grid-stride over n quads), so its body is arithmetic and its
// stores trickle out; FORM 0 = plain 16-byte stores, 1 = write-through (aux 16 = sc1) 16-byte buffer stores, 2 / 3 = the same as four 4-byte
// stores per lane to four planes (adjacent lanes write adjacent dwords, as a one-value-per-lane epilogue does).  span (may be null): per workgroup
// {start, end} in 100 MHz ticks; latest end - earliest start = the body without the launch and without whatever the kernel's end does to the L2s.
template <int FORM>
__global__ void k_ibw(float* out, int n, int chain, float seed, unsigned long long* span) {
    if (span && threadIdx.x == 0) span[2 * blockIdx.x] = wall_clock64();
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(out, 0, n * 16, 0x00020000);
    float x = seed + (float)threadIdx.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        for (int k = 0; k < chain; ++k) x = __builtin_fmaf(x, 0.99999f, 0.5f);
        if (FORM == 0) reinterpret_cast<float4*>(out)[i] = make_float4(x, x + 1.f, x + 2.f, x + 3.f);
        else if (FORM == 1) { typedef unsigned u4 __attribute__((ext_vector_type(4))); __builtin_amdgcn_raw_buffer_store_b128(u4{__float_as_uint(x), __float_as_uint(x + 1.f), __float_as_uint(x + 2.f), __float_as_uint(x + 3.f)}, r, i * 16, 0, 16); }
        else
            for (int j = 0; j < 4; ++j) {
                if (FORM == 2) out[(size_t)j * n + i] = x + (float)j;
                else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x + (float)j), r, i * 4, j * n * 4, 16);
            }
    }
    if (span && threadIdx.x == 0) span[2 * blockIdx.x + 1] = wall_clock64();
}
__global__ void k_ibr(const float4* a, float4* b, int n, unsigned long long* span) {       // reads all n quads, (practically) never writes
    if (span && threadIdx.x == 0) span[2 * blockIdx.x] = wall_clock64();
    float s = 0.f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { const float4 v = a[i]; s += v.x + v.w; }
    if (s == 123456.f) b[threadIdx.x] = make_float4(s, s, s, s);
    if (span && threadIdx.x == 0) span[2 * blockIdx.x + 1] = wall_clock64();
}
template <typename F> static float timeit(F f, int reps) {
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (int i = 0; i < 20; ++i) f(i);
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < reps; ++i) f(i);
    (void)hipEventRecord(e1, 0); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    return ms / reps * 1e3f;
}
int main() {
    const int reps = 2000;
    float4 *a, *b, *c, *fa, *fb;
    CK(hipMalloc(&a, 64 << 20)); CK(hipMalloc(&b, 64 << 20)); CK(hipMalloc(&c, 64 << 20));
    CK(hipExtMallocWithFlags((void**)&fa, 64 << 20, hipDeviceMallocFinegrained)); CK(hipExtMallocWithFlags((void**)&fb, 64 << 20, hipDeviceMallocFinegrained));
    CK(hipMemset(a, 0, 64 << 20)); CK(hipMemset(b, 0, 64 << 20)); CK(hipMemset(c, 0, 64 << 20)); CK(hipMemset(fa, 0, 64 << 20)); CK(hipMemset(fb, 0, 64 << 20));
    for (int grid : {64, 504, 3360})
        printf("empty  grid %5d x 512                         : %6.2f us / launch\n", grid, timeit([&](int) { hipLaunchKernelGGL(k_empty, dim3(grid), dim3(512), 0, 0); }, reps));
    for (int kb : {64, 1024, 10240}) {
        const int n = kb * 1024 / 16;
        const int grid = n / 256 < 504 ? (n / 256 > 0 ? n / 256 : 1) : 504;
        printf("--- %d KB, grid %d x 256 / 512\n", kb, grid);
        printf("write (same buffer)                             : %6.2f\n", timeit([&](int) { hipLaunchKernelGGL(k_write, dim3(grid), dim3(256), 0, 0, a, n); }, reps));
        printf("read never-written buffer                       : %6.2f\n", timeit([&](int) { hipLaunchKernelGGL(k_read, dim3(grid), dim3(256), 0, 0, c, b, n); }, reps));
        printf("copy c -> a (source never rewritten)            : %6.2f\n", timeit([&](int) { hipLaunchKernelGGL(k_copy, dim3(grid), dim3(256), 0, 0, c, a, n); }, reps));
        printf("copy ping-pong a <-> b (read after write)       : %6.2f\n", timeit([&](int i) { if (i & 1) hipLaunchKernelGGL(k_copy, dim3(grid), dim3(256), 0, 0, b, a, n); else hipLaunchKernelGGL(k_copy, dim3(grid), dim3(256), 0, 0, a, b, n); }, reps));
        printf("copy ping-pong, fine-grained allocations        : %6.2f\n", timeit([&](int i) { if (i & 1) hipLaunchKernelGGL(k_copy, dim3(grid), dim3(256), 0, 0, fb, fa, n); else hipLaunchKernelGGL(k_copy, dim3(grid), dim3(256), 0, 0, fa, fb, n); }, reps));
        printf("write a ; read a (alternating)                  : %6.2f (per pair of launches)\n", 2 * timeit([&](int i) { if (i & 1) hipLaunchKernelGGL(k_read, dim3(grid), dim3(256), 0, 0, a, b, n); else hipLaunchKernelGGL(k_write, dim3(grid), dim3(256), 0, 0, a, n); }, reps));
    }
    // issue-bound writer -> reader: period of a pair of launches and the bodies' own durations, plain against write-through
    constexpr int kMaxGrid = 3360;
    unsigned long long* span;
    static unsigned long long got[2 * kMaxGrid];
    CK(hipMalloc(&span, sizeof(got)));
    auto body_us = [&](int grid, auto launch) {            // mean body duration of 20 single launches
        double sum = 0;
        for (int i = 0; i < 20; ++i) {
            launch(span);
            (void)hipDeviceSynchronize();
            (void)hipMemcpy(got, span, sizeof(got[0]) * 2 * grid, hipMemcpyDeviceToHost);
            unsigned long long t0 = ~0ull, t1 = 0;
            for (int b = 0; b < grid; ++b) { t0 = got[2 * b] < t0 ? got[2 * b] : t0; t1 = got[2 * b + 1] > t1 ? got[2 * b + 1] : t1; }
            sum += (double)(t1 - t0) * 0.01;
        }
        return (float)(sum / 20);
    };
    auto writer = [&](int form, int grid, int block, float* out, int n, int chain, unsigned long long* sp) {
        if (form == 0) hipLaunchKernelGGL(k_ibw<0>, dim3(grid), dim3(block), 0, 0, out, n, chain, 1.f, sp);
        else if (form == 1) hipLaunchKernelGGL(k_ibw<1>, dim3(grid), dim3(block), 0, 0, out, n, chain, 1.f, sp);
        else if (form == 2) hipLaunchKernelGGL(k_ibw<2>, dim3(grid), dim3(block), 0, 0, out, n, chain, 1.f, sp);
        else hipLaunchKernelGGL(k_ibw<3>, dim3(grid), dim3(block), 0, 0, out, n, chain, 1.f, sp);
    };
    static const char* const form_name[4] = {"plain 16 B        ", "write-through 16 B", "plain 4 x 4 B     ", "write-through 4x4B"};
    for (int mb : {10, 31})
        for (int cfg = 0; cfg < 2; ++cfg) {
            const int grid = cfg ? 3360 : 252, block = cfg ? 256 : 1024, n = mb * 1024 * 1024 / 16;
            // chain length for a ~15 us body: two points of the (linear) duration of the plain writer
            const float d1 = body_us(grid, [&](unsigned long long* sp) { writer(0, grid, block, (float*)a, n, 64, sp); });
            const float d2 = body_us(grid, [&](unsigned long long* sp) { writer(0, grid, block, (float*)a, n, 576, sp); });
            int chain = d2 > d1 ? (int)(64.f + (15.f - d1) * 512.f / (d2 - d1)) : 64;
            chain = chain < 8 ? 8 : chain > 100000 ? 100000 : chain;
            printf("--- issue-bound writer, %d MB, grid %d x %d, %d dependent FMAs per 16 bytes (bodies: %.1f us at 64, %.1f us at 576)\n", mb, grid, block, chain, d1, d2);
            const float rd = body_us(grid, [&](unsigned long long* sp) { hipLaunchKernelGGL(k_ibr, dim3(grid), dim3(block), 0, 0, c, b, n, sp); });
            for (int form = 0; form < 4; ++form) {
                const float wd = body_us(grid, [&](unsigned long long* sp) { writer(form, grid, block, (float*)a, n, chain, sp); });
                const float rda = body_us(grid, [&](unsigned long long* sp) { writer(form, grid, block, (float*)a, n, chain, nullptr); hipLaunchKernelGGL(k_ibr, dim3(grid), dim3(block), 0, 0, a, b, n, sp); });
                const float ww = timeit([&](int) { writer(form, grid, block, (float*)a, n, chain, nullptr); }, reps);
                const float pair = 2 * timeit([&](int i) { if (i & 1) hipLaunchKernelGGL(k_ibr, dim3(grid), dim3(block), 0, 0, a, b, n, (unsigned long long*)nullptr); else writer(form, grid, block, (float*)a, n, chain, nullptr); }, reps);
                printf("%s : writer body %6.2f us, reader body %6.2f us (%.2f on a never-written buffer), writer ; writer period %6.2f us, writer ; reader period %6.2f us per pair, pair minus bodies %6.2f us\n",
                       form_name[form], wd, rda, rd, ww, pair, pair - wd - rda);
            }
        }
    return 0;
}
