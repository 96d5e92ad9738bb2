// softstats_host.cpp -- the arithmetic of csrc/softstats.hip (convexadam_amd/csrc/softstats_core.h) run on the host over raw arrays: the same
// text the kernels compile, under the host compiler's sanitizers (tests/test_softstats_reference.py builds it with -O1 -ffp-contract=off
// -fsanitize=address,undefined and compares it with tests/softstats_restatement.py bit for bit).
//
//   softstats_host stats h w d hw half has_field coupling beta ssd.bin [field.bin] out.bin
//       ssd.bin    the volume [K][V], K = (2 hw + 1)^3, V = h w d: float (half = 0) or float16 (1) elements
//       field.bin  (has_field = 1) [3][V] floats
//       coupling, beta   decimal text of float32 values
//       out.bin    out [12][V] float | the number of non-finite columns, int64
//   softstats_host expf n in.bin out.bin
//       in.bin     n floats in -104 .. 0;  out.bin  soft_expf of each
// Exit status 0, or 2 with a message for a bad command line or a short file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "softstats_core.h"

static bool read_all(const char* path, void* p, size_t bytes) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(p, 1, bytes, f);
    const bool at_end = fgetc(f) == EOF;
    fclose(f);
    return got == bytes && at_end;
}

static int write_file(const char* path, const void* a, size_t abytes, const void* b, size_t bbytes) {
    FILE* f = fopen(path, "wb");
    if (!f) return fprintf(stderr, "softstats_host: cannot write %s\n", path), 2;
    const bool ok = fwrite(a, 1, abytes, f) == abytes && (!bbytes || fwrite(b, 1, bbytes, f) == bbytes);
    return fclose(f) == 0 && ok ? 0 : 2;
}

template <typename T>
static int run_stats(size_t V, int hw, float coupling, float beta, const char* ssd_path, const char* field_path, const char* out_path) {
    const int n = 2 * hw + 1;
    const size_t K = (size_t)n * n * n;
    std::vector<T> ssd(K * V);
    if (!read_all(ssd_path, ssd.data(), K * V * sizeof(T))) return fprintf(stderr, "softstats_host: %s does not hold %zu elements\n", ssd_path, K * V), 2;
    std::vector<float> u(field_path ? 3 * V : 0);
    if (field_path && !read_all(field_path, u.data(), 3 * V * 4)) return fprintf(stderr, "softstats_host: %s does not hold %zu floats\n", field_path, 3 * V), 2;
    std::vector<float> out(cvx::SOFT_CHANNELS * V);
    int64_t bad = 0;
    for (size_t x = 0; x < V; ++x) {
        cvx::SoftColumn<T> col;
        col.ssd = ssd.data() + x;
        col.V = V;
        col.hw = hw;
        col.has_field = field_path != nullptr;
        col.coupling = coupling;
        col.u0 = field_path ? u[x] : 0.0f;
        col.u1 = field_path ? u[V + x] : 0.0f;
        col.u2 = field_path ? u[2 * V + x] : 0.0f;
        float o[cvx::SOFT_CHANNELS];
        bad += cvx::soft_column(col, beta, o);
        for (int i = 0; i < cvx::SOFT_CHANNELS; ++i) out[i * V + x] = o[i];
    }
    return write_file(out_path, out.data(), out.size() * 4, &bad, 8);
}

static int run_expf(size_t n, const char* in, const char* out) {
    std::vector<float> a(n), b(n);
    if (!read_all(in, a.data(), n * 4)) return fprintf(stderr, "softstats_host: %s does not hold %zu floats\n", in, n), 2;
    for (size_t i = 0; i < n; ++i) {
        if (!(a[i] >= -104.0f && a[i] <= 0.0f)) return fprintf(stderr, "softstats_host: argument %zu outside -104 .. 0\n", i), 2;
        b[i] = cvx::soft_expf(a[i]);
    }
    return write_file(out, b.data(), n * 4, nullptr, 0);
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "expf")) {
        const long n = atol(argv[2]);
        if (n < 1 || n > (1L << 26)) return fprintf(stderr, "softstats_host: n outside 1 .. 2^26\n"), 2;
        return run_expf((size_t)n, argv[3], argv[4]);
    }
    const bool stats = argc >= 12 && !strcmp(argv[1], "stats") && argc == 12 + (atoi(argv[7]) != 0);
    if (!stats) {
        fprintf(stderr, "usage: softstats_host stats h w d hw half has_field coupling beta ssd.bin [field.bin] out.bin\n"
                        "       softstats_host expf n in.bin out.bin\n");
        return 2;
    }
    const int h = atoi(argv[2]), w = atoi(argv[3]), d = atoi(argv[4]), hw = atoi(argv[5]);
    const bool half = atoi(argv[6]) != 0, has_field = atoi(argv[7]) != 0;
    const float coupling = (float)strtod(argv[8], nullptr), beta = (float)strtod(argv[9], nullptr);
    if (h < 1 || w < 1 || d < 1 || hw < 0 || hw > 15 || (double)h * w * d * (2 * hw + 1) * (2 * hw + 1) * (2 * hw + 1) > 1e8)
        return fprintf(stderr, "softstats_host: bad extent\n"), 2;
    if (!(beta > 0.0f) || !(coupling >= 0.0f)) return fprintf(stderr, "softstats_host: bad beta or coupling\n"), 2;
    const size_t V = (size_t)h * w * d;
    const char* field = has_field ? argv[11] : nullptr;
    const char* out = argv[has_field ? 12 : 11];
    return half ? run_stats<cvx::soft_half>(V, hw, coupling, beta, argv[10], field, out) : run_stats<float>(V, hw, coupling, beta, argv[10], field, out);
}
