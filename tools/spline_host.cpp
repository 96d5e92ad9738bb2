// spline_host.cpp -- the arithmetic of csrc/spline.hip (convexadam_amd/csrc/spline_core.h) run on the host over raw arrays: the same text
// the kernels compile, under the host compiler's sanitizers (tests/test_spline_reference.py builds it with -O1 -ffp-contract=off
// -fsanitize=address,undefined and compares it with tests/spline_restatement.py bit for bit).
//
//   spline_host H W D kind n default src.bin coords.bin out.bin
//       kind        1 float samples, 2 double samples
//       n           number of points; coords.bin holds n x 3 doubles (axis 0, 1, 2), NaN and infinities allowed
//       default     what itk_cubic_f64 answers outside (decimal text)
//       out.bin     coefficients double[H W D] | map_cubic_f64 double[n] | itk_cubic_f64 double[n]
// Exit status 0, or 2 with a message for a bad command line or a short file.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "spline_core.h"

static bool read_all(const char* path, void* p, size_t bytes) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = bytes ? fread(p, 1, bytes, f) : 0;
    const bool at_end = fgetc(f) == EOF;
    fclose(f);
    return got == bytes && at_end;
}

int main(int argc, char** argv) {
    if (argc != 10) {
        fprintf(stderr, "usage: spline_host H W D kind n default src.bin coords.bin out.bin\n");
        return 2;
    }
    const int H = atoi(argv[1]), W = atoi(argv[2]), D = atoi(argv[3]), kind = atoi(argv[4]), n = atoi(argv[5]);
    const double dflt = strtod(argv[6], nullptr);
    if (H < 1 || W < 1 || D < 1 || (double)H * W * D > 1e8 || (kind != 1 && kind != 2) || n < 0 || n > (1 << 24))
        return fprintf(stderr, "spline_host: bad extent, sample kind or number of points\n"), 2;
    const size_t V = (size_t)H * W * D;
    std::vector<double> coef(V), coords((size_t)n * 3), out((size_t)n * 2);
    if (kind == 1) {
        std::vector<float> src(V);
        if (!read_all(argv[7], src.data(), V * 4)) return fprintf(stderr, "spline_host: the volume does not hold %zu floats\n", V), 2;
        cvx::spline_prefilter_all(src.data(), coef.data(), H, W, D);
    } else {
        std::vector<double> src(V);
        if (!read_all(argv[7], src.data(), V * 8)) return fprintf(stderr, "spline_host: the volume does not hold %zu doubles\n", V), 2;
        cvx::spline_prefilter_all(src.data(), coef.data(), H, W, D);
    }
    if (!read_all(argv[8], coords.data(), coords.size() * 8)) return fprintf(stderr, "spline_host: the points file does not hold %d x 3 doubles\n", n), 2;
    for (int p = 0; p < n; ++p) {
        const double cz = coords[3 * (size_t)p], cy = coords[3 * (size_t)p + 1], cx = coords[3 * (size_t)p + 2];
        out[p] = cvx::map_cubic_f64(coef.data(), H, W, D, cz, cy, cx);
        out[(size_t)n + p] = cvx::itk_cubic_f64(coef.data(), H, W, D, cz, cy, cx, dflt);
    }
    FILE* f = fopen(argv[9], "wb");
    if (!f) return fprintf(stderr, "spline_host: cannot write %s\n", argv[9]), 2;
    const bool ok = fwrite(coef.data(), 8, V, f) == V && fwrite(out.data(), 8, out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 2;
}
