// affine_host.cpp -- the arithmetic of csrc/affine.hip (convexadam_amd/csrc/affine_core.h) run on the host over raw arrays: the same text the
// kernels compile, under the host compiler's sanitizers (tests/test_affine_reference.py builds it with -O1 -ffp-contract=off
// -fsanitize=address,undefined and compares the field with tests/affine_restatement.py bit for bit, the solve with numpy.linalg.solve).
//
//   affine_host field H W D f64 planar has_u theta.bin [u.bin] out.bin
//       theta.bin  12 floats (3 x 4)
//       u.bin      (has_u = 1) the field, float (f64 = 0) or double (1) elements, [H][W][D][3] (planar = 0) or [3][H][W][D] (1)
//       out.bin    out [H][W][D][3] double
//   affine_host solve nrhs aug.bin out.bin
//       aug.bin    [A | B]: 4 rows of 8 doubles
//       out.bin    X 4 x 4 doubles (columns >= nrhs zero; all zero unless the status is 0) | status int64
// Exit status 0, or 2 with a message for a bad command line or a short file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "affine_core.h"

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
    if (!f) return fprintf(stderr, "affine_host: cannot write %s\n", path), 2;
    const bool ok = fwrite(a, 1, abytes, f) == abytes && (!bbytes || fwrite(b, 1, bbytes, f) == bbytes);
    return fclose(f) == 0 && ok ? 0 : 2;
}

template <typename T>
static int run_field(int H, int W, int D, bool planar, const char* theta, const char* in, const char* out) {
    const size_t V = (size_t)H * W * D, cs = planar ? V : 1, vs = planar ? 1 : 3;
    float th[12];
    if (!read_all(theta, th, sizeof th)) return fprintf(stderr, "affine_host: %s does not hold 12 floats\n", theta), 2;
    std::vector<T> u(in ? 3 * V : 0);
    if (in && !read_all(in, u.data(), 3 * V * sizeof(T))) return fprintf(stderr, "affine_host: %s does not hold %zu elements\n", in, 3 * V), 2;
    std::vector<double> o(3 * V);
    for (int i0 = 0; i0 < H; ++i0)
        for (int i1 = 0; i1 < W; ++i1)
            for (int i2 = 0; i2 < D; ++i2) {
                double r[3];
                cvx::affine_field_voxel(th, in ? u.data() : (const T*)nullptr, cs, vs, H, W, D, i0, i1, i2, r);
                for (int c = 0; c < 3; ++c) o[3 * ((((size_t)i0 * W + i1) * D) + i2) + c] = r[c];
            }
    return write_file(out, o.data(), 3 * V * 8, nullptr, 0);
}

static int run_solve(int nrhs, const char* in, const char* out) {
    double aug[4][8], X[16];
    if (!read_all(in, aug, sizeof aug)) return fprintf(stderr, "affine_host: %s does not hold 32 doubles\n", in), 2;
    const int64_t status = cvx::affine_solve4(aug, nrhs);
    for (int r = 0; r < 4; ++r)
        for (int j = 0; j < 4; ++j) X[4 * r + j] = status == 0 && j < nrhs ? aug[r][4 + j] : 0.0;
    return write_file(out, X, sizeof X, &status, 8);
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "solve")) {
        const int nrhs = atoi(argv[2]);
        if (nrhs < 1 || nrhs > 4) return fprintf(stderr, "affine_host: nrhs outside 1 .. 4\n"), 2;
        return run_solve(nrhs, argv[3], argv[4]);
    }
    const bool field = argc >= 10 && !strcmp(argv[1], "field") && argc == 10 + (atoi(argv[7]) != 0);
    if (!field) {
        fprintf(stderr, "usage: affine_host field H W D f64 planar has_u theta.bin [u.bin] out.bin\n"
                        "       affine_host solve nrhs aug.bin out.bin\n");
        return 2;
    }
    const int H = atoi(argv[2]), W = atoi(argv[3]), D = atoi(argv[4]);
    const bool f64 = atoi(argv[5]) != 0, planar = atoi(argv[6]) != 0, has_u = atoi(argv[7]) != 0;
    if (H < 1 || W < 1 || D < 1 || (double)H * W * D > 1e8) return fprintf(stderr, "affine_host: bad extent\n"), 2;
    const char* in = has_u ? argv[9] : nullptr;
    const char* out = argv[has_u ? 10 : 9];
    return f64 ? run_field<double>(H, W, D, planar, argv[8], in, out) : run_field<float>(H, W, D, planar, argv[8], in, out);
}
