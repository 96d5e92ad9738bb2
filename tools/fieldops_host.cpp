// fieldops_host.cpp -- the per-voxel arithmetic of csrc/fieldops.hip (convexadam_amd/csrc/fieldops_core.h) run on the host, voxel by voxel,
// over raw arrays: the same text the kernels compile, under the host compiler's sanitizers (tests/test_fieldops_reference.py builds it with
// -O1 -ffp-contract=off -fsanitize=address,undefined and compares its output with tests/fieldops_restatement.py bit for bit).
//
//   fieldops_host invert  H W D f64 planar max_iters tol u.bin out.bin
//       u.bin    the field, float (f64 = 0) or double (1) elements, [H][W][D][3] (planar = 0) or [3][H][W][D] (1)
//       out.bin  v [H][W][D][3] double | residual [H][W][D] double | stats 3 x int64 | iters [H][W][D] uint8
//   fieldops_host compose H W D f64 planar a.bin b.bin out.bin
//       out.bin  out [H][W][D][3] double
// Exit status 0, or 2 with a message for a bad command line or a short file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fieldops_core.h"

static bool read_all(const char* path, void* p, size_t bytes) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(p, 1, bytes, f);
    const bool at_end = fgetc(f) == EOF;
    fclose(f);
    return got == bytes && at_end;
}

static bool write_all(FILE* f, const void* p, size_t bytes) { return fwrite(p, 1, bytes, f) == bytes; }

template <typename T>
static int run_invert(int H, int W, int D, bool planar, int max_iters, double tol, const char* in, const char* out) {
    const size_t V = (size_t)H * W * D, cs = planar ? V : 1, vs = planar ? 1 : 3;
    std::vector<T> u(3 * V);
    if (!read_all(in, u.data(), 3 * V * sizeof(T))) return fprintf(stderr, "fieldops_host: %s does not hold %zu elements\n", in, 3 * V), 2;
    std::vector<double> v(3 * V), res(V);
    std::vector<unsigned char> iters(V);
    int64_t stats[3] = {0, 0, 0};
    for (int i0 = 0; i0 < H; ++i0)
        for (int i1 = 0; i1 < W; ++i1)
            for (int i2 = 0; i2 < D; ++i2) {
                const size_t q = ((size_t)i0 * W + i1) * D + i2;
                double r, vv[3];
                int it;
                const int flag = cvx::field_invert_voxel(u.data(), cs, vs, H, W, D, i0, i1, i2, max_iters, tol, vv, r, it);
                for (int a = 0; a < 3; ++a) v[3 * q + a] = vv[a];
                res[q] = r;
                iters[q] = (unsigned char)it;
                stats[0] += flag == cvx::FIELD_NOT_CONVERGED;
                stats[1] += flag == cvx::FIELD_NON_FINITE;
                if (flag != cvx::FIELD_NON_FINITE) {
                    int64_t bits;
                    memcpy(&bits, &r, 8);
                    if (bits > stats[2]) stats[2] = bits;
                }
            }
    FILE* f = fopen(out, "wb");
    if (!f) return fprintf(stderr, "fieldops_host: cannot write %s\n", out), 2;
    const bool ok = write_all(f, v.data(), 3 * V * 8) && write_all(f, res.data(), V * 8) && write_all(f, stats, 24) && write_all(f, iters.data(), V);
    return fclose(f) == 0 && ok ? 0 : 2;
}

template <typename T>
static int run_compose(int H, int W, int D, bool planar, const char* ina, const char* inb, const char* out) {
    const size_t V = (size_t)H * W * D, cs = planar ? V : 1, vs = planar ? 1 : 3;
    std::vector<T> a(3 * V), b(3 * V);
    if (!read_all(ina, a.data(), 3 * V * sizeof(T)) || !read_all(inb, b.data(), 3 * V * sizeof(T)))
        return fprintf(stderr, "fieldops_host: an input does not hold %zu elements\n", 3 * V), 2;
    std::vector<double> o(3 * V);
    for (int i0 = 0; i0 < H; ++i0)
        for (int i1 = 0; i1 < W; ++i1)
            for (int i2 = 0; i2 < D; ++i2) {
                double r[3];
                cvx::field_compose_voxel(a.data(), cs, vs, b.data(), cs, vs, H, W, D, i0, i1, i2, r);
                for (int c = 0; c < 3; ++c) o[3 * ((((size_t)i0 * W + i1) * D) + i2) + c] = r[c];
            }
    FILE* f = fopen(out, "wb");
    if (!f) return fprintf(stderr, "fieldops_host: cannot write %s\n", out), 2;
    const bool ok = write_all(f, o.data(), 3 * V * 8);
    return fclose(f) == 0 && ok ? 0 : 2;
}

int main(int argc, char** argv) {
    const bool invert = argc == 11 && !strcmp(argv[1], "invert"), compose = argc == 10 && !strcmp(argv[1], "compose");
    if (!invert && !compose) {
        fprintf(stderr, "usage: fieldops_host invert H W D f64 planar max_iters tol u.bin out.bin\n"
                        "       fieldops_host compose H W D f64 planar a.bin b.bin out.bin\n");
        return 2;
    }
    const int H = atoi(argv[2]), W = atoi(argv[3]), D = atoi(argv[4]);
    const bool f64 = atoi(argv[5]) != 0, planar = atoi(argv[6]) != 0;
    if (H < 1 || W < 1 || D < 1 || (double)H * W * D > 1e8) return fprintf(stderr, "fieldops_host: bad extent\n"), 2;
    if (invert) {
        const int max_iters = atoi(argv[7]);
        const double tol = strtod(argv[8], nullptr);
        if (max_iters < 1 || max_iters > 1000 || !(tol >= 0.0 && tol <= DBL_MAX)) return fprintf(stderr, "fieldops_host: bad max_iters or tol\n"), 2;
        return f64 ? run_invert<double>(H, W, D, planar, max_iters, tol, argv[9], argv[10])
                   : run_invert<float>(H, W, D, planar, max_iters, tol, argv[9], argv[10]);
    }
    return f64 ? run_compose<double>(H, W, D, planar, argv[7], argv[8], argv[9]) : run_compose<float>(H, W, D, planar, argv[7], argv[8], argv[9]);
}
