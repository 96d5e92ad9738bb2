// simhist_host.cpp -- the arithmetic of csrc/simhist.hip (convexadam_amd/csrc/simhist_core.h) run on the host over raw arrays: the same text
// the kernels compile, under the host compiler's sanitizers (tests/test_simhist_reference.py builds it with -O1 -ffp-contract=off
// -fsanitize=address,undefined and compares it with tests/simhist_restatement.py bit for bit).
//
//   simhist_host H W D field cs vs has_mask drop given lo_a hi_a lo_b hi_b n ba_1 bb_1 .. ba_n bb_n fixed.bin moving.bin [field.bin] [mask.bin] out.bin
//       field      0 none, 1 float elements, 2 double elements; cs, vs its component and voxel stride in elements (ignored without a field)
//       given      1: the histograms use the range lo_a .. hi_b (decimal text of float32 values, inf and nan allowed); 0: the range found
//       n          number of (bins_a, bins_b) pairs that follow
//       fixed.bin, moving.bin   H W D floats;  field.bin  2 cs + (H W D - 1) vs + 1 elements;  mask.bin  H W D bytes
//       out.bin    range float[4] | range stats int64[5] | per pair: hist int64[ba][bb] | stats int64[5]
// Exit status 0, or 2 with a message for a bad command line or a short file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "simhist_core.h"

static bool read_all(const char* path, void* p, size_t bytes) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(p, 1, bytes, f);
    const bool at_end = fgetc(f) == EOF;
    fclose(f);
    return got == bytes && at_end;
}

static bool append(FILE* f, const void* p, size_t bytes) { return fwrite(p, 1, bytes, f) == bytes; }

struct Job {
    int H, W, D, field, has_mask, drop, given;
    size_t cs, vs;
    float range[4];
    std::vector<int> bins;
};

template <typename TU>
static int run(const Job& j, const std::vector<float>& fixed, const std::vector<float>& moving, const TU* u, const unsigned char* mask, const char* out_path) {
    float range[4];
    int64_t stats[cvx::SIM_STATS];
    cvx::sim_range_all(fixed.data(), moving.data(), u, j.cs, j.vs, mask, j.H, j.W, j.D, j.drop, range, stats);
    FILE* f = fopen(out_path, "wb");
    if (!f) return fprintf(stderr, "simhist_host: cannot write %s\n", out_path), 2;
    bool ok = append(f, range, sizeof range) && append(f, stats, sizeof stats);
    for (size_t k = 0; k + 1 < j.bins.size(); k += 2) {
        const int ba = j.bins[k], bb = j.bins[k + 1];
        std::vector<int64_t> hist((size_t)ba * bb);
        cvx::sim_hist_all(fixed.data(), moving.data(), u, j.cs, j.vs, mask, j.H, j.W, j.D, ba, bb, j.given ? j.range : range, j.drop, hist.data(), stats);
        ok = ok && append(f, hist.data(), hist.size() * 8) && append(f, stats, sizeof stats);
    }
    return fclose(f) == 0 && ok ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc < 16) {
        fprintf(stderr, "usage: simhist_host H W D field cs vs has_mask drop given lo_a hi_a lo_b hi_b n ba_1 bb_1 .. fixed.bin moving.bin [field.bin] [mask.bin] out.bin\n");
        return 2;
    }
    Job j;
    j.H = atoi(argv[1]), j.W = atoi(argv[2]), j.D = atoi(argv[3]), j.field = atoi(argv[4]);
    j.cs = (size_t)atoll(argv[5]), j.vs = (size_t)atoll(argv[6]);
    j.has_mask = atoi(argv[7]) != 0, j.drop = atoi(argv[8]) != 0, j.given = atoi(argv[9]) != 0;
    for (int i = 0; i < 4; ++i) j.range[i] = (float)strtod(argv[10 + i], nullptr);
    const int n = atoi(argv[14]);
    if (j.H < 1 || j.W < 1 || j.D < 1 || (double)j.H * j.W * j.D > 1e8 || j.field < 0 || j.field > 2 || n < 0 || n > 64)
        return fprintf(stderr, "simhist_host: bad extent, field kind or number of bin pairs\n"), 2;
    const int files = 15 + 2 * n;
    if (argc != files + 3 + (j.field != 0) + j.has_mask) return fprintf(stderr, "simhist_host: %d arguments do not match the command line's own counts\n", argc), 2;
    for (int i = 0; i < 2 * n; ++i) {
        const int b = atoi(argv[15 + i]);
        if (b < cvx::SIM_MIN_BINS || b > cvx::SIM_MAX_BINS) return fprintf(stderr, "simhist_host: bins outside 2 .. 256\n"), 2;
        j.bins.push_back(b);
    }
    const size_t V = (size_t)j.H * j.W * j.D;
    std::vector<float> fixed(V), moving(V);
    if (!read_all(argv[files], fixed.data(), V * 4) || !read_all(argv[files + 1], moving.data(), V * 4))
        return fprintf(stderr, "simhist_host: an image does not hold %zu floats\n", V), 2;
    int next = files + 2;
    std::vector<unsigned char> raw_field, mask;
    if (j.field) {
        if (j.cs < 1 || j.vs < 1 || j.cs > (1u << 30) || j.vs > (1u << 20)) return fprintf(stderr, "simhist_host: bad strides\n"), 2;
        const size_t elems = 2 * j.cs + (V - 1) * j.vs + 1;
        raw_field.resize(elems * (j.field == 2 ? 8 : 4));
        if (!read_all(argv[next++], raw_field.data(), raw_field.size())) return fprintf(stderr, "simhist_host: the field does not hold %zu elements\n", elems), 2;
    }
    if (j.has_mask) {
        mask.resize(V);
        if (!read_all(argv[next++], mask.data(), V)) return fprintf(stderr, "simhist_host: the mask does not hold %zu bytes\n", V), 2;
    }
    const unsigned char* m = j.has_mask ? mask.data() : nullptr;
    const char* out = argv[next];
    // (a vector's storage is aligned for any element type)
    if (j.field == 2) return run(j, fixed, moving, reinterpret_cast<const double*>(raw_field.data()), m, out);
    if (j.field == 1) return run(j, fixed, moving, reinterpret_cast<const float*>(raw_field.data()), m, out);
    return run(j, fixed, moving, static_cast<const float*>(nullptr), m, out);
}
