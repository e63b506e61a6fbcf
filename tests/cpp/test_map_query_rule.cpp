// tests/cpp/test_map_query_rule.cpp -- the rule of a voxel map's query (icet_amd/csrc/icet_map_query.h, the text the kernels compile) as a stand-alone host
// program, for tests/test_map_query_host.py.  Built with g++ -ffp-contract=off.  Every float travels as the hexadecimal of its bits.
//   cells FILE     line 1: cell min_range max_range min_points flags n; then n lines of 16 pose words, 3 centroid words and a count (decimal).
//                  Prints per line: pose_ok kept row_x row_y row_z (the row's bits; zeros where the cell is not kept).
//   interval FILE  lines: cell max_range prune (decimal) and 16 pose words.  Prints lo hi of the run of x cells.
//   params FILE    lines: min_range max_range flags r0 r1 r2 r3 (the last five decimal).  Prints params_ok.
//   submap FILE    lines: has_xyz ld cap_rows (decimal).  Prints submap_ok.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "../../icet_amd/csrc/icet_map_query.h"

namespace qrule = icet_map_query_rule;

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static bool read_words(FILE* f, float* v, int n) {
    for (int j = 0; j < n; j++) { uint32_t w; if (fscanf(f, "%" SCNx32, &w) != 1) return false; v[j] = from_bits(w); }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: test_map_query_rule cells|interval|params|submap FILE\n"); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    int rc = 0;
    if (!strcmp(argv[1], "cells")) {
        uint32_t cb, mnb, mxb; int32_t minp, flags; long n;
        if (fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNd32 " %" SCNd32 " %ld", &cb, &mnb, &mxb, &minp, &flags, &n) != 6) { fclose(f); return 3; }
        const qrule::Consts k = qrule::make_consts(from_bits(cb), from_bits(mnb), from_bits(mxb), minp, flags);
        for (long i = 0; i < n; i++) {
            float T[16], m[3]; long long cnt;
            if (!read_words(f, T, 16) || !read_words(f, m, 3) || fscanf(f, "%lld", &cnt) != 1) { rc = 3; break; }
            const bool ok = qrule::pose_ok(T);
            double d[3] = {0, 0, 0};
            const bool kept = ok && qrule::keep(k, T, m[0], m[1], m[2], cnt, d);
            uint32_t r[3] = {0, 0, 0};
            for (int a = 0; a < 3 && kept; a++) r[a] = to_bits(k.world ? m[a] : qrule::row(T, d, a));
            printf("%d %d %08x %08x %08x\n", ok ? 1 : 0, kept ? 1 : 0, r[0], r[1], r[2]);
        }
    } else if (!strcmp(argv[1], "interval")) {
        uint32_t cb, mxb; int prune;
        while (fscanf(f, "%" SCNx32 " %" SCNx32 " %d", &cb, &mxb, &prune) == 3) {
            float T[16];
            if (!read_words(f, T, 16)) { rc = 3; break; }
            const qrule::Consts k = qrule::make_consts(from_bits(cb), 0.f, from_bits(mxb), 1, 0);
            int32_t lo, hi;
            qrule::x_interval(k, T, prune != 0, lo, hi);
            printf("%d %d\n", lo, hi);
        }
    } else if (!strcmp(argv[1], "params")) {
        uint32_t mnb, mxb; int32_t fl, r[4];
        while (fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32, &mnb, &mxb, &fl, &r[0], &r[1], &r[2], &r[3]) == 7)
            printf("%d\n", qrule::params_ok(from_bits(mnb), from_bits(mxb), fl, r) ? 1 : 0);
    } else if (!strcmp(argv[1], "submap")) {
        static float row[3];
        int has; int64_t ld, cap;
        while (fscanf(f, "%d %" SCNd64 " %" SCNd64, &has, &ld, &cap) == 3) printf("%d\n", qrule::submap_ok(has ? row : nullptr, ld, cap) ? 1 : 0);
    } else {
        rc = 2;
    }
    fclose(f);
    return rc;
}
