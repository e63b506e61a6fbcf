// tests/cpp/test_map_evidence_rule.cpp -- the rule of a voxel map's visibility evidence (icet_amd/csrc/icet_map_evidence.h, the text the kernels compile) as a
// stand-alone host program, for tests/test_map_evidence_host.py.  Built with g++ -ffp-contract=off.  Every float travels as the hexadecimal of its bits.
//   rows FILE      line 1: min_range image_log2 (decimal) n; then n lines of 3 row words.  Prints per line: part pixel word (zeros where the row takes no part).
//   cells FILE     line 1: cell min_range max_range margin image_log2 n; then n lines of 16 pose words, 3 centroid words and a near word.
//                  Prints per line: pose_ok part pixel class (0 none, 1 miss, 2 agree, 3 occluded).
//   near FILE      line 1: image_log2 window; then W^2 words.  Prints the W^2 words of the near image.
//   decide FILE    lines: miss agree min_miss agree_factor (decimal).  Prints the decision.
//   params FILE    lines: min_range max_range margin image_log2 window min_miss agree_factor flags (the last five decimal).  Prints params_ok.
//   interval FILE  lines: cell max_range prune (decimal) and 16 pose words.  Prints lo hi of the run of x cells.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../icet_amd/csrc/icet_map_evidence.h"

namespace erule = icet_map_evidence_rule;
namespace qrule = icet_map_query_rule;

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static bool read_words(FILE* f, float* v, int n) {
    for (int j = 0; j < n; j++) { uint32_t w; if (fscanf(f, "%" SCNx32, &w) != 1) return false; v[j] = from_bits(w); }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: test_map_evidence_rule rows|cells|near|decide|params|interval FILE\n"); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    int rc = 0;
    if (!strcmp(argv[1], "rows")) {
        uint32_t mnb; int32_t log2; long n;
        if (fscanf(f, "%" SCNx32 " %" SCNd32 " %ld", &mnb, &log2, &n) != 3) { fclose(f); return 3; }
        const erule::Consts k = erule::make_consts(0.1f, from_bits(mnb), 1.f, 0.f, log2, 0, 0, 0);
        for (long i = 0; i < n; i++) {
            float p[3];
            if (!read_words(f, p, 3)) { rc = 3; break; }
            int32_t pix = 0; uint32_t word = 0;
            const bool part = erule::row_pixel(k, p[0], p[1], p[2], pix, word);
            printf("%d %d %08x\n", part ? 1 : 0, part ? pix : 0, part ? word : 0u);
        }
    } else if (!strcmp(argv[1], "cells")) {
        uint32_t cb, mnb, mxb, mgb; int32_t log2; long n;
        if (fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNd32 " %ld", &cb, &mnb, &mxb, &mgb, &log2, &n) != 6) { fclose(f); return 3; }
        const erule::Consts k = erule::make_consts(from_bits(cb), from_bits(mnb), from_bits(mxb), from_bits(mgb), log2, 0, 0, 0);
        for (long i = 0; i < n; i++) {
            float T[16], m[3]; uint32_t near;
            if (!read_words(f, T, 16) || !read_words(f, m, 3) || fscanf(f, "%" SCNx32, &near) != 1) { rc = 3; break; }
            const bool ok = qrule::pose_ok(T);
            int32_t pix = 0; double d2 = 0.0;
            const bool part = ok && erule::cell_pixel(k, T, m[0], m[1], m[2], pix, d2);
            printf("%d %d %d %d\n", ok ? 1 : 0, part ? 1 : 0, part ? pix : 0, part ? erule::cell_class(k, d2, near) : 0);
        }
    } else if (!strcmp(argv[1], "near")) {
        int32_t log2, window;
        if (fscanf(f, "%" SCNd32 " %" SCNd32, &log2, &window) != 2 || log2 < 0 || log2 > 10) { fclose(f); return 3; }
        const erule::Consts k = erule::make_consts(0.1f, 0.f, 1.f, 0.f, log2, window, 0, 0);
        std::vector<uint32_t> img((size_t)k.width * k.width);
        for (uint32_t& w : img) if (fscanf(f, "%" SCNx32, &w) != 1) { fclose(f); return 3; }
        for (int32_t v = 0; v < k.width; v++)
            for (int32_t u = 0; u < k.width; u++) printf("%08x\n", erule::near_word(k, img.data(), u, v));
    } else if (!strcmp(argv[1], "decide")) {
        int32_t miss, agree, mm, af;
        while (fscanf(f, "%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32, &miss, &agree, &mm, &af) == 4) {
            const erule::Consts k = erule::make_consts(0.1f, 0.f, 1.f, 0.f, 4, 0, mm, af);
            printf("%d\n", erule::transient(k, miss, agree) ? 1 : 0);
        }
    } else if (!strcmp(argv[1], "params")) {
        uint32_t a, b, c; int32_t v[5];
        while (fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32, &a, &b, &c, &v[0], &v[1], &v[2], &v[3], &v[4]) == 8)
            printf("%d\n", erule::params_ok(from_bits(a), from_bits(b), from_bits(c), v[0], v[1], v[2], v[3], v[4]) ? 1 : 0);
    } else if (!strcmp(argv[1], "interval")) {
        uint32_t cb, mxb; int prune;
        while (fscanf(f, "%" SCNx32 " %" SCNx32 " %d", &cb, &mxb, &prune) == 3) {
            float T[16];
            if (!read_words(f, T, 16)) { rc = 3; break; }
            const erule::Consts k = erule::make_consts(from_bits(cb), 0.f, from_bits(mxb), 0.f, 4, 0, 0, 0);
            int32_t lo, hi;
            erule::x_interval(k, T, prune != 0, lo, hi);
            printf("%d %d\n", lo, hi);
        }
    } else {
        rc = 2;
    }
    fclose(f);
    return rc;
}
