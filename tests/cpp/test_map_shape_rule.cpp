// tests/cpp/test_map_shape_rule.cpp -- the voxel map's shape rule (icet_amd/csrc/icet_map_shape.h, the text the kernels compile) as a stand-alone host program,
// for tests/test_map_shape_host.py.  Built with g++ -ffp-contract=off.  Every float travels as the hexadecimal of its bits, every double as 16 hex digits.
//   rows FILE    line 1: cell min_range max_range n; then n lines of 16 pose words and 3 row words.  Prints per row: class h_x h_y h_z and the nine increments
//                (all zero for a row that is not kept).
//   cov FILE     lines: cell n w_0 .. w_8 (n and the words decimal, the words as uint64).  Prints the six float32 cov values, then the six doubles of C.
//   eigen FILE   lines: the six doubles of C.  Prints evals[3] and normal[3] as float32 bits.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "../../icet_amd/csrc/icet_map_shape.h"

namespace rule = icet_map_rule;
namespace srule = icet_map_shape_rule;

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static double from_bits64(uint64_t b) { double f; memcpy(&f, &b, 8); return f; }
static uint64_t to_bits64(double f) { uint64_t b; memcpy(&b, &f, 8); return b; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: test_map_shape_rule rows|cov|eigen FILE\n"); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    int rc = 0;
    if (!strcmp(argv[1], "rows")) {
        uint32_t cb, mnb, mxb; long n;
        if (fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %ld", &cb, &mnb, &mxb, &n) != 4) { fclose(f); return 3; }
        const rule::Consts k = rule::make_consts(from_bits(cb), from_bits(mnb), from_bits(mxb));
        for (long i = 0; i < n && !rc; i++) {
            float T[16], p[3];
            for (int j = 0; j < 19; j++) {
                uint32_t w;
                if (fscanf(f, "%" SCNx32, &w) != 1) { rc = 3; break; }
                if (j < 16) T[j] = from_bits(w); else p[j - 16] = from_bits(w);
            }
            if (rc) break;
            rule::Point pt; pt.key = 0; pt.q[0] = pt.q[1] = pt.q[2] = 0;
            const int cls = rule::classify(k, T, p[0], p[1], p[2], pt);
            uint32_t S[3] = {0, 0, 0}, M[6] = {0, 0, 0, 0, 0, 0};
            if (cls == rule::kRowKept) srule::row_moments(pt.q, S, M);
            printf("%d %u %u %u", cls, S[0], S[1], S[2]);
            for (int a = 0; a < 3; a++) printf(" %u", S[a]);
            for (int j = 0; j < 6; j++) printf(" %u", M[j]);
            printf("\n");
        }
    } else if (!strcmp(argv[1], "cov")) {
        uint32_t cb; int64_t n; uint64_t w[srule::kWords];
        while (fscanf(f, "%" SCNx32 " %" SCNd64, &cb, &n) == 2) {
            for (int j = 0; j < srule::kWords; j++) if (fscanf(f, "%" SCNu64, &w[j]) != 1) { rc = 3; break; }
            if (rc) break;
            double C[6];
            srule::cov(srule::make_consts(from_bits(cb)), n, w, C);
            for (int j = 0; j < 6; j++) printf("%08x ", to_bits((float)C[j]));
            for (int j = 0; j < 6; j++) printf("%016" PRIx64 "%s", to_bits64(C[j]), j == 5 ? "\n" : " ");
        }
    } else if (!strcmp(argv[1], "eigen")) {
        uint64_t b[6];
        while (fscanf(f, "%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &b[0], &b[1], &b[2], &b[3], &b[4], &b[5]) == 6) {
            double C[6]; float ev[3], nm[3];
            for (int j = 0; j < 6; j++) C[j] = from_bits64(b[j]);
            srule::eigen(C, ev, nm);
            printf("%08x %08x %08x %08x %08x %08x\n", to_bits(ev[0]), to_bits(ev[1]), to_bits(ev[2]), to_bits(nm[0]), to_bits(nm[1]), to_bits(nm[2]));
        }
    } else {
        rc = 2;
    }
    fclose(f);
    return rc;
}
