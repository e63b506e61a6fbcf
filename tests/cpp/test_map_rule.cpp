// tests/cpp/test_map_rule.cpp -- the voxel map's rule (icet_amd/csrc/icet_map.h, the text the kernels compile) as a stand-alone host program, for
// tests/test_map_host.py.  Built with g++ -ffp-contract=off.  Every float travels as the hexadecimal of its bits.
//   rows FILE      line 1: cell min_range max_range n; then n lines of 16 pose words and 3 row words.  Prints per row: class key q_x q_y q_z.
//   centroid FILE  lines: cell c sum n (c, sum, n decimal).  Prints the bits of the centroid coordinate.
//   params FILE    lines: cell min_range max_range table_log2 flags (the last two decimal).  Prints params_ok.
//   sign FILE      lines: sign (decimal).  Prints sign_ok.
//   scan FILE      lines: n ld has_ptr (decimal).  Prints dev_scan_ok of the descriptor (icet_staging.h: the check every add runs per scan).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "../../icet_amd/csrc/icet_map.h"
#include "../../icet_amd/csrc/icet_staging.h"

namespace rule = icet_map_rule;

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: test_map_rule rows|centroid|params|sign|scan FILE\n"); return 2; }
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
            if (cls != rule::kRowKept) { pt.key = 0; pt.q[0] = pt.q[1] = pt.q[2] = 0; }
            printf("%d %" PRIu64 " %u %u %u\n", cls, pt.key, pt.q[0], pt.q[1], pt.q[2]);
        }
    } else if (!strcmp(argv[1], "centroid")) {
        uint32_t cb; int32_t c; uint64_t sum; int64_t n;
        while (fscanf(f, "%" SCNx32 " %" SCNd32 " %" SCNu64 " %" SCNd64, &cb, &c, &sum, &n) == 4) {
            const rule::Consts k = rule::make_consts(from_bits(cb), 0.f, 0.f);
            printf("%08x\n", to_bits(rule::centroid(k, c, sum, n)));
        }
    } else if (!strcmp(argv[1], "params")) {
        uint32_t cb, mnb, mxb; int32_t l2, fl;
        while (fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNd32 " %" SCNd32, &cb, &mnb, &mxb, &l2, &fl) == 5)
            printf("%d\n", rule::params_ok(from_bits(cb), from_bits(mnb), from_bits(mxb), l2, fl) ? 1 : 0);
    } else if (!strcmp(argv[1], "sign")) {
        int32_t s;
        while (fscanf(f, "%" SCNd32, &s) == 1) printf("%d\n", rule::sign_ok(s) ? 1 : 0);
    } else if (!strcmp(argv[1], "scan")) {
        static float row[3];
        int64_t n, ld; int has;
        while (fscanf(f, "%" SCNd64 " %" SCNd64 " %d", &n, &ld, &has) == 3) {
            icet_dev_scan d; d.ptr = has ? row : nullptr; d.n = n; d.ld = ld;
            printf("%d\n", icet::dev_scan_ok(d) ? 1 : 0);
        }
    } else {
        rc = 2;
    }
    fclose(f);
    return rc;
}
