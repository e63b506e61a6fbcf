// tests/cpp/test_deskew_rule.cpp -- the deskew rule (icet_amd/csrc/icet_deskew.h, the text the kernels compile) as a stand-alone host program, for
// tests/test_deskew_host.py.  Built with g++ -ffp-contract=off (and, for the sanitizer run, -fsanitize=address,undefined).  Every float and double travels as
// the hexadecimal of its bits.
//   rows FILE    line 1: mode period t0 inv_span s_ref xi[6] n (mode, period, n decimal); then n lines x y z time.  Prints per row: class out_x out_y out_z.
//   pose FILE    lines: xi[6] s.  Prints the 16 words of exp(s xi).
//   twist FILE   lines: T[16].  Prints the 6 words of log(T).
//   between FILE lines: T0[16] T1[16] (float32 words) scale.  Prints the 6 words of scale log(T0^-1 T1).
//   check FILE   lines: n ld ld_out mode period src_word dst_word (decimal; the two pointers as float offsets into one buffer, -1 = NULL).  Prints
//                shape_ok mode_ok overlap.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../icet_amd/csrc/icet_deskew.h"

namespace rule = icet_deskew_rule;

static float f32(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t bits32(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static double f64(uint64_t b) { double f; memcpy(&f, &b, 8); return f; }
static uint64_t bits64(double f) { uint64_t b; memcpy(&b, &f, 8); return b; }
static bool read64(FILE* f, double* v, int n) {
    for (int k = 0; k < n; k++) { uint64_t w; if (fscanf(f, "%" SCNx64, &w) != 1) return false; v[k] = f64(w); }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: test_deskew_rule rows|pose|twist|between|check FILE\n"); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    int rc = 0;
    if (!strcmp(argv[1], "rows")) {
        rule::Motion m; double par[9]; long n = 0;
        if (fscanf(f, "%" SCNd32 " %" SCNd32, &m.mode, &m.period) != 2 || !read64(f, par, 9) || fscanf(f, "%ld", &n) != 1 || n < 0) { fclose(f); return 3; }
        m.t0 = par[0]; m.inv_span = par[1]; m.s_ref = par[2];
        for (int a = 0; a < 6; a++) m.xi[a] = par[3 + a];
        std::vector<uint32_t> in(4 * (size_t)n);
        for (size_t k = 0; k < in.size(); k++) if (fscanf(f, "%" SCNx32, &in[k]) != 1) { fclose(f); return 3; }
        for (long i = 0; i < n; i++) {
            float o[3] = {0.f, 0.f, 0.f};
            const int cls = rule::deskew_row(m, (int32_t)i, f32(in[4 * i + 3]), f32(in[4 * i]), f32(in[4 * i + 1]), f32(in[4 * i + 2]), o);
            if (cls == rule::kRowMoved) printf("%d %08x %08x %08x\n", cls, bits32(o[0]), bits32(o[1]), bits32(o[2]));
            else printf("%d %08x %08x %08x\n", cls, in[4 * i], in[4 * i + 1], in[4 * i + 2]);      // (the caller's copy of the bits)
        }
    } else if (!strcmp(argv[1], "pose")) {
        double v[7], T[16];
        while (read64(f, v, 7)) {
            rule::pose_from_twist(v, v[6], T);
            for (int j = 0; j < 16; j++) printf("%016" PRIx64 "%c", bits64(T[j]), j == 15 ? '\n' : ' ');
        }
    } else if (!strcmp(argv[1], "twist")) {
        double T[16], xi[6];
        while (read64(f, T, 16)) {
            rule::twist_from_pose(T, xi);
            for (int j = 0; j < 6; j++) printf("%016" PRIx64 "%c", bits64(xi[j]), j == 5 ? '\n' : ' ');
        }
    } else if (!strcmp(argv[1], "between")) {
        for (;;) {
            float T[32]; double scale, xi[6]; uint32_t w; int got = 0;
            for (; got < 32; got++) { if (fscanf(f, "%" SCNx32, &w) != 1) break; T[got] = f32(w); }
            if (got < 32 || !read64(f, &scale, 1)) break;
            rule::twist_between(T, T + 16, scale, xi);
            for (int j = 0; j < 6; j++) printf("%016" PRIx64 "%c", bits64(xi[j]), j == 5 ? '\n' : ' ');
        }
    } else if (!strcmp(argv[1], "check")) {
        static float buf[4096];
        int64_t n, ld, ld_out, so, dof; int32_t mode, period;
        while (fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd32 " %" SCNd32 " %" SCNd64 " %" SCNd64, &n, &ld, &ld_out, &mode, &period, &so, &dof) == 7) {
            const float* src = so < 0 ? nullptr : buf + so;
            const float* dst = dof < 0 ? nullptr : buf + dof;
            printf("%d %d %d\n", rule::shape_ok(n, ld, ld_out) ? 1 : 0, rule::mode_ok(mode, period) ? 1 : 0, rule::overlap(src, ld, dst, ld_out, n));
        }
    } else {
        rc = 2;
    }
    fclose(f);
    return rc;
}
