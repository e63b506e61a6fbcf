// tests/cpp/test_appearance.cpp -- the rule of the appearance search (icet_amd/csrc/icet_appearance.h) on the host: the text the kernels compile, driven by
// tests/test_appearance.py against the NumPy model (tests/appearance_model.py).  P = sectors rings rho_max z_lo z_hi.
//     test_appearance self                   the parameter ranges, asserted here
//     test_appearance consts  P OUT          -> OUT: 3 float32 kr, ka, kz
//     test_appearance cells   P IN OUT       IN: n x 3 float32 points                         -> OUT: n x 4 int32 (counts, ring, sector, q; zeros when it does not)
//     test_appearance weights P IN OUT       IN: n descriptors (rings x sectors bytes)        -> OUT: n x sectors float32
//     test_appearance dist    P IN OUT       IN: n pairs (Dq bytes, Dc bytes, wq, wc float32) -> OUT: n x (float32 distance, int32 shift)
//     test_appearance yaw     P OUT          -> OUT: sectors float32, the yaw of every shift
// Build: g++ -std=c++17 -O2 -ffp-contract=off tests/cpp/test_appearance.cpp -o <out>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../icet_amd/csrc/icet_appearance.h"

namespace rule = icet_appearance_rule;

static std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> b;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    unsigned char tmp[65536]; size_t k;
    while ((k = std::fread(tmp, 1, sizeof(tmp), f)) > 0) b.insert(b.end(), tmp, tmp + k);
    std::fclose(f);
    return b;
}
static void spill(const char* path, const void* p, size_t bytes) {
    FILE* f = std::fopen(path, "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) { std::perror(path); std::exit(2); }
    std::fclose(f);
}

static int self() {
    int bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED: %s\n", #x); bad++; } } while (0)
    CHECK(rule::params_ok(120, 20, 80.f, -3.f, 12.f));
    CHECK(rule::params_ok(8, 1, 1.f, 0.f, 1.f) && rule::params_ok(360, 64, 200.f, -10.f, 10.f));
    CHECK(!rule::params_ok(6, 20, 80.f, -3.f, 12.f) && !rule::params_ok(362, 20, 80.f, -3.f, 12.f) && !rule::params_ok(121, 20, 80.f, -3.f, 12.f));
    CHECK(!rule::params_ok(120, 0, 80.f, -3.f, 12.f) && !rule::params_ok(120, 65, 80.f, -3.f, 12.f));
    CHECK(!rule::params_ok(120, 20, 0.f, -3.f, 12.f) && !rule::params_ok(120, 20, NAN, -3.f, 12.f) && !rule::params_ok(120, 20, INFINITY, -3.f, 12.f));
    CHECK(!rule::params_ok(120, 20, 80.f, 12.f, 12.f) && !rule::params_ok(120, 20, 80.f, NAN, 12.f) && !rule::params_ok(120, 20, 80.f, -3.f, INFINITY));
    CHECK(rule::min_columns(120) == 30 && rule::min_columns(8) == 2 && rule::min_columns(10) == 3);
    CHECK(rule::column_weight(0) == 0.f && rule::column_weight(4) == 0.5f);
    CHECK(rule::shift_distance(0.0, 29, 120) == INFINITY && rule::shift_distance(30.0, 30, 120) == 0.f && rule::shift_distance(31.0, 30, 120) == 0.f && !std::signbit(rule::shift_distance(31.0, 30, 120)));
    CHECK(rule::candidate_key(0.5f, 0.5f, 0, 0, 0, 3) == icet_closure_rule::make_key(0.5f, 3) && rule::candidate_key(0.6f, 0.5f, 0, 0, 0, 3) == rule::kNoKey);
    CHECK(rule::candidate_key(NAN, INFINITY, 0, 0, 0, 3) == rule::kNoKey && rule::candidate_key(INFINITY, INFINITY, 0, 0, 0, 3) != rule::kNoKey);
    CHECK(rule::candidate_key(0.1f, 1.f, 100, 95, 10, 3) == rule::kNoKey && rule::candidate_key(0.1f, 1.f, 100, 90, 10, 3) != rule::kNoKey);
    CHECK(rule::shift_yaw(0, 120) == 0.f && rule::shift_yaw(60, 120) == (float)3.141592653589793 && rule::shift_yaw(61, 120) < 0.f);
#undef CHECK
    std::printf(bad ? "self FAILED\n" : "self ok\n");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "self") return self();
    if (argc < 8) { std::printf("usage: test_appearance self | consts|yaw P OUT | cells|weights|dist P IN OUT   (P = sectors rings rho_max z_lo z_hi)\n"); return 2; }
    const std::string mode = argv[1];
    const int A = std::atoi(argv[2]), Rn = std::atoi(argv[3]);
    const float rho_max = (float)std::atof(argv[4]), z_lo = (float)std::atof(argv[5]), z_hi = (float)std::atof(argv[6]);
    if (!rule::params_ok(A, Rn, rho_max, z_lo, z_hi)) { std::printf("parameters out of range\n"); return 2; }
    const rule::Consts c = rule::make_consts(A, Rn, rho_max, z_lo, z_hi);
    const size_t cells = (size_t)A * Rn;
    if (mode == "consts") { const float k[3] = {c.kr, c.ka, c.kz}; spill(argv[7], k, sizeof(k)); return 0; }
    if (mode == "yaw") {
        std::vector<float> y((size_t)A);
        for (int s = 0; s < A; s++) y[(size_t)s] = rule::shift_yaw(s, A);
        spill(argv[7], y.data(), sizeof(float) * y.size());
        return 0;
    }
    if (argc < 9) return 2;
    const std::vector<unsigned char> in = slurp(argv[7]);
    if (mode == "cells") {
        const size_t n = in.size() / 12;
        const float* p = reinterpret_cast<const float*>(in.data());
        std::vector<int32_t> out(4 * n, 0);
        for (size_t i = 0; i < n; i++) {
            int ring = 0, sector = 0, q = 0;
            if (rule::cell_of(c, p[3 * i], p[3 * i + 1], p[3 * i + 2], ring, sector, q)) { out[4 * i] = 1; out[4 * i + 1] = ring; out[4 * i + 2] = sector; out[4 * i + 3] = q; }
        }
        spill(argv[8], out.data(), sizeof(int32_t) * out.size());
        return 0;
    }
    if (mode == "weights") {
        const size_t n = in.size() / cells;
        std::vector<float> out(n * A);
        for (size_t i = 0; i < n; i++)
            for (int j = 0; j < A; j++) {
                uint32_t e = 0;
                for (int r = 0; r < Rn; r++) { const uint32_t v = in[i * cells + (size_t)r * A + j]; e += v * v; }
                out[i * A + j] = rule::column_weight(e);
            }
        spill(argv[8], out.data(), sizeof(float) * out.size());
        return 0;
    }
    if (mode == "dist") {
        const size_t rec = 2 * cells + 8 * (size_t)A;
        const size_t n = in.size() / rec;
        std::vector<unsigned char> out(8 * n);
        std::vector<float> wq((size_t)A), wc((size_t)A);
        for (size_t i = 0; i < n; i++) {
            const unsigned char* b = in.data() + i * rec;
            std::memcpy(wq.data(), b + 2 * cells, 4 * (size_t)A); std::memcpy(wc.data(), b + 2 * cells + 4 * (size_t)A, 4 * (size_t)A);
            int shift = 0;
            const float d = rule::distance(b, wq.data(), b + cells, wc.data(), A, Rn, &shift);
            const int32_t s32 = shift;
            std::memcpy(&out[8 * i], &d, 4); std::memcpy(&out[8 * i + 4], &s32, 4);
        }
        spill(argv[8], out.data(), out.size());
        return 0;
    }
    return 2;
}
