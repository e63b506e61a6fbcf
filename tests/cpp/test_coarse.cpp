// tests/cpp/test_coarse.cpp -- the rule of the coarse alignment (icet_amd/csrc/icet_coarse.h) on the host: the text the kernels compile, driven by
// tests/test_coarse.py against the NumPy model (tests/coarse_model.py).  P = cells cell z_lo z_hi min_span.
//     test_coarse self                  the parameter ranges and the key, asserted here
//     test_coarse consts P OUT          -> OUT: float32 kc, kz, int32 span_codes
//     test_coarse points P IN OUT       IN: n x 3 float32 points            -> OUT: n x 5 int32 (counts, ix, iy, q, is a structure point; zeros when it does not count)
//     test_coarse grid   P IN OUT       IN: n x 3 float32 points            -> OUT: G x G / 32 words, the keyframe grid
//     test_coarse live   P IN OUT       IN: X0[6] yaw_step (float32) y f (int32), then points                 -> OUT: 6 float32 M rows, then the live grid's words
//     test_coarse shifts P IN OUT       IN: window h (int32), live words, key words                           -> OUT: (2 window + 1)^2 uint32 scores [a][b], uint64 best key
//     test_coarse search P IN OUT       IN: X0[6] yaw_step (float32) window Y half_turn min_score has_key (int32), key words, then points
//                                       -> OUT: 8 int32 (the match record), 6 float32 start pose, uint64 key
// Build: g++ -std=c++17 -O2 -ffp-contract=off tests/cpp/test_coarse.cpp -o <out>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../icet_amd/csrc/icet_coarse.h"

namespace rule = icet_coarse_rule;

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
    CHECK(rule::params_ok(256, 0.25f, -3.f, 12.f, 0.5f) && rule::params_ok(64, 1.f, 0.f, 1.f, 0.1f) && rule::params_ok(512, 0.1f, -10.f, 10.f, 3.f) && rule::params_ok(96, 0.5f, -3.f, 12.f, 0.5f));
    CHECK(!rule::params_ok(32, 0.25f, -3.f, 12.f, 0.5f) && !rule::params_ok(544, 0.25f, -3.f, 12.f, 0.5f) && !rule::params_ok(100, 0.25f, -3.f, 12.f, 0.5f));
    CHECK(!rule::params_ok(256, 0.f, -3.f, 12.f, 0.5f) && !rule::params_ok(256, -1.f, -3.f, 12.f, 0.5f) && !rule::params_ok(256, NAN, -3.f, 12.f, 0.5f) && !rule::params_ok(256, INFINITY, -3.f, 12.f, 0.5f));
    CHECK(!rule::params_ok(256, 0.25f, 12.f, 12.f, 0.5f) && !rule::params_ok(256, 0.25f, NAN, 12.f, 0.5f) && !rule::params_ok(256, 0.25f, -3.f, INFINITY, 0.5f));
    CHECK(!rule::params_ok(256, 0.25f, -3.f, 12.f, 0.f) && !rule::params_ok(256, 0.25f, -3.f, 12.f, NAN));
    CHECK(rule::n_hypotheses(0, 0) == 1 && rule::n_hypotheses(1, 1) == 6 && rule::n_hypotheses(8, 1) == 34);
    for (int h = 0; h < 6; h++) { int y, f; rule::hypothesis_of(h, 1, y, f); CHECK(f * 3 + (y + 1) == h && y >= -1 && y <= 1 && (f == 0 || f == 1)); }
    // the order: score first, then the smaller shift, then h, a, b; and the key decodes
    CHECK(rule::shift_key(5, 32, 32, 33) > rule::shift_key(4, 0, 0, 0));
    CHECK(rule::shift_key(5, 1, 0, 0) > rule::shift_key(5, 1, 1, 0) && rule::shift_key(5, 0, 0, 3) > rule::shift_key(5, 0, 1, 0));
    CHECK(rule::shift_key(5, 2, 1, 0) > rule::shift_key(5, 2, 1, 1) && rule::shift_key(5, -2, 1, 4) > rule::shift_key(5, 2, -1, 4) && rule::shift_key(5, 1, -2, 4) > rule::shift_key(5, 1, 2, 4));
    CHECK(rule::shift_key(0, 32, 32, 33) != 0);
    for (int a = -32; a <= 32; a += 8) for (int b = -32; b <= 32; b += 4) for (int h = 0; h < 34; h += 11) {
        uint32_t s; int a2, b2, h2;
        rule::key_decode(rule::shift_key(123456u, a, b, h), s, a2, b2, h2);
        CHECK(s == 123456u && a2 == a && b2 == b && h2 == h);
    }
    CHECK(rule::shift_code(-32, 32, 5) == (5 | (0 << 8) | (64 << 16)));
#undef CHECK
    std::printf(bad ? "self FAILED\n" : "self ok\n");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "self") return self();
    if (argc < 8) { std::printf("usage: test_coarse self | consts P OUT | points|grid|live|shifts|search P IN OUT   (P = cells cell z_lo z_hi min_span)\n"); return 2; }
    const std::string mode = argv[1];
    const int G = std::atoi(argv[2]);
    const float cell = (float)std::atof(argv[3]), z_lo = (float)std::atof(argv[4]), z_hi = (float)std::atof(argv[5]), min_span = (float)std::atof(argv[6]);
    if (!rule::params_ok(G, cell, z_lo, z_hi, min_span)) { std::printf("parameters out of range\n"); return 2; }
    const rule::Consts c = rule::make_consts(G, cell, z_lo, z_hi, min_span);
    const size_t words = (size_t)c.G * c.W;
    if (mode == "consts") {
        unsigned char k[12];
        std::memcpy(k, &c.kc, 4); std::memcpy(k + 4, &c.kz, 4); std::memcpy(k + 8, &c.span_codes, 4);
        spill(argv[7], k, sizeof(k));
        return 0;
    }
    if (argc < 9) return 2;
    const std::vector<unsigned char> in = slurp(argv[7]);
    if (mode == "points" || mode == "grid") {
        const size_t n = in.size() / 12;
        const float* p = reinterpret_cast<const float*>(in.data());
        std::vector<uint32_t> grid(words);
        rule::keyframe_grid(c, p, n, grid.data());
        if (mode == "grid") { spill(argv[8], grid.data(), 4 * words); return 0; }
        std::vector<int32_t> out(5 * n, 0);
        for (size_t i = 0; i < n; i++) {
            int ix = 0, iy = 0, q = 0;
            if (rule::count_point(c, p[3 * i], p[3 * i + 1], p[3 * i + 2], ix, iy, q)) {
                out[5 * i] = 1; out[5 * i + 1] = ix; out[5 * i + 2] = iy; out[5 * i + 3] = q; out[5 * i + 4] = rule::get_bit(c, grid.data(), ix, iy) ? 1 : 0;
            }
        }
        spill(argv[8], out.data(), sizeof(int32_t) * out.size());
        return 0;
    }
    if (mode == "live") {
        float X0[6], step; int32_t yf[2];
        std::memcpy(X0, in.data(), 24); std::memcpy(&step, in.data() + 24, 4); std::memcpy(yf, in.data() + 28, 8);
        const float* p = reinterpret_cast<const float*>(in.data() + 36);
        const size_t n = (in.size() - 36) / 12;
        std::vector<uint32_t> own(words), live(words);
        rule::keyframe_grid(c, p, n, own.data());
        double Rh[9]; float m[6];
        rule::hypothesis_rotation(X0, yf[0], yf[1], step, Rh);
        rule::hypothesis_rows(Rh, m);
        rule::live_grid(c, p, n, own.data(), m, X0, live.data());
        std::vector<unsigned char> out(24 + 4 * words);
        std::memcpy(out.data(), m, 24); std::memcpy(out.data() + 24, live.data(), 4 * words);
        spill(argv[8], out.data(), out.size());
        return 0;
    }
    if (mode == "shifts") {
        int32_t wh[2];
        std::memcpy(wh, in.data(), 8);
        const uint32_t* live = reinterpret_cast<const uint32_t*>(in.data() + 8);
        const uint32_t* key = live + words;
        const int M = wh[0], side = 2 * M + 1;
        std::vector<uint32_t> S((size_t)side * side);
        for (int a = -M; a <= M; a++) for (int b = -M; b <= M; b++) S[(size_t)(a + M) * side + (b + M)] = rule::shift_score(c, live, key, a, b);
        const uint64_t best = rule::best_shift(c, live, key, M, wh[1]);
        std::vector<unsigned char> out(4 * S.size() + 8);
        std::memcpy(out.data(), S.data(), 4 * S.size()); std::memcpy(out.data() + 4 * S.size(), &best, 8);
        spill(argv[8], out.data(), out.size());
        return 0;
    }
    if (mode == "search") {
        float X0[6], step; int32_t se[5];
        std::memcpy(X0, in.data(), 24); std::memcpy(&step, in.data() + 24, 4); std::memcpy(se, in.data() + 28, 20);
        const uint32_t* key = reinterpret_cast<const uint32_t*>(in.data() + 48);
        const float* p = reinterpret_cast<const float*>(in.data() + 48 + 4 * words);
        const size_t n = (in.size() - 48 - 4 * words) / 12;
        const int M = se[0], Y = se[1], H = rule::n_hypotheses(Y, se[2]);
        int32_t rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        float X[6];
        for (int k = 0; k < 6; k++) X[k] = X0[k];
        uint64_t best = 0;
        if (se[4]) {
            std::vector<uint32_t> own(words), live(words);
            rule::keyframe_grid(c, p, n, own.data());
            std::vector<uint32_t> bits((size_t)H);
            for (int h = 0; h < H; h++) {
                int y, f; double Rh[9]; float m[6];
                rule::hypothesis_of(h, Y, y, f);
                rule::hypothesis_rotation(X0, y, f, step, Rh);
                rule::hypothesis_rows(Rh, m);
                rule::live_grid(c, p, n, own.data(), m, X0, live.data());
                bits[(size_t)h] = rule::grid_bits(c, live.data());
                const uint64_t k = rule::best_shift(c, live.data(), key, M, h);
                if (k > best) best = k;
            }
            uint32_t s; int a, b, h;
            rule::key_decode(best, s, a, b, h);
            rec[0] = (int32_t)s; rec[1] = a; rec[2] = b; rec[3] = h; rec[4] = (int32_t)bits[(size_t)h]; rec[5] = (int32_t)rule::grid_bits(c, key);
            if ((int64_t)s >= (int64_t)se[3]) {
                rec[6] = 1;
                int y, f; double Rh[9];
                rule::hypothesis_of(h, Y, y, f);
                rule::hypothesis_rotation(X0, y, f, step, Rh);
                rule::start_pose(c, X0, Rh, a, b, y, f, X);
            }
        }
        unsigned char out[64];
        std::memcpy(out, rec, 32); std::memcpy(out + 32, X, 24); std::memcpy(out + 56, &best, 8);
        spill(argv[8], out, sizeof(out));
        return 0;
    }
    return 2;
}
