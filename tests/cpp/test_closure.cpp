// tests/cpp/test_closure.cpp -- the rule of the loop-closure query (icet_amd/csrc/icet_closure.h) on the host: the text the kernels compile, driven by
// tests/test_loop_closure.py, which compares what this prints into files with its NumPy model.
//     test_closure self                   the integer parts of the rule (stamp gaps at the ends of int64, keys), asserted here
//     test_closure start  IN OUT          IN: n x 32 float32 (pose of the live scan, pose of the keyframe, row-major 4 x 4) -> OUT: n x 6 float32 X0
//     test_closure step   IN OUT          IN: n x 6 float32 X                                                            -> OUT: n x 16 float32 T
//     test_closure key    IN OUT          IN: n x 8 float32 (t_q, t_slot, radius, slot)                                  -> OUT: n uint64 keys (all ones: not eligible)
//     test_closure euler  IN OUT          IN: n x 3 float64 angles -> OUT: n x 3 float64 angles after euler_R and euler_of_R
#include "../../icet_amd/csrc/icet_closure.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace rule = icet_closure_rule;

template <class T> static std::vector<T> read_all(const char* path) {
    std::vector<T> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END); const long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    std::fclose(f);
    return v;
}
template <class T> static bool write_all(const char* path, const std::vector<T>& v) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}

#define CHECK(x) do { if (!(x)) { std::printf("FAILED: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static int self_test() {
    const int64_t lo = std::numeric_limits<int64_t>::min(), hi = std::numeric_limits<int64_t>::max();
    CHECK(rule::stamp_gap_ok(5, 5, 0) && rule::stamp_gap_ok(5, 5, -3) && !rule::stamp_gap_ok(5, 5, 1));
    CHECK(rule::stamp_gap_ok(100, 50, 50) && rule::stamp_gap_ok(50, 100, 50) && !rule::stamp_gap_ok(100, 51, 50) && !rule::stamp_gap_ok(51, 100, 50));
    CHECK(rule::stamp_gap_ok(lo, hi, hi) && rule::stamp_gap_ok(hi, lo, hi) && rule::stamp_gap_ok(lo, 0, hi) && !rule::stamp_gap_ok(-1, hi - 2, hi));   // no overflow
    // ties in d2 go to the lower slot; a larger d2 ranks behind whatever the slot; the key gives both back
    CHECK(rule::make_key(1.5f, 3) < rule::make_key(1.5f, 4) && rule::make_key(1.5f, 4000000) < rule::make_key(1.5000001f, 0));
    CHECK(rule::make_key(0.f, 0) == 0 && rule::make_key(std::numeric_limits<float>::infinity(), 0x7fffffff) < rule::kNoKey);
    CHECK(rule::key_slot(rule::make_key(2.25f, 77)) == 77 && rule::key_d2(rule::make_key(2.25f, 77)) == 2.25f && rule::key_slot(rule::kNoKey) == -1);
    // d2 == radius^2 is in, the next float is out, NaN is never a candidate (in the pose or in the query)
    const float nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(rule::candidate_key(3.f, 0.f, 0.f, 0, 0.f, 4.f, 0.f, 0, rule::radius2(5.f), 0, 9) == rule::make_key(25.f, 9));
    CHECK(rule::candidate_key(3.f, 0.f, 0.f, 0, 0.f, 4.f, 0.f, 0, std::nextafter(25.f, 0.f), 0, 9) == rule::kNoKey);
    CHECK(rule::candidate_key(3.f, 0.f, 0.f, 0, nan, 4.f, 0.f, 0, 1e30f, 0, 9) == rule::kNoKey && rule::candidate_key(3.f, 0.f, nan, 0, 0.f, 4.f, 0.f, 0, 1e30f, 0, 9) == rule::kNoKey);
    CHECK(rule::candidate_key(3.f, 0.f, 0.f, 10, 0.f, 4.f, 0.f, 20, 25.f, 11, 9) == rule::kNoKey && rule::candidate_key(3.f, 0.f, 0.f, 10, 0.f, 4.f, 0.f, 20, 25.f, 10, 9) != rule::kNoKey);
    std::printf("self ok\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "self") return self_test();
    if (argc < 4) { std::printf("usage: test_closure self | start|step|key|euler IN OUT\n"); return 2; }
    if (mode == "start") {
        const std::vector<float> in = read_all<float>(argv[2]);
        const size_t n = in.size() / 32;
        std::vector<float> out(n * 6);
        for (size_t i = 0; i < n; i++) rule::start_pose_T(&in[32 * i], &in[32 * i + 16], &out[6 * i]);
        return n > 0 && write_all(argv[3], out) ? 0 : 1;
    }
    if (mode == "step") {
        const std::vector<float> in = read_all<float>(argv[2]);
        const size_t n = in.size() / 6;
        std::vector<float> out(n * 16);
        for (size_t i = 0; i < n; i++) rule::pose_step_from_X(&in[6 * i], &out[16 * i]);
        return n > 0 && write_all(argv[3], out) ? 0 : 1;
    }
    if (mode == "key") {
        const std::vector<float> in = read_all<float>(argv[2]);
        const size_t n = in.size() / 8;
        std::vector<uint64_t> out(n);
        for (size_t i = 0; i < n; i++) {
            const float* r = &in[8 * i];
            out[i] = rule::candidate_key(r[0], r[1], r[2], 0, r[3], r[4], r[5], 0, rule::radius2(r[6]), 0, (int32_t)r[7]);
        }
        return n > 0 && write_all(argv[3], out) ? 0 : 1;
    }
    if (mode == "euler") {
        const std::vector<double> in = read_all<double>(argv[2]);
        const size_t n = in.size() / 3;
        std::vector<double> out(n * 3);
        for (size_t i = 0; i < n; i++) { double R[9]; rule::euler_R(in[3 * i], in[3 * i + 1], in[3 * i + 2], R); rule::euler_of_R(R, &out[3 * i]); }
        return n > 0 && write_all(argv[3], out) ? 0 : 1;
    }
    std::printf("unknown mode %s\n", mode.c_str());
    return 2;
}
