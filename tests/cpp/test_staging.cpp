// tests/cpp/test_staging.cpp -- the HIP-free rules of icet_amd/csrc/icet_staging.h on the host: the layout of host scans in a staging buffer, the two halves
// of a pair descriptor, the layout of a call's descriptors (offsets, segment table, totals), the unpacking of n x 48 result floats and the check of a call's device scans.
// Build: g++ -std=c++17 -I <repo root> (also with -fsanitize=address,undefined).  Prints one line per case and OK.
#include "icet_amd/csrc/icet_staging.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace icet;

namespace {
[[noreturn]] void die(const char* what, int line) { std::printf("FAILED line %d: %s\n", line, what); std::exit(1); }
#define CHECK(x) do { if (!(x)) die(#x, __LINE__); } while (0)

// Lays `n` out in a buffer of exactly the size the layout asks for, and writes every float of every block once: a block past the end, or two that overlap, shows.
void layout_case(const char* name, const std::vector<int64_t>& n) {
    const int32_t count = (int32_t)n.size();
    const int64_t total = stage_layout(n.data(), count, nullptr, nullptr);
    std::vector<float> buf((size_t)(3 * total), 0.f);      // what ensure_stage allocates: 3 floats per row
    std::vector<icet_dev_scan> d((size_t)count);
    CHECK(stage_layout(n.data(), count, buf.data(), d.data()) == total);
    int64_t sum = 0;
    for (int k = 0; k < count; k++) {
        CHECK(d[k].n == n[k] && d[k].ld == padded_ld(n[k]) && d[k].ld % 64 == 0 && d[k].ld >= n[k] && d[k].ld < n[k] + 64);
        CHECK(d[k].ptr == buf.data() + 3 * sum);          // back to back, in order
        CHECK(n[k] == 0 || dev_scan_ok(d[k]));
        float* p = const_cast<float*>(d[k].ptr);
        for (int64_t i = 0; i < 3 * d[k].ld; i++) { CHECK(p[i] == 0.f); p[i] = 1.f; }
        sum += d[k].ld;
    }
    CHECK(sum == total);
    for (float f : buf) CHECK(f == 1.f);                   // disjoint blocks that cover the buffer
    std::printf("layout %s: %d scans, %lld rows\n", name, count, (long long)total);
}

void layout() {
    CHECK(padded_ld(0) == 0 && padded_ld(1) == 64 && padded_ld(63) == 64 && padded_ld(64) == 64 && padded_ld(65) == 128);
    layout_case("0", {0}); layout_case("1", {1}); layout_case("63", {63}); layout_case("64", {64}); layout_case("65", {65});
    layout_case("mix", {65, 0, 1, 64, 0, 63, 1000, 128});
    layout_case("none", {});
}

void halves() {
    float a[4], b[4];
    const icet_dev_scan s1{a, 100, 128}, s2{b, 90, 96};
    PairDesc d;
    std::memset(&d, 0x5A, sizeof(d));
    set_scan1(d, s1);
    CHECK(d.s1 == a && d.n1 == 100 && d.ld1 == 128 && d.s2 == nullptr && d.n2 == 0 && d.ld2 == 0 && d.off1 == 0 && d.off2 == 0);
    CHECK(same_scan1(d, s1) && !same_scan2(d, s2));
    set_scan2(d, s2);
    CHECK(d.s2 == b && d.n2 == 90 && d.ld2 == 96 && same_scan1(d, s1) && same_scan2(d, s2));
    d.off1 = 7; d.off2 = 9;                                // (lay_out_staging's; a new scan 2 leaves them)
    set_scan2(d, s2);
    CHECK(d.off1 == 7 && d.off2 == 9);
    // one field apart
    CHECK(!same_scan1(d, icet_dev_scan{a, 100, 129}) && !same_scan1(d, icet_dev_scan{a, 99, 128}) && !same_scan1(d, icet_dev_scan{a + 1, 100, 128}));
    CHECK(!same_scan2(d, icet_dev_scan{b, 90, 97}) && !same_scan2(d, icet_dev_scan{b, 89, 96}) && !same_scan2(d, icet_dev_scan{b + 1, 90, 96}));
    // a new scan 1 makes a new pair: the scan-2 half and the offsets are reset
    set_scan1(d, icet_dev_scan{a + 1, 100, 128});
    CHECK(d.s1 == a + 1 && d.s2 == nullptr && d.n2 == 0 && d.ld2 == 0 && d.off1 == 0 && d.off2 == 0 && !same_scan2(d, s2) && !same_scan1(d, s1));
    // the registration staging: no scan 1
    set_scan1(d, icet_dev_scan{nullptr, 0, 0}); set_scan2(d, s2);
    CHECK(d.s1 == nullptr && d.n1 == 0 && d.ld1 == 0 && same_scan2(d, s2));
    std::printf("halves: set, same, one field apart, reset\n");
}

// lay_out_staging: the offsets, the n + 1 segment words and the totals, against values worked out by hand.
bool totals_are(const StagingTotals& t, int64_t tot1, int64_t tot2, int32_t mx1, int32_t mx2, int32_t v4) {
    return t.total_n1 == tot1 && t.total_n2 == tot2 && t.max_n1 == mx1 && t.max_n2 == mx2 && t.vec4_ok == v4;
}
void staging_layout() {
    alignas(16) static float a[16], b[16];                 // b + 1 .. b + 3 are not 16-byte aligned
    {   // no pair: one segment word, nothing else touched (exact sizes: a write past either ends the sanitised run)
        std::vector<int32_t> hs(1, -1);
        CHECK(totals_are(lay_out_staging(nullptr, hs.data(), 0), 0, 0, 0, 0, 1) && hs[0] == 0);
        CHECK(totals_are(lay_out_staging(nullptr, nullptr, 0), 0, 0, 0, 0, 1));
        std::printf("staging layout: no pair\n");
    }
    {   // one pair
        std::vector<PairDesc> d(1); std::vector<int32_t> hs(2, -1);
        set_scan1(d[0], icet_dev_scan{a, 100, 128}); set_scan2(d[0], icet_dev_scan{b, 90, 96});
        d[0].off1 = 7; d[0].off2 = 9;
        CHECK(totals_are(lay_out_staging(d.data(), hs.data(), 1), 100, 90, 100, 90, 1));
        CHECK(d[0].off1 == 0 && d[0].off2 == 0 && hs[0] == 0 && hs[1] == 100);
        CHECK(d[0].s1 == a && d[0].n1 == 100 && d[0].ld1 == 128 && d[0].s2 == b && d[0].n2 == 90 && d[0].ld2 == 96);      // nothing else written
        std::printf("staging layout: one pair\n");
    }
    // three pairs, the middle one with both scans empty (null pointers, which count as aligned)
    auto three = [&](std::vector<PairDesc>& d) {
        d.assign(3, PairDesc{});
        set_scan1(d[0], icet_dev_scan{a, 10, 64});  set_scan2(d[0], icet_dev_scan{b, 7, 8});
        set_scan1(d[1], icet_dev_scan{nullptr, 0, 0}); set_scan2(d[1], icet_dev_scan{nullptr, 0, 0});
        set_scan1(d[2], icet_dev_scan{a, 5, 64});   set_scan2(d[2], icet_dev_scan{b + 4, 11, 12});
    };
    {
        std::vector<PairDesc> d; three(d); std::vector<int32_t> hs(4, -1);
        CHECK(totals_are(lay_out_staging(d.data(), hs.data(), 3), 15, 18, 10, 11, 1));
        CHECK(d[0].off1 == 0 && d[1].off1 == 10 && d[2].off1 == 10 && d[0].off2 == 0 && d[1].off2 == 7 && d[2].off2 == 7);
        CHECK(hs[0] == 0 && hs[1] == 10 && hs[2] == 10 && hs[3] == 15);
        // laying out twice gives the same words
        const std::vector<PairDesc> d_once = d; const std::vector<int32_t> hs_once = hs;
        CHECK(totals_are(lay_out_staging(d.data(), hs.data(), 3), 15, 18, 10, 11, 1));
        CHECK(std::memcmp(d.data(), d_once.data(), sizeof(PairDesc) * 3) == 0 && hs == hs_once);
        // no segment table (an indexed call keeps its keyframe index there): the same offsets and totals
        std::vector<PairDesc> e; three(e);
        CHECK(totals_are(lay_out_staging(e.data(), nullptr, 3), 15, 18, 10, 11, 1));
        CHECK(std::memcmp(e.data(), d.data(), sizeof(PairDesc) * 3) == 0);
        std::printf("staging layout: three pairs, an empty one in the middle; twice; without a segment table\n");
        // a scan-2 pointer, then a leading dimension, that is not 16-byte aligned, in the LAST pair only: everything as before, vec4_ok 0
        set_scan2(d[2], icet_dev_scan{b + 1, 11, 12});
        CHECK(totals_are(lay_out_staging(d.data(), hs.data(), 3), 15, 18, 10, 11, 0) && hs == hs_once && d[2].off1 == 10 && d[2].off2 == 7);
        set_scan2(d[2], icet_dev_scan{b + 4, 11, 13});
        CHECK(totals_are(lay_out_staging(d.data(), hs.data(), 3), 15, 18, 10, 11, 0) && hs == hs_once);
        set_scan2(d[2], icet_dev_scan{b + 4, 11, 12});
        CHECK(totals_are(lay_out_staging(d.data(), hs.data(), 3), 15, 18, 10, 11, 1));
        std::printf("staging layout: unaligned scan 2 in the last pair\n");
        // a new scan 1 in the first pair resets its offsets and its scan-2 half: the next layout moves everything behind it
        set_scan1(d[0], icet_dev_scan{a, 12, 64});
        CHECK(d[0].off1 == 0 && d[0].off2 == 0 && d[0].n2 == 0);
        CHECK(totals_are(lay_out_staging(d.data(), hs.data(), 3), 17, 11, 12, 11, 1));
        CHECK(d[0].off1 == 0 && d[1].off1 == 12 && d[2].off1 == 12 && d[0].off2 == 0 && d[1].off2 == 0 && d[2].off2 == 0);
        CHECK(hs[0] == 0 && hs[1] == 12 && hs[2] == 12 && hs[3] == 17);
        // ... and in the LAST pair, whose own offsets the reset zeroed: the layout puts them back
        set_scan1(d[2], icet_dev_scan{a, 5, 64});
        CHECK(d[2].off1 == 0 && d[2].off2 == 0);
        CHECK(totals_are(lay_out_staging(d.data(), hs.data(), 3), 17, 0, 12, 0, 1) && d[2].off1 == 12 && d[2].off2 == 0 && hs[3] == 17);
        std::printf("staging layout: after a set_scan1 reset\n");
    }
}

void unpack() {
    const int n = 3;
    std::vector<float> res((size_t)48 * n);
    for (size_t i = 0; i < res.size(); i++) res[i] = (float)i;
    for (int with_cov = 0; with_cov < 2; with_cov++) {
        std::vector<float> x((size_t)6 * n, -1.f), ps((size_t)6 * n, -1.f), cov((size_t)36 * n, -1.f);      // exact sizes: a write past one ends the sanitised run
        unpack_results(res.data(), n, x.data(), ps.data(), with_cov ? cov.data() : nullptr);
        for (int k = 0; k < n; k++) {
            for (int i = 0; i < 6; i++) CHECK(x[6 * k + i] == (float)(48 * k + i) && ps[6 * k + i] == (float)(48 * k + 6 + i));
            for (int i = 0; i < 36; i++) CHECK(cov[36 * k + i] == (with_cov ? (float)(48 * k + 12 + i) : -1.f));
        }
        std::printf("unpack %d x 48: cov %s\n", n, with_cov ? "given" : "null");
    }
    unpack_results(res.data(), 0, nullptr, nullptr, nullptr);      // nothing to do, nothing touched
}

void scans() {
    float a[4];
    const icet_dev_scan good[3] = {{a, 10, 10}, {nullptr, 0, 0}, {a, 5, ((int64_t)1 << 30) - 1}};
    int64_t rows = -1;
    CHECK(dev_scans_ok(good, 3, &rows) && rows == 15);
    CHECK(dev_scans_ok(good, 0, &rows) && rows == 0);
    const icet_dev_scan bad[4] = {{a, -1, 10}, {a, 10, 9}, {nullptr, 1, 1}, {a, 5, (int64_t)1 << 30}};
    const char* why[4] = {"n < 0", "ld < n", "null with n > 0", "ld >= 2^30"};
    for (int b = 0; b < 4; b++) {
        CHECK(!dev_scan_ok(bad[b]));
        for (int at = 0; at < 3; at++) {                   // wherever it stands among good ones
            icet_dev_scan s[3] = {good[0], good[1], good[2]};
            s[at] = bad[b];
            CHECK(!dev_scans_ok(s, 3, &rows));
        }
        std::printf("scan check: %s refused\n", why[b]);
    }
}
}  // namespace

int main() {
    layout();
    halves();
    staging_layout();
    unpack();
    scans();
    std::printf("OK\n");
    return 0;
}
