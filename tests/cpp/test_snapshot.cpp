// tests/cpp/test_snapshot.cpp -- icet_amd/csrc/icet_snapshot.h on its own (tests/test_snapshot.py builds and runs this with AddressSanitizer + UBSan; host code,
// its own executable).  Modes:
//   selftest            synthetic images (V = 21 and V = 1800; entries of 0, 1 and V records; with and without each feature): write -> parse gives every field
//                       and byte back; every proper prefix is refused; every single-byte change is refused; images with valid checksums and bad contents are
//                       refused -- all without an out-of-range read.
//   write OUT           one synthetic image into the file OUT (tests/snapshot_model.py must read it and write the same bytes)
//   rewrite IN OUT      the file IN (written by tests/snapshot_model.py) parsed and written again from its contents into OUT: the same bytes
#include "../../icet_amd/csrc/icet_snapshot.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace icet_snapshot;
typedef std::vector<uint8_t> Bytes;
static const uint32_t kLayout = 1;

struct Ent {
    int32_t slot = 0; int64_t stamp = -1; bool has_pose = false, has_desc = false, has_grid = false; uint32_t pose[12];
    std::vector<uint32_t> hot, fit, desc, w, grid; std::vector<int16_t> sov;
};
struct Img { Header h; std::vector<Ent> e; };

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static uint64_t rng_state = 1;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 32); }

static void put_words(Bytes& b, uint64_t at, const void* src, uint64_t bytes) { if (bytes) memcpy(b.data() + at, src, bytes); }

static Bytes build(const Img& im) {
    Header h = im.h;
    h.n_entries = (uint32_t)im.e.size();
    std::vector<Entry> dir(im.e.size());
    uint64_t at = directory_end(h.n_entries);
    for (size_t k = 0; k < im.e.size(); k++) {
        const Ent& s = im.e[k];
        Entry& d = dir[k];
        d.slot = s.slot; d.n_slots = (int32_t)(s.hot.size() / 12); d.stamp = s.stamp;
        d.flags = (s.has_pose ? kFlagPose : 0) | (s.has_desc ? kFlagDesc : 0) | (s.has_grid ? kFlagGrid : 0);
        for (int j = 0; j < 12; j++) d.pose[j] = s.has_pose ? s.pose[j] : 0xFFFFFFFFu;
        d.off = at; d.bytes = layout(h.V, d.n_slots, d.flags, h.A(), h.Rp(), h.G()).size; d.sum = 0;
        at += d.bytes;
    }
    h.file_bytes = at;
    Bytes b((size_t)at, 0);
    for (size_t k = 0; k < im.e.size(); k++) {
        const Ent& s = im.e[k];
        const Layout l = layout(h.V, dir[k].n_slots, dir[k].flags, h.A(), h.Rp(), h.G());
        const uint64_t o = dir[k].off;
        put_words(b, o + l.hot, s.hot.data(), 4 * s.hot.size()); put_words(b, o + l.fit, s.fit.data(), 4 * s.fit.size());
        CHECK(2 * s.sov.size() == l.sov_bytes);
        put_words(b, o + l.sov, s.sov.data(), l.sov_bytes);
        if (s.has_desc) { CHECK(4 * s.desc.size() == l.desc_bytes && 4 * s.w.size() == l.w_bytes); put_words(b, o + l.desc, s.desc.data(), l.desc_bytes); put_words(b, o + l.w, s.w.data(), l.w_bytes); }
        if (s.has_grid) { CHECK(o + l.grid + 4 * s.grid.size() == o + l.size); put_words(b, o + l.grid, s.grid.data(), 4 * s.grid.size()); }
        dir[k].sum = checksum(b.data() + o, dir[k].bytes);
    }
    put_header(b.data(), h, kLayout);
    for (size_t k = 0; k < dir.size(); k++) put_entry(b.data() + kHeaderBytes + (size_t)kEntryBytes * k, dir[k]);
    seal(b.data(), h.n_entries);
    return b;
}

static bool valid(const Bytes& b, Header* h = nullptr, std::vector<Entry>* e = nullptr, const char** why = nullptr) {
    // an exact-size heap copy: the sanitizers see any read behind the image
    uint8_t* p = (uint8_t*)std::malloc(b.size() ? b.size() : 1);
    if (!b.empty()) memcpy(p, b.data(), b.size());
    std::vector<Entry> ent(b.size() / kEntryBytes + 1);
    Header hd;
    const bool ok = validate(p, b.size(), kLayout, &hd, ent.data(), ent.size(), why);
    std::free(p);
    if (ok && h) *h = hd;
    if (ok && e) { ent.resize(hd.n_entries); *e = ent; }
    return ok;
}

static bool parse(const Bytes& b, Img& im) {
    std::vector<Entry> dir;
    if (!valid(b, &im.h, &dir)) return false;
    im.e.clear();
    for (const Entry& d : dir) {
        Ent s;
        const Layout l = layout(im.h.V, d.n_slots, d.flags, im.h.A(), im.h.Rp(), im.h.G());
        const uint8_t* q = b.data() + d.off;
        s.slot = d.slot; s.stamp = d.stamp; s.has_pose = d.flags & kFlagPose; s.has_desc = d.flags & kFlagDesc; s.has_grid = d.flags & kFlagGrid;
        memcpy(s.pose, d.pose, sizeof(s.pose));
        s.hot.resize(12 * (size_t)d.n_slots); s.fit.resize(20 * (size_t)d.n_slots); s.sov.resize(l.sov_bytes / 2);
        if (d.n_slots) { memcpy(s.hot.data(), q + l.hot, 4 * s.hot.size()); memcpy(s.fit.data(), q + l.fit, 4 * s.fit.size()); }
        memcpy(s.sov.data(), q + l.sov, l.sov_bytes);
        if (s.has_desc) { s.desc.resize(l.desc_bytes / 4); s.w.resize(l.w_bytes / 4); memcpy(s.desc.data(), q + l.desc, l.desc_bytes); memcpy(s.w.data(), q + l.w, l.w_bytes); }
        if (s.has_grid) { s.grid.resize((l.size - l.grid) / 4); memcpy(s.grid.data(), q + l.grid, l.size - l.grid); }
        im.e.push_back(s);
    }
    return true;
}

static Img synthetic(int bins_theta, int bins_phi, const std::vector<int>& n_slots, bool app, bool coarse) {
    Img im;
    memset(&im.h, 0, sizeof(im.h));
    im.h.bins_phi = bins_phi; im.h.bins_theta = bins_theta; im.h.n = 25; im.h.thresh_bits = 0x3DCCCCCDu; im.h.buff_bits = 0x3DCCCCCDu; im.h.V = bins_phi * bins_theta;
    const float f[4] = {80.f, -3.f, 12.f, 0.25f};
    uint32_t fb[4]; memcpy(fb, f, sizeof(fb));
    if (app) { im.h.features |= kHasAppearance; im.h.app[0] = 10; im.h.app[1] = 5; im.h.app[2] = fb[0]; im.h.app[3] = fb[1]; im.h.app[4] = fb[2]; }      // 10 sectors, 5 rings: Rp = 2, padded parts
    if (coarse) { im.h.features |= kHasCoarse; im.h.coarse[0] = 64; im.h.coarse[1] = fb[3]; im.h.coarse[2] = fb[1]; im.h.coarse[3] = fb[2]; im.h.coarse[4] = fb[3]; }
    const int V = im.h.V;
    for (size_t k = 0; k < n_slots.size(); k++) {
        Ent s;
        const int ns = n_slots[k];
        s.slot = 3 * (int)k + 1; s.has_pose = k % 2 == 0; s.stamp = s.has_pose ? 1000 + (int64_t)k : (k == 1 ? 77 : -1);
        for (int j = 0; j < 12; j++) s.pose[j] = rnd() & 0x7FFFFFFFu;
        s.hot.resize(12 * (size_t)ns); s.fit.resize(20 * (size_t)ns); s.sov.assign(((size_t)V + 1) & ~(size_t)1, -1);
        for (auto& v : s.hot) v = rnd();
        for (auto& v : s.fit) v = rnd();
        for (int i = 0; i < ns; i++) { const int v = (i + 5 * (int)k) % V; s.hot[12 * i + 9] = (uint32_t)v; s.fit[20 * i + 19] = (uint32_t)v; s.sov[v] = (int16_t)i; }
        if (app && k != 1) { s.has_desc = true; s.desc.resize(10 * 2); s.w.resize(10); for (auto& v : s.desc) v = rnd(); for (auto& v : s.w) v = rnd(); }
        if (coarse && k != 0) { s.has_grid = true; s.grid.resize(64 * 64 / 32); for (auto& v : s.grid) v = rnd(); }
        im.e.push_back(s);
    }
    return im;
}

static bool same(const Img& a, const Img& b) {
    const Header &g = a.h, &h = b.h;
    if (g.bins_phi != h.bins_phi || g.bins_theta != h.bins_theta || g.n != h.n || g.thresh_bits != h.thresh_bits || g.buff_bits != h.buff_bits || g.shape_flags != h.shape_flags ||
        g.V != h.V || g.features != h.features || memcmp(g.app, h.app, sizeof(g.app)) != 0 || memcmp(g.coarse, h.coarse, sizeof(g.coarse)) != 0 || a.e.size() != b.e.size()) return false;
    for (size_t k = 0; k < a.e.size(); k++) {
        const Ent &x = a.e[k], &y = b.e[k];
        if (x.slot != y.slot || x.stamp != y.stamp || x.has_pose != y.has_pose || x.has_desc != y.has_desc || x.has_grid != y.has_grid) return false;
        if (x.has_pose && memcmp(x.pose, y.pose, sizeof(x.pose)) != 0) return false;
        if (x.hot != y.hot || x.fit != y.fit || x.sov != y.sov || x.desc != y.desc || x.w != y.w || x.grid != y.grid) return false;
    }
    return true;
}

// Directory entry k of an image, read and written in place; the checksums above it made valid again.
static Entry get_entry(const Bytes& b, size_t k) {
    const uint8_t* p = b.data() + kHeaderBytes + kEntryBytes * k;
    Entry e; e.slot = (int32_t)get32(p); e.n_slots = (int32_t)get32(p + 4); e.flags = get32(p + 8); e.stamp = (int64_t)get64(p + 16);
    for (int j = 0; j < 12; j++) e.pose[j] = get32(p + 24 + 4 * j);
    e.off = get64(p + 72); e.bytes = get64(p + 80); e.sum = get64(p + 88);
    return e;
}
static void set_entry(Bytes& b, size_t k, const Entry& e) { put_entry(b.data() + kHeaderBytes + kEntryBytes * k, e); seal(b.data(), get32(b.data() + 56)); }
static void reseal_payload(Bytes& b, size_t k) { Entry e = get_entry(b, k); e.sum = checksum(b.data() + e.off, e.bytes); set_entry(b, k, e); }

static void refused(const Bytes& b, const char* what) {
    const char* why = "";
    if (valid(b, nullptr, nullptr, &why)) { std::fprintf(stderr, "an image with %s was accepted\n", what); std::exit(1); }
}

// Every proper prefix; every single-byte change.  Images below `exhaustive_below` bytes: all of them.  Above: the header, the directory, 64 bytes around every
// part's edge and every 61st byte of the rest (each byte lies in exactly one checksummed range: the places differ only in which range refuses).
static void prefixes_and_flips(const Bytes& b, size_t exhaustive_below) {
    std::vector<uint8_t> pick(b.size() + 1, b.size() < exhaustive_below);
    if (b.size() >= exhaustive_below) {
        Header h; std::vector<Entry> dir;
        CHECK(valid(b, &h, &dir));
        auto mark = [&](uint64_t at) { for (uint64_t i = at > 64 ? at - 64 : 0; i < at + 64 && i < pick.size(); i++) pick[i] = 1; };
        for (uint64_t i = 0; i < directory_end(h.n_entries); i++) pick[i] = 1;
        mark(directory_end(h.n_entries)); mark(b.size());
        for (const Entry& d : dir) {
            const Layout l = layout(h.V, d.n_slots, d.flags, h.A(), h.Rp(), h.G());
            for (uint32_t o : {l.hot, l.fit, l.sov, l.desc, l.w, l.grid, l.size}) mark(d.off + o);
        }
        for (size_t i = 0; i < pick.size(); i += 61) pick[i] = 1;
    }
    size_t tried = 0;
    for (size_t n = 0; n < b.size(); n++) {
        if (!pick[n]) continue;
        if (valid(Bytes(b.begin(), b.begin() + n))) { std::fprintf(stderr, "the prefix of %zu bytes was accepted\n", n); std::exit(1); }
        tried++;
    }
    // one exact-size heap copy, changed in place: the sanitizers see any read behind the image
    uint8_t* c = (uint8_t*)std::malloc(b.size());
    CHECK(c);
    memcpy(c, b.data(), b.size());
    std::vector<Entry> ent(b.size() / kEntryBytes + 1);
    Header hd;
    for (size_t i = 0; i < b.size(); i++) {
        if (!pick[i]) continue;
        for (uint8_t x : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xFF}) {
            c[i] = b[i] ^ x;
            if (validate(c, b.size(), kLayout, &hd, ent.data(), ent.size(), nullptr)) { std::fprintf(stderr, "byte %zu ^ 0x%02x was accepted\n", i, x); std::exit(1); }
        }
        c[i] = b[i]; tried++;
    }
    CHECK(tried > 0 && validate(c, b.size(), kLayout, &hd, ent.data(), ent.size(), nullptr));
    std::free(c);
}

static void bad_contents(const Img& good) {       // entry 2 holds V records, entry 1 one, entry 0 none
    const Bytes ok = build(good);
    CHECK(valid(ok));
    const int V = good.h.V;
    { Img m = good; for (int v = 0; v < V; v++) if (m.e[1].sov[v] < 0) { m.e[1].sov[v] = 1; break; } refused(build(m), "a slot_of_voxel entry >= n_slots"); }
    { Img m = good; m.e[1].sov[V - 1] = (int16_t)-2; if (good.e[1].sov[V - 1] < 0) refused(build(m), "a slot_of_voxel entry < -1"); }
    { Img m = good; m.e[2].hot[12 * 3 + 9] = (uint32_t)V; refused(build(m), "a SlotHot voxel >= V"); }
    { Img m = good; m.e[2].fit[20 * 3 + 19] = 0x80000000u; refused(build(m), "a negative SlotFit voxel"); }
    { Img m = good; m.e[1].fit[19] = 0x7FFFFFFFu; refused(build(m), "a huge SlotFit voxel"); }
    { Img m = good; std::swap(m.e[2].hot[12 * 2 + 9], m.e[2].hot[12 * 5 + 9]); refused(build(m), "slot_of_voxel[voxel_i] != i (hot)"); }
    { Img m = good; std::swap(m.e[2].sov[0], m.e[2].sov[1]); refused(build(m), "slot_of_voxel[voxel_i] != i (swapped entries)"); }
    { Img m = good; m.e[1].slot = m.e[2].slot; m.e[2].slot = good.e[1].slot; refused(build(m), "descending slots"); }
    { Img m = good; m.e[2].slot = m.e[1].slot; refused(build(m), "a repeated slot"); }
    { Img m = good; m.e[0].slot = -1; refused(build(m), "a negative slot"); }
    { Bytes b = ok; Entry e = get_entry(b, 2); e.off = get_entry(b, 1).off; set_entry(b, 2, e); reseal_payload(b, 2); refused(b, "overlapping payloads"); }
    { Bytes b = ok; Entry e1 = get_entry(b, 1), e2 = get_entry(b, 2); if (e2.bytes >= e1.bytes) { e2.off = e1.off; e1.off = e2.off + e2.bytes; set_entry(b, 1, e1); set_entry(b, 2, e2); }
      refused(b, "payloads out of order"); }
    { Bytes b = ok; b.resize(b.size() + 16, 0); put64(b.data() + 128, b.size()); seal(b.data(), get32(b.data() + 56)); refused(b, "sizes that do not add up to the file's size"); }
    { Bytes b = ok; put64(b.data() + 128, b.size() + 16); seal(b.data(), get32(b.data() + 56)); refused(b, "a file size the file does not have"); }
    { Bytes b = ok; Entry e = get_entry(b, 2); e.off = 0xFFFFFFFFFFFFFFF0ull; set_entry(b, 2, e); refused(b, "an offset whose end wraps around 2^64"); }
    { Bytes b = ok; Entry e = get_entry(b, 2); e.bytes = 0xFFFFFFFFFFFFFFF0ull; set_entry(b, 2, e); refused(b, "a size whose end wraps around 2^64"); }
    { Bytes b = ok; Entry e = get_entry(b, 1); e.off += 8; set_entry(b, 1, e); refused(b, "a misaligned offset"); }
    { Bytes b = ok; Entry e = get_entry(b, 1); e.n_slots = V + 1; set_entry(b, 1, e); refused(b, "n_slots > V"); }
    { Bytes b = ok; Entry e = get_entry(b, 1); e.n_slots = -1; set_entry(b, 1, e); refused(b, "n_slots < 0"); }
    { Bytes b = ok; put32(b.data() + 56, 0x7FFFFFFFu); seal(b.data(), 3); refused(b, "an entry count the file cannot hold"); }
    { Bytes b = ok; put32(b.data() + 52, kLayout + 1); seal(b.data(), 3); refused(b, "another slot-layout version"); }
    { Bytes b = ok; b[150] = 1; seal(b.data(), 3); refused(b, "a reserved header byte set"); }
    { Bytes b = ok; b[kHeaderBytes + 100] = 1; seal(b.data(), 3); refused(b, "a reserved directory byte set"); }
    { Bytes b = ok; const Entry e = get_entry(b, 0); const Layout l = layout(V, e.n_slots, e.flags, good.h.A(), good.h.Rp(), good.h.G());
      if (pad16(l.sov_bytes) != l.sov_bytes) { b[e.off + l.sov + l.sov_bytes] = 1; reseal_payload(b, 0); refused(b, "padding that is not zero"); } }
}

static void selftest() {
    size_t images = 0;
    for (int big = 0; big < 2; big++) for (int app = 0; app < 2; app++) for (int coarse = 0; coarse < 2; coarse++) {
        const int bt = big ? 75 : 7, bp = big ? 24 : 3, V = bt * bp;
        const Img im = synthetic(bt, bp, {0, 1, V}, app, coarse);
        const Bytes b = build(im);
        Img back;
        CHECK(parse(b, back) && same(im, back));            // 1 every field and byte
        CHECK(build(back) == b);
        if (!big) prefixes_and_flips(b, (size_t)1 << 30);      // 2, 3 exhaustively
        else {
            prefixes_and_flips(build(synthetic(bt, bp, {0, 1}, app, coarse)), (size_t)1 << 30);      // V = 1800, the short entries: exhaustively
            if (app && coarse) prefixes_and_flips(b, 0);                                                // and the entry of V records
        }
        bad_contents(im);                                   // 4
        images++;
    }
    { const Img none = synthetic(7, 3, {}, true, false); const Bytes b = build(none); Img back; CHECK(parse(b, back) && same(none, back) && b.size() == kHeaderBytes); prefixes_and_flips(b, 4096); }
    std::printf("snapshot ok: %zu images\n", images);
}

static Bytes slurp(const char* path) {
    FILE* f = std::fopen(path, "rb"); CHECK(f);
    Bytes b; uint8_t buf[4096]; size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    std::fclose(f);
    return b;
}
static void spill(const char* path, const Bytes& b) { FILE* f = std::fopen(path, "wb"); CHECK(f); CHECK(std::fwrite(b.data(), 1, b.size(), f) == b.size()); std::fclose(f); }

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "selftest";
    if (mode == "selftest") { selftest(); return 0; }
    if (mode == "write" && argc == 3) { spill(argv[2], build(synthetic(7, 3, {0, 1, 21, 5}, true, true))); return 0; }
    if (mode == "rewrite" && argc == 4) {
        const Bytes in = slurp(argv[2]);
        Img im;
        const char* why = "";
        if (!valid(in, nullptr, nullptr, &why)) { std::fprintf(stderr, "refused: %s\n", why); return 2; }
        CHECK(parse(in, im));
        spill(argv[3], build(im));
        return 0;
    }
    std::fprintf(stderr, "usage: test_snapshot selftest | write OUT | rewrite IN OUT\n");
    return 64;
}
