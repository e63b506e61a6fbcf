// tests/cpp/test_buffer_group.cpp -- icet::BufferGroup (icet_amd/csrc/icet_buffers.h) on the host: the four icet::mem functions over malloc, with counters, a
// table of live blocks (a free of anything else, or a second free, ends the program) and a "fail the k-th allocation" switch.  Every block has its exact size, so
// the address sanitizer sees a write past one and a use after release.  What it checks: a refused allocation at every position of a group of six, the
// grow-then-swap of the keyframe store's reserve with a refusal at every position, and the grow step (icet::grow) of a one-buffer group and of a pair with a
// refusal at every position, a retry, a growth that is not needed, and a second call at the old size after a refused growth.
// Build: g++ -std=c++17 -I <repo root> (also with -fsanitize=address,undefined).  Prints one line per case and OK.
#include "icet_amd/csrc/icet_buffers.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>

namespace {
struct Block { size_t bytes; bool pinned; };
std::map<void*, Block> live;
long allocs = 0, frees = 0, calls = 0, fail_at = 0;      // fail_at: the calls-th allocation from now on is refused (0: none)
unsigned last_flags = 0;

[[noreturn]] void die(const char* what, int line) { std::printf("FAILED line %d: %s\n", line, what); std::exit(1); }
#define CHECK(x) do { if (!(x)) die(#x, __LINE__); } while (0)

int alloc(void** p, size_t bytes, bool pinned) {
    if (++calls == fail_at) return 2;                     // (out of memory)
    *p = std::malloc(bytes);
    if (!*p) die("malloc", __LINE__);
    live[*p] = Block{bytes, pinned}; allocs++;
    return 0;
}
int release_block(void* p, bool pinned) {
    const auto it = live.find(p);
    if (it == live.end()) die("free of a block that is not live", __LINE__);
    if (it->second.pinned != pinned) die("free through the wrong function", __LINE__);
    live.erase(it); std::free(p); frees++;
    return 0;
}
void arm(long k) { calls = 0; fail_at = k; }
}  // namespace

int icet::mem::dev_alloc(void** p, size_t bytes) { return alloc(p, bytes, false); }
int icet::mem::dev_free(void* p) { return release_block(p, false); }
int icet::mem::pinned_alloc(void** p, size_t bytes, unsigned flags) { last_flags = flags; return alloc(p, bytes, true); }
int icet::mem::pinned_free(void* p) { return release_block(p, true); }

namespace {
// Six mixed allocations, as an ensure_* makes them: in order, stopping at the first refusal.
struct Six {
    float* a = nullptr; int32_t* b = nullptr; uint64_t* c = nullptr; uint8_t* d = nullptr; double* e = nullptr; int16_t* f = nullptr;
    icet::BufferGroup g;
    void** slot(int k) { void** s[6] = {(void**)&a, (void**)&b, (void**)&c, (void**)&d, (void**)&e, (void**)&f}; return s[k]; }
    static size_t bytes(int k) { const size_t n[6] = {7 * 4, 3 * 4, 5 * 8, 13, 2 * 8, 9 * 2}; return n[k]; }
    int one(int k) {
        switch (k) {
            case 0: return g.device(a, 7);
            case 1: return g.pinned(b, 3, 0x40u);
            case 2: return g.device(c, 5);
            case 3: return g.device(d, 13);
            case 4: return g.pinned(e, 2);
            default: return g.device(f, 9);
        }
    }
    int all() { for (int k = 0; k < 6; k++) { const int e_ = one(k); if (e_) return k + 1; } return 0; }      // 0, or the 1-based position that was refused
};

void six_refused_at(int k) {
    const long a0 = allocs, f0 = frees;
    auto s = std::make_unique<Six>();
    arm(k);
    CHECK(s->all() == k);
    arm(0);
    for (int j = 0; j < 6; j++) {
        if (j < k - 1) { CHECK(*s->slot(j) != nullptr); CHECK(live.at(*s->slot(j)).bytes == Six::bytes(j)); std::memset(*s->slot(j), 0x5A, Six::bytes(j)); }      // earlier slots are live
        else CHECK(*s->slot(j) == nullptr);                                                                                                                          // the refused one (and what was never tried) is null
    }
    CHECK(allocs - a0 == k - 1 && frees == f0);
    s->g.release();
    for (int j = 0; j < 6; j++) CHECK(*s->slot(j) == nullptr);
    CHECK(frees - f0 == allocs - a0 && s->g.empty());
    s->g.release();                                                                                                                                                  // a second release frees nothing
    CHECK(frees - f0 == allocs - a0);
    CHECK(s->all() == 0);                                                                                                                                            // the retry
    for (int j = 0; j < 6; j++) { CHECK(*s->slot(j) != nullptr); std::memset(*s->slot(j), 0xA5, Six::bytes(j)); }
    CHECK(live.at(s->b).pinned && live.at(s->e).pinned && !live.at(s->a).pinned && last_flags == 0u);
    float* none = nullptr;
    CHECK(s->g.device(none, 0) == 0 && none == nullptr && allocs - a0 == (k - 1) + 6);                                                                               // nothing to own: no block, no record
    s.reset();                                                                                                                                                       // the destructor releases
    CHECK(allocs - a0 == (k - 1) + 6 && frees - f0 == allocs - a0);
    std::printf("six, allocation %d refused: %d live before release, slots null after, retry ok\n", k, k - 1);
}

// The store's tables, their owner, and a reserve: a new group beside the old one, the rows carried over, then the swap.
struct Store {
    int32_t cap = 0; uint32_t* rows = nullptr; float* w = nullptr; int32_t* stage = nullptr;
    icet::BufferGroup tables;
};
int tables_alloc(icet::BufferGroup& g, int32_t cap, uint32_t*& rows, float*& w, int32_t*& stage) {
    int e = g.device(rows, (size_t)cap * 5);
    if (!e) e = g.device(w, (size_t)cap);
    if (!e) e = g.pinned(stage, (size_t)cap);
    return e;
}
int reserve(Store* s, int32_t cap) {
    uint32_t* rows = nullptr; float* w = nullptr; int32_t* stage = nullptr;
    icet::BufferGroup fresh;                                                // (behind its slots: it nulls them when it goes)
    const int e = tables_alloc(fresh, cap, rows, w, stage);
    if (e) return e;                                                        // `fresh` frees what it got; the store is untouched
    std::memset(rows, 0xFF, sizeof(uint32_t) * 5 * (size_t)cap); std::memset(w, 0, sizeof(float) * (size_t)cap); std::memset(stage, 0, sizeof(int32_t) * (size_t)cap);
    std::memcpy(rows, s->rows, sizeof(uint32_t) * 5 * (size_t)s->cap); std::memcpy(w, s->w, sizeof(float) * (size_t)s->cap); std::memcpy(stage, s->stage, sizeof(int32_t) * (size_t)s->cap);
    s->tables.swap(fresh);
    CHECK(rows != s->rows && w != s->w && stage != s->stage);               // the locals hold the old tables now, and `fresh` frees them
    s->cap = cap;
    return 0;
}

void reserve_cases() {
    const long a0 = allocs, f0 = frees;
    auto s = std::make_unique<Store>();
    s->cap = 4;
    CHECK(tables_alloc(s->tables, 4, s->rows, s->w, s->stage) == 0);
    for (int i = 0; i < 20; i++) s->rows[i] = 0x9E3779B9u * (uint32_t)(i + 1);
    for (int i = 0; i < 4; i++) { s->w[i] = 0.25f * (float)(i + 1); s->stage[i] = -i; }
    uint32_t rows0[20]; float w0[4]; int32_t st0[4];
    std::memcpy(rows0, s->rows, sizeof(rows0)); std::memcpy(w0, s->w, sizeof(w0)); std::memcpy(st0, s->stage, sizeof(st0));
    void* const p0[3] = {s->rows, s->w, s->stage};
    for (int k = 1; k <= 3; k++) {
        arm(k);
        CHECK(reserve(s.get(), 16) != 0);
        arm(0);
        CHECK(s->cap == 4 && s->rows == p0[0] && s->w == p0[1] && s->stage == p0[2] && live.size() == 3);
        CHECK(!std::memcmp(rows0, s->rows, sizeof(rows0)) && !std::memcmp(w0, s->w, sizeof(w0)) && !std::memcmp(st0, s->stage, sizeof(st0)));
        std::printf("reserve, allocation %d refused: the store keeps its tables, byte for byte\n", k);
    }
    CHECK(reserve(s.get(), 16) == 0);
    CHECK(s->cap == 16 && live.size() == 3);
    CHECK(live.at(s->rows).bytes == 16 * 5 * 4 && live.at(s->w).bytes == 16 * 4 && live.at(s->stage).pinned);
    CHECK(!std::memcmp(rows0, s->rows, sizeof(rows0)) && !std::memcmp(w0, s->w, sizeof(w0)) && !std::memcmp(st0, s->stage, sizeof(st0)));
    CHECK(s->rows[20] == 0xFFFFFFFFu && s->rows[79] == 0xFFFFFFFFu && s->w[15] == 0.f && s->stage[15] == 0);
    s.reset();
    CHECK(live.empty() && frees - f0 == allocs - a0);
    std::printf("reserve: rows carried over, old tables freed once, balance %ld\n", (allocs - a0) - (frees - f0));
}

// The grow step as its callers use it: a capacity check, (the drain), icet::grow.  One buffer sized like a scan (3 floats per row), and a pair like the range
// filter's block counts and bases.
struct Grown {
    float* rows = nullptr; int64_t cap_rows = 0;
    int32_t* counts = nullptr; int32_t* bases = nullptr; int64_t cap_blocks = 0;
    icet::BufferGroup rows_mem, blocks_mem;
};
int ensure_rows(Grown& s, int64_t n) {
    if (n <= s.cap_rows) return 0;
    return icet::grow(s.rows_mem, s.cap_rows, n, [&] { return s.rows_mem.device(s.rows, 3 * (size_t)n); });
}
int ensure_blocks(Grown& s, int64_t n) {
    if (n <= s.cap_blocks) return 0;
    return icet::grow(s.blocks_mem, s.cap_blocks, n, [&] { const int e = s.blocks_mem.device(s.counts, (size_t)n); return e ? e : s.blocks_mem.device(s.bases, (size_t)n); });
}

// `pair`: the counts-and-bases pair (two allocations), else the one buffer.  Grown to 5, then to 40 with allocation k refused, then the retry.
void grow_refused_at(bool pair, int k) {
    const long a0 = allocs, f0 = frees;
    const int per = pair ? 2 : 1;
    auto s = std::make_unique<Grown>();
    auto ensure = [&](int64_t n) { return pair ? ensure_blocks(*s, n) : ensure_rows(*s, n); };
    auto cap = [&] { return pair ? s->cap_blocks : s->cap_rows; };
    auto all_null = [&] { return pair ? (!s->counts && !s->bases) : !s->rows; };
    auto bytes_ok = [&](int64_t n) {
        if (pair) return live.at(s->counts).bytes == 4 * (size_t)n && live.at(s->bases).bytes == 4 * (size_t)n;
        return live.at(s->rows).bytes == 12 * (size_t)n;
    };
    auto fill = [&](int64_t n, int v) { if (pair) { std::memset(s->counts, v, 4 * (size_t)n); std::memset(s->bases, v, 4 * (size_t)n); } else std::memset(s->rows, v, 12 * (size_t)n); };
    CHECK(ensure(5) == 0 && cap() == 5 && bytes_ok(5));
    fill(5, 0x11);
    CHECK(allocs - a0 == per && frees == f0);
    CHECK(ensure(5) == 0 && ensure(3) == 0 && allocs - a0 == per && frees == f0);                   // not needed: nothing allocated, nothing freed
    arm(k);
    CHECK(ensure(40) == 2);                                                                         // the runtime's code
    arm(0);
    CHECK(cap() == 0 && all_null() && s->rows_mem.empty() && s->blocks_mem.empty());
    CHECK(allocs - a0 == per + (k - 1) && frees - f0 == allocs - a0 && live.empty());               // the old blocks and what the refused growth got: each freed once
    // the shape of the two holes: a second call at the OLD size after the refusal must allocate, not "fit"
    CHECK(ensure(5) == 0 && cap() == 5 && !all_null() && bytes_ok(5) && allocs - a0 == 2 * per + (k - 1));
    fill(5, 0x22);
    CHECK(ensure(40) == 0 && cap() == 40 && bytes_ok(40));                                          // the retry: the wanted capacity, exact sizes
    fill(40, 0x33);
    CHECK((int)live.size() == per && allocs - a0 == 3 * per + (k - 1) && frees - f0 == 2 * per + (k - 1));
    s.reset();
    CHECK(live.empty() && frees - f0 == allocs - a0);
    std::printf("grow %s, allocation %d refused: capacity 0 and null slots, old blocks freed once, old size allocates, retry ok, balance %ld\n", pair ? "pair" : "one", k,
                (allocs - a0) - (frees - f0));
}
}  // namespace

int main() {
    for (int k = 1; k <= 6; k++) six_refused_at(k);
    reserve_cases();
    grow_refused_at(false, 1);
    for (int k = 1; k <= 2; k++) grow_refused_at(true, k);
    CHECK(live.empty() && allocs == frees);
    std::printf("allocations %ld, frees %ld\nOK\n", allocs, frees);
    return 0;
}
