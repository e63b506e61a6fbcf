// tests/cpp/test_map_register_neighbours.cpp -- the neighbourhood rule of the registration against a shaped voxel map (icet_amd/csrc/icet_map_register.h, the text
// the kernels compile) as a stand-alone host program, for tests/test_map_register_neighbours_host.py.  Built with g++ -ffp-contract=off.  The formats are those of
// tests/cpp/test_map_register_rule.cpp -- every float the hexadecimal of its bits, every double 16 hex digits, counts, keys and table words decimal -- with the
// neighbourhood (1, 7 or 27) added:
//   rows FILE    line 1: cell min_range max_range scale N K n; then K lines key mu[3] W[6] (ascending keys); then n lines of 12 pose doubles (R row-major, t) and 3
//                row floats.  Prints per row: class key matched s omega rho v[0..27], matched = 1 + the winner's place, 0 for a miss.
//   loop FILE    line 1: cell min_range max_range sigma_min scale tol_t tol_r lambda0 min_points min_matched max_iters E Q N; then E lines key n sum_0..2 w_0..8;
//                then per query: 16 pose floats, n, and n lines of 3 row floats.  The whole call on the CPU through the header's bodies against exact-size
//                buffers: an open-addressing table, the Gaussians, one partial per (query, chunk), the steps.  Prints per query the record.
//   flags        prints neighbours_of(flags) for flags -1 .. 9.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/icet_hip.h"
#include "../../icet_amd/csrc/icet_map_register.h"

namespace rr = icet_map_register_rule;
namespace mrule = icet_map_rule;
namespace srule = icet_map_shape_rule;

static_assert(rr::kFlagNeighbours7 == ICET_VOXEL_MAP_REG_NEIGHBOURS_7 && rr::kFlagNeighbours27 == ICET_VOXEL_MAP_REG_NEIGHBOURS_27, "the flags the header names");

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static double from_bits64(uint64_t b) { double f; memcpy(&f, &b, 8); return f; }
static uint64_t to_bits64(double f) { uint64_t b; memcpy(&b, &f, 8); return b; }

static bool rd_f(FILE* f, float& v) { uint32_t b; if (fscanf(f, "%" SCNx32, &b) != 1) return false; v = from_bits(b); return true; }
static bool rd_d(FILE* f, double& v) { uint64_t b; if (fscanf(f, "%" SCNx64, &b) != 1) return false; v = from_bits64(b); return true; }
static bool rd_u(FILE* f, uint64_t& v) { return fscanf(f, "%" SCNu64, &v) == 1; }
static bool rd_i(FILE* f, int64_t& v) { return fscanf(f, "%" SCNd64, &v) == 1; }
static void pr_d(double v) { printf(" %016" PRIx64, to_bits64(v)); }

// The selection of one row over the cells a look-up finds: find(key) gives the Gaussian of a key, or NULL.  The winner, or NULL, and its place.
template <class Find>
static const rr::Gauss* select_cell(int N, uint64_t own, const double w[3], Find find, int& place) {
    rr::Best best;
    rr::best_start(best);
    const rr::Gauss* win = nullptr;
    for (int j = 0; j < N; j++) {
        uint64_t key;
        if (N == 1) key = own;
        else if (!rr::neighbour_key(N, j, own, key)) continue;
        const rr::Gauss* G = find(key);
        if (G && G->n > 0 && rr::best_offer(best, j, rr::match_s(*G, w))) win = G;
    }
    place = best.place;
    // the cells offered in the reverse order under the (s, place) rule -- what a kernel that does not walk the places in order uses -- select the same cell
    rr::Best any;
    rr::best_start(any);
    const rr::Gauss* win_any = nullptr;
    for (int j = N - 1; j >= 0; j--) {
        uint64_t key;
        if (N == 1) key = own;
        else if (!rr::neighbour_key(N, j, own, key)) continue;
        const rr::Gauss* G = find(key);
        if (G && G->n > 0 && rr::best_offer_any(any, j, rr::match_s(*G, w))) win_any = G;
    }
    if (any.place != best.place || win_any != win) { fprintf(stderr, "the order of the offers changed the selection\n"); exit(6); }
    if (N == 27 && place >= 0) {                                       // place27 is the inverse of the order of the places
        int32_t d[3];
        rr::neighbour_offset(27, place, d);
        if (rr::place27(d[0], d[1], d[2]) != place) exit(7);
    }
    return win;
}

static int run_rows(FILE* f) {
    float cell, mn, mx; double scale; int64_t N, K, n;
    if (!rd_f(f, cell) || !rd_f(f, mn) || !rd_f(f, mx) || !rd_d(f, scale) || !rd_i(f, N) || !rd_i(f, K) || !rd_i(f, n)) return 3;
    if (N != 1 && N != 7 && N != 27) return 5;
    const rr::Consts k = rr::make_consts(cell, mn, mx, 0.02, scale, 0.0, 0.0, 1.0, 1, 0, 0);
    std::vector<uint64_t> keys((size_t)K);
    std::vector<rr::Gauss> G((size_t)K);
    for (int64_t i = 0; i < K; i++) {
        if (!rd_u(f, keys[(size_t)i])) return 3;
        for (int a = 0; a < 3; a++) if (!rd_d(f, G[(size_t)i].mu[a])) return 3;
        for (int j = 0; j < 6; j++) if (!rd_d(f, G[(size_t)i].W[j])) return 3;
        G[(size_t)i].n = 1;
    }
    auto find = [&](uint64_t key) -> const rr::Gauss* {
        int64_t lo = 0, hi = K;                                        // the first key not below `key`
        while (lo < hi) { const int64_t mid = (lo + hi) / 2; if (keys[(size_t)mid] < key) lo = mid + 1; else hi = mid; }
        return lo < K && keys[(size_t)lo] == key ? &G[(size_t)lo] : nullptr;
    };
    for (int64_t i = 0; i < n; i++) {
        rr::Pose P; float p[3];
        for (int j = 0; j < 9; j++) if (!rd_d(f, P.R[j])) return 3;
        for (int a = 0; a < 3; a++) if (!rd_d(f, P.t[a])) return 3;
        for (int a = 0; a < 3; a++) if (!rd_f(f, p[a])) return 3;
        int cls = rr::row_class(k, p[0], p[1], p[2]);
        uint64_t key = mrule::kEmpty; int place = -1;
        rr::Terms tm; tm.s = tm.omega = tm.rho = 0.0;
        for (int j = 0; j < rr::kSums; j++) tm.v[j] = 0.0;
        if (cls == mrule::kRowKept) {
            double r[3], w[3];
            const bool in = rr::row_world(k, P, p[0], p[1], p[2], r, w, key);
            if (!in) cls = mrule::kRowOutside;
            const rr::Gauss* win = in ? select_cell((int)N, key, w, find, place) : nullptr;
            if (win) rr::match_terms(k, *win, r, w, tm);
            else rr::miss_terms(k, tm);
        }
        printf("%d %" PRIu64 " %d", cls, key, place + 1);
        pr_d(tm.s); pr_d(tm.omega); pr_d(tm.rho);
        for (int j = 0; j < rr::kSums; j++) pr_d(tm.v[j]);
        printf("\n");
    }
    return 0;
}

struct Entry { uint64_t key; int64_t n; uint64_t sum[3], w[srule::kWords]; };
static bool rd_entry(FILE* f, Entry& e) {
    if (!rd_u(f, e.key) || !rd_i(f, e.n)) return false;
    for (int a = 0; a < 3; a++) if (!rd_u(f, e.sum[a])) return false;
    for (int j = 0; j < srule::kWords; j++) if (!rd_u(f, e.w[j])) return false;
    return true;
}

// the entry of `key` in the table of size 2^log2, or -1: the kernels' probe
static int64_t probe(const std::vector<uint64_t>& tkey, uint32_t log2, uint64_t key) {
    const uint64_t mask = ((uint64_t)1 << log2) - 1;
    uint64_t h = mrule::mix(key) & mask;
    for (uint64_t p = 0; p <= mask; p++) {
        const uint64_t k = tkey[(size_t)h];
        if (k == key) return (int64_t)h;
        if (k == mrule::kEmpty) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

static int run_loop(FILE* f) {
    float cell, mn, mx; double sigma, scale, tol_t, tol_r, lambda0; int64_t minp, minm, iters, E, Q, N;
    if (!rd_f(f, cell) || !rd_f(f, mn) || !rd_f(f, mx) || !rd_d(f, sigma) || !rd_d(f, scale) || !rd_d(f, tol_t) || !rd_d(f, tol_r) || !rd_d(f, lambda0) ||
        !rd_i(f, minp) || !rd_i(f, minm) || !rd_i(f, iters) || !rd_i(f, E) || !rd_i(f, Q) || !rd_i(f, N)) return 3;
    const int32_t flags = N == 7 ? rr::kFlagNeighbours7 : N == 27 ? rr::kFlagNeighbours27 : 0;
    if (!rr::params_ok(mn, mx, sigma, scale, tol_t, tol_r, lambda0, (int32_t)iters, 0) || rr::neighbours_of(flags) != (int)N) return 5;
    const rr::Consts k = rr::make_consts(cell, mn, mx, sigma, scale, tol_t, tol_r, lambda0, (int32_t)minp, (int32_t)minm, (int32_t)iters);
    uint32_t log2 = 4;
    while (((int64_t)1 << log2) < 2 * E + 1) log2++;
    const size_t size = (size_t)1 << log2;
    // the table as the map keeps it: key | count | sum[3] | mom[9], each of `size` entries, and the Gaussians beside it
    std::vector<uint64_t> tkey(size, mrule::kEmpty), tcount(size, 0), tsum(3 * size, 0), tmom(srule::kWords * size, 0);
    for (int64_t i = 0; i < E; i++) {
        Entry e;
        if (!rd_entry(f, e)) return 3;
        const uint64_t mask = size - 1;
        uint64_t h = mrule::mix(e.key) & mask;
        while (tkey[(size_t)h] != mrule::kEmpty) h = (h + 1) & mask;
        tkey[(size_t)h] = e.key; tcount[(size_t)h] = (uint64_t)e.n;
        for (int a = 0; a < 3; a++) tsum[a * size + (size_t)h] = e.sum[a];
        for (int j = 0; j < srule::kWords; j++) tmom[j * size + (size_t)h] = e.w[j];
    }
    std::vector<rr::Gauss> gauss(size);
    for (size_t i = 0; i < size; i++) {                                // k_mapreg_gauss
        if (tkey[i] == mrule::kEmpty) { gauss[i].n = 0; continue; }
        uint64_t sum[3], w[srule::kWords];
        for (int a = 0; a < 3; a++) sum[a] = tsum[a * size + i];
        for (int j = 0; j < srule::kWords; j++) w[j] = tmom[j * size + i];
        rr::gauss(k, tkey[i], (int64_t)tcount[i], sum, w, gauss[i]);
    }
    auto find = [&](uint64_t key) -> const rr::Gauss* {
        const int64_t e = probe(tkey, log2, key);
        return e >= 0 ? &gauss[(size_t)e] : nullptr;
    };
    for (int64_t q = 0; q < Q; q++) {
        float start[16]; int64_t n;
        for (int j = 0; j < 16; j++) if (!rd_f(f, start[j])) return 3;
        if (!rd_i(f, n)) return 3;
        std::vector<float> rows(3 * (size_t)n);
        for (size_t j = 0; j < rows.size(); j++) if (!rd_f(f, rows[j])) return 3;
        const int64_t chunks = (n + rr::kChunkRows - 1) / rr::kChunkRows;
        std::vector<rr::Acc> part((size_t)chunks);
        rr::State st; rr::Record rec;
        memset(&st, 0, sizeof(st)); memset(&rec, 0, sizeof(rec));
        for (int pass = 0; pass <= (int)iters; pass++) {
            if (pass > 0 && st.status != rr::kIterationCap) break;     // frozen
            rr::Pose P;
            if (pass == 0) rr::pose_from_float(start, P); else P = st.trial;
            for (int64_t c = 0; c < chunks; c++) {                     // k_mapreg_rows_nb, one partial per chunk (here: the chunk's rows in row order)
                rr::Acc acc; rr::acc_zero(acc);
                const int64_t end = n < (c + 1) * rr::kChunkRows ? n : (c + 1) * rr::kChunkRows;
                for (int64_t i = c * rr::kChunkRows; i < end; i++) {
                    const float x = rows[3 * (size_t)i], y = rows[3 * (size_t)i + 1], z = rows[3 * (size_t)i + 2];
                    if (rr::row_class(k, x, y, z) != mrule::kRowKept) continue;
                    double r[3], w[3]; uint64_t key; rr::Terms tm; int place = -1;
                    const bool in = rr::row_world(k, P, x, y, z, r, w, key);
                    const rr::Gauss* win = in ? select_cell((int)N, key, w, find, place) : nullptr;
                    if (win) rr::match_terms(k, *win, r, w, tm);
                    else rr::miss_terms(k, tm);
                    rr::acc_row(acc, tm, win != nullptr);
                }
                part[(size_t)c] = acc;
            }
            rr::Acc tot; rr::acc_zero(tot);                            // k_mapreg_step: the partials in ascending chunk order
            for (int64_t c = 0; c < chunks; c++) rr::acc_add(tot, part[(size_t)c]);
            rr::step(k, pass, start, tot, st, rec);
        }
        printf("%d %d %d %d %d", rec.status, rec.iterations, rec.accepted, rec.rows_scored, rec.rows_matched);
        for (int j = 0; j < 16; j++) printf(" %08x", to_bits(rec.pose[j]));
        pr_d(rec.cost); pr_d(rec.cost_start); pr_d(rec.lambda);
        for (int j = 0; j < 6; j++) pr_d(rec.g[j]);
        for (int j = 0; j < 21; j++) pr_d(rec.info[j]);
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "flags")) {
        for (int32_t fl = -1; fl < 10; fl++) printf("%d ", rr::neighbours_of(fl));
        printf("\n");
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: test_map_register_neighbours rows|loop FILE, or flags\n"); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    int rc = 2;
    if (!strcmp(argv[1], "rows")) rc = run_rows(f);
    else if (!strcmp(argv[1], "loop")) rc = run_loop(f);
    fclose(f);
    return rc;
}
