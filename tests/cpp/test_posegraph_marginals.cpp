// tests/cpp/test_posegraph_marginals.cpp -- the pose graph's MARGINAL COVARIANCES on the host: pg_marginals of icet_amd/csrc/icet_posegraph_driver.h over the
// bodies of icet_posegraph_body.h, icet_posegraph_direct.h and icet_posegraph_marginals.h, through a backend that loops where the device launches.  Every work
// array is a heap block of its exact size (pg_bind, pg_bind_direct, pg_bind_marg), so the address sanitizer sees any index the device would take out of bounds.
// Plain build: a "workgroup" is one thread.  With -DICET_PG_EMU -pthread: four real threads and a barrier; the two must write the same bytes.
// Build: g++ -std=c++17 -ffp-contract=off -I <repo root> (also with -fsanitize=address,undefined).
// Usage: test_posegraph_marginals IN OUT.  IN as tests/cpp/test_posegraph_optimize.cpp reads it (the options are not used).  OUT per graph: int32 status, m,
//     factor_status, wm_status, ks_status, 0 | int32 ends[m] | double D[n x 36], B[n x 36], A[C x 36], band_cov[n x 36], cov[n x 36] (NaN where the run wrote
//     nothing).  A graph with more end nodes than kPgDirectMaxEnds is an error.  Prints OK.
// Usage: test_posegraph_marginals blocks IN OUT.  IN with, behind every graph, double D[n x 36], B[n x 36], A[C x 36]: the run starts at the band's factor on
//     these blocks (a device's own, so that the two results differ by the marginals' arithmetic alone and not by the Jacobians').  OUT as above.
#if defined(ICET_PG_EMU)
#include <pthread.h>
static thread_local int pg_emu_tid = 0;
static pthread_barrier_t pg_emu_barrier;
#define ICET_PG_EMU_THREADS 4
#define ICET_PG_DEV static inline
#define ICET_PG_TID pg_emu_tid
#define ICET_PG_SYNC() pthread_barrier_wait(&pg_emu_barrier)
#define ICET_PG_UNROLL
#endif
#include "icet_amd/csrc/icet_posegraph_driver.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#if defined(ICET_PG_EMU)
#include <thread>
#endif

using namespace icet;

struct HostAlloc {
    std::vector<std::unique_ptr<double[]>> dd;
    std::vector<std::unique_ptr<int32_t[]>> ii;
    double* d(size_t n) { dd.emplace_back(new double[n]); return dd.back().get(); }
    int32_t* i(size_t n) { ii.emplace_back(new int32_t[n]); return ii.back().get(); }
};

struct HostBackend {
    long launches = 0;
    bool grid(PgGridKernel k, int count, const PgArgs& a) {
        launches++;
        for (int gi = 0; gi < count; gi++)
            switch (k) {
                case kPgInit: pg_init(a, gi); break;
                case kPgChi: pg_chi(a, gi); break;
                case kPgLinearise: pg_linearise(a, gi); break;
                case kPgAssemble: pg_assemble(a, gi); break;
                case kPgOffband: pg_offband(a, gi); break;
                case kPgHp: pg_hp(a, gi); break;
                case kPgRetract: pg_retract(a, gi); break;
                case kPgFinish: pg_finish(a, gi); break;
            }
        return true;
    }
    bool dgrid(PgDirectGridKernel k, int count, const PgArgs& a, const PgDirect& d) {
        launches++;
        for (int gi = 0; gi < count; gi++)
            switch (k) {
                case kPgZ: pg_z(a, d, gi); break;
                case kPgWm: pg_wm(a, d, gi); break;
                case kPgSl: pg_sl(a, d, gi); break;
                case kPgKs: pg_ks(a, d, gi); break;
                case kPgZw: pg_zw(a, d, gi); break;
                case kPgResid: pg_resid(a, d, gi); break;
            }
        return true;
    }
    bool mgrid(PgMargGridKernel k, int count, const PgArgs& a, const PgDirect& d, const PgMarg& mg) {
        launches++;
        for (int gi = 0; gi < count; gi++)
            switch (k) {
                case kPgSelinvPrep: pg_selinv_prep(a, mg, gi); break;
                case kPgMargLt: pg_marg_lt(a, d, mg, gi); break;
            }
        return true;
    }
    template <class Body> static void workgroup(Body body) {
#if defined(ICET_PG_EMU)
        std::vector<std::thread> th;
        for (int t = 0; t < kPgThreads; t++) th.emplace_back([&body, t]() { pg_emu_tid = t; body(); });
        for (auto& t : th) t.join();
#else
        body();
#endif
    }
    bool group(PgGroupKernel k, const PgArgs& a) {
        launches++;
        static PgShared sh;
        static PgRed red;
        workgroup([&]() {
            switch (k) {
                case kPgFactor: pg_group_factor(a, sh); break;
                case kPgPrecond: pg_group_precond(a, sh, red); break;
                case kPgStep: pg_group_step(a, red); break;
                case kPgStats: pg_group_stats(a, red); break;
            }
        });
        return true;
    }
    bool dgroup(PgDirectGroupKernel k, const PgArgs& a, const PgDirect& d) {
        launches++;
        static PgShared sh;
        workgroup([&]() {
            switch (k) {
                case kPgCholW: pg_group_chol(a, d, 0); break;
                case kPgCholK: pg_group_chol(a, d, 1); break;
                case kPgBand: pg_group_band(a, d, sh); break;
                case kPgCapSolve: pg_group_cap_solve(a, d); break;
            }
        });
        return true;
    }
    // the group body once per group index: the device runs them as the workgroups of one launch, here one behind the other
    bool mgroups(PgMargGroupKernel k, int groups, const PgArgs& a, const PgDirect& d, const PgMarg& mg) {
        launches++;
        static PgShared sh;
        static PgMargShared msh;
        for (int g = 0; g < groups; g++)
            workgroup([&]() {
                switch (k) {
                    case kPgSelinv: pg_group_selinv(a, mg, sh); break;
                    case kPgMargNode: pg_group_marg(a, d, mg, g, msh); break;
                }
            });
        return true;
    }
    bool scalars(const PgArgs& a, double out[kPgScalars]) { for (int i = 0; i < kPgScalars; i++) out[i] = a.sc[i]; return true; }
    bool fetch(void* host, const void* dev, size_t bytes) { memcpy(host, dev, bytes); return true; }
    bool put(void* dev, const void* host, size_t bytes) { memcpy(dev, host, bytes); return true; }
};

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static bool wr(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    const bool blocks = argc == 4 && strcmp(argv[1], "blocks") == 0;
    if (argc != 3 && !blocks) { printf("usage: %s [blocks] IN OUT\n", argv[0]); return 2; }
    if (blocks) { argv++; argc--; }
#if defined(ICET_PG_EMU)
    pthread_barrier_init(&pg_emu_barrier, nullptr, ICET_PG_EMU_THREADS);
#endif
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { printf("cannot open the files\n"); return 2; }
    int32_t count = 0;
    if (fread(&count, 4, 1, in) != 1) return 2;
    for (int gix = 0; gix < count; gix++) {
        int32_t hd[4]; double tol[3];
        if (fread(hd, 4, 4, in) != 4 || fread(tol, 8, 3, in) != 3) { printf("short header\n"); return 2; }
        const int n = hd[0], C = hd[1];
        const size_t N = (size_t)n, Cc = (size_t)C, E = (size_t)pg::edge_count(n, C);
        std::vector<float> poses, odo_X, odo_info, clo_X, clo_info;
        std::vector<int32_t> ci, cj;
        std::vector<uint8_t> fixed;
        if (!rd(in, poses, N * 16) || !rd(in, odo_X, (N - 1) * 6) || !rd(in, odo_info, (N - 1) * 36) || !rd(in, ci, Cc) || !rd(in, cj, Cc) || !rd(in, clo_X, Cc * 6) ||
            !rd(in, clo_info, Cc * 36) || !rd(in, fixed, N)) { printf("short graph\n"); return 2; }
        if (!pg::closures_ok(n, C, ci.data(), cj.data())) { printf("bad closures\n"); return 2; }
        PgGraph graph;
        graph.build(n, C, ci.data(), cj.data(), fixed.data());
        const size_t m = graph.ends.size();
        if (m > (size_t)kPgDirectMaxEnds) { printf("graph %d has %zu end nodes: above the limit\n", gix, m); return 2; }
        PgArgs a{};
        PgDirect dir{};
        PgMarg mg{};
        a.N = n; a.C = C; a.E = (int)E;
        HostAlloc al;
        const PgGraphDev gd = pg_bind(a, al, graph.items.size());
        const PgDirectDev dd = pg_bind_direct(a, dir, al, m);
        pg_bind_marg(a, dir, mg, al, true);
        for (size_t i = 0; i < N * 36; i++) { mg.cov[i] = std::nan(""); mg.band_cov[i] = std::nan(""); }
        if (E) { memcpy(gd.ei, graph.ei.data(), 4 * E); memcpy(gd.ej, graph.ej.data(), 4 * E); }
        memcpy(gd.off, graph.off.data(), 4 * (N + 1));
        if (!graph.items.empty()) memcpy(gd.items, graph.items.data(), 4 * graph.items.size());
        if (m) memcpy(dd.ends, graph.ends.data(), 4 * m);
        memcpy(dd.end_of, graph.end_of.data(), 4 * N);
        // the caller's arrays at their exact sizes too
        std::unique_ptr<float[]> h_poses(new float[N * 16]), h_oX(new float[(N - 1) * 6]), h_oI(new float[(N - 1) * 36]), h_cX(new float[Cc * 6]), h_cI(new float[Cc * 36]);
        memcpy(h_poses.get(), poses.data(), 4 * N * 16);
        if (N > 1) { memcpy(h_oX.get(), odo_X.data(), 4 * (N - 1) * 6); memcpy(h_oI.get(), odo_info.data(), 4 * (N - 1) * 36); }
        if (Cc) { memcpy(h_cX.get(), clo_X.data(), 4 * Cc * 6); memcpy(h_cI.get(), clo_info.data(), 4 * Cc * 36); }
        a.poses_in = h_poses.get(); a.odo_X = h_oX.get(); a.odo_info = h_oI.get(); a.clo_X = h_cX.get(); a.clo_info = h_cI.get();
        a.poses_out = nullptr; a.poses64_out = nullptr; a.edge_chi2_out = nullptr;          // (kPgFinish does not run)
        // the hook's outputs at their exact sizes, NaN where the run writes nothing
        const size_t sizes[4] = {N * 36, N * 36, Cc * 36, N * 36};
        std::vector<std::unique_ptr<double[]>> arr;
        for (size_t sz : sizes) { arr.emplace_back(new double[sz]); for (size_t i = 0; i < sz; i++) arr.back()[i] = std::nan(""); }
        PgMargTap tap;
        tap.D = arr[0].get(); tap.B = arr[1].get(); tap.A = arr[2].get(); tap.band_cov = arr[3].get();
        HostBackend be;
        icet_pose_graph_marginals_result res{};
        if (blocks) {
            std::vector<double> bD, bB, bA;
            if (!rd(in, bD, N * 36) || !rd(in, bB, N * 36) || !rd(in, bA, Cc * 36)) { printf("short blocks\n"); return 2; }
            memcpy(a.D, bD.data(), 8 * N * 36); memcpy(a.B, bB.data(), 8 * N * 36);
            if (Cc) memcpy(a.A, bA.data(), 8 * Cc * 36);
            for (size_t i = 0; i < N * 6; i++) a.g[i] = 0.0;
            for (int i = 0; i < kPgScalars; i++) a.sc[i] = 0.0;
        }
        if (!pg_marginals(be, a, dir, mg, &res, &tap, blocks)) { printf("the driver failed\n"); return 1; }
        printf("graph %d: n %d C %d, %d end nodes: status %d (factor %d, Wm %d, Ks %d), %ld launches\n", gix, n, C, res.m, res.status, res.factor_status, res.wm_status,
               res.ks_status, be.launches);
        const int32_t oh[6] = {res.status, res.m, res.factor_status, res.wm_status, res.ks_status, res.reserved};
        if (!wr(out, oh, 6) || !wr(out, graph.ends.data(), m)) { printf("write failed\n"); return 2; }
        for (int i = 0; i < 4; i++) if (!wr(out, arr[(size_t)i].get(), sizes[i])) { printf("write failed\n"); return 2; }
        if (!wr(out, mg.cov, N * 36)) { printf("write failed\n"); return 2; }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("OK\n");
    return 0;
}
