// tests/cpp/test_posegraph_optimize.cpp -- the WHOLE pose-graph optimiser on the host: the driver of icet_amd/csrc/icet_posegraph_driver.h over the bodies of
// icet_posegraph_body.h, through a backend that loops where the device launches.  Every work array is a heap block of its exact size, so the address sanitizer sees
// any index the device would take out of bounds.  Plain build: a "workgroup" is one thread.  With -DICET_PG_EMU -pthread: four real threads and a barrier; the two
// must write the same bytes.  Build: g++ -std=c++17 -I <repo root> (also with -fsanitize=address,undefined).
// Usage: test_posegraph_optimize IN OUT.  IN: int32 count, then per graph
//     int32 n, C, gn_iters, max_pcg | double dx_tol, damping, pcg_tol | float poses[n x 16], odo_X[(n-1) x 6], odo_info[(n-1) x 36] | int32 ci[C], cj[C] |
//     float clo_X[C x 6], clo_info[C x 36] | uint8 fixed[n]
// OUT per graph: int32 status, gn_iterations, pcg_iterations, 0 | double chi2_initial, chi2_final, max_dx | float poses[n x 16] | double poses64[n x 12] |
//     double edge_chi2[2 x E].  Prints OK.
// Usage: test_posegraph_optimize step IN OUT: pg_debug_step, the test hook's run (include/icet_hip.h icet_debug_pose_graph_step), on the same backend.  IN as
// above with, behind every graph, int32 K | double p[K x n x 6] (gn_iters and dx_tol are not used).  OUT per graph: int32 factor_status, cg_status, band_solves,
//     cg_end, cap, c_offband, trial, 0 | double chi2_start, chi2_trial, max_dx | double J[E x 72], res[E x 6], chi_start[E], chi_trial[E], D[n x 36], B[n x 36],
//     A[C x 36], g[n x 6], x[n x 6], Pt[n x 12], q[K x n x 6], cg_scalars[cap x 2] (NaN behind band_solves rows).
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
    static void group_body(PgGroupKernel k, const PgArgs& a) {
        static PgShared sh;
        static PgRed red;
        switch (k) {
            case kPgFactor: pg_group_factor(a, sh); break;
            case kPgPrecond: pg_group_precond(a, sh, red); break;
            case kPgStep: pg_group_step(a, red); break;
            case kPgStats: pg_group_stats(a, red); break;
        }
    }
    bool group(PgGroupKernel k, const PgArgs& a) {
        launches++;
#if defined(ICET_PG_EMU)
        std::vector<std::thread> th;
        for (int t = 0; t < kPgThreads; t++) th.emplace_back([k, &a, t]() { pg_emu_tid = t; group_body(k, a); });
        for (auto& t : th) t.join();
#else
        group_body(k, a);
#endif
        return true;
    }
    bool scalars(const PgArgs& a, double out[kPgScalars]) { for (int i = 0; i < kPgScalars; i++) out[i] = a.sc[i]; return true; }
    bool fetch(void* host, const void* dev, size_t bytes) { memcpy(host, dev, bytes); return true; }
    bool put(void* dev, const void* host, size_t bytes) { memcpy(dev, host, bytes); return true; }
};

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static bool wr(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    const bool step = argc == 4 && strcmp(argv[1], "step") == 0;
    if (argc != 3 && !step) { printf("usage: %s [step] IN OUT\n", argv[0]); return 2; }
    if (step) { argv++; argc--; }
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
        icet_pose_graph_options o = pg_default_options();
        o.gn_iters = hd[2]; o.max_pcg = hd[3]; o.dx_tol = tol[0]; o.damping = tol[1]; o.pcg_tol = tol[2];
        PgGraph graph;
        graph.build(n, C, ci.data(), cj.data(), fixed.data());
        PgArgs a{};
        a.N = n; a.C = C; a.E = (int)E;
        HostAlloc al;
        const PgGraphDev gd = pg_bind(a, al, graph.items.size());
        if (E) { memcpy(gd.ei, graph.ei.data(), 4 * E); memcpy(gd.ej, graph.ej.data(), 4 * E); }
        memcpy(gd.off, graph.off.data(), 4 * (N + 1));
        if (!graph.items.empty()) memcpy(gd.items, graph.items.data(), 4 * graph.items.size());
        // the caller's arrays and the outputs at their exact sizes too
        std::unique_ptr<float[]> h_poses(new float[N * 16]), h_oX(new float[(N - 1) * 6]), h_oI(new float[(N - 1) * 36]), h_cX(new float[Cc * 6]), h_cI(new float[Cc * 36]),
            h_out(new float[N * 16]);
        std::unique_ptr<double[]> h_p64(new double[N * 12]), h_chi(new double[2 * E]);
        memcpy(h_poses.get(), poses.data(), 4 * N * 16);
        if (N > 1) { memcpy(h_oX.get(), odo_X.data(), 4 * (N - 1) * 6); memcpy(h_oI.get(), odo_info.data(), 4 * (N - 1) * 36); }
        if (Cc) { memcpy(h_cX.get(), clo_X.data(), 4 * Cc * 6); memcpy(h_cI.get(), clo_info.data(), 4 * Cc * 36); }
        a.poses_in = h_poses.get(); a.odo_X = h_oX.get(); a.odo_info = h_oI.get(); a.clo_X = h_cX.get(); a.clo_info = h_cI.get();
        a.poses_out = h_out.get(); a.poses64_out = h_p64.get(); a.edge_chi2_out = h_chi.get();
        HostBackend be;
        if (step) {
            int32_t K = 0;
            std::vector<double> p;
            if (fread(&K, 4, 1, in) != 1 || K < 0 || !rd(in, p, (size_t)K * N * 6)) { printf("short vectors\n"); return 2; }
            // every output at its exact size, NaN where the run writes nothing
            const int cap = pg_cg_cap(graph.c_offband, o);
            const size_t sizes[12] = {E * 72, E * 6, E, E, N * 36, N * 36, Cc * 36, N * 6, N * 6, N * 12, (size_t)K * N * 6, (size_t)cap * 2};
            std::vector<std::unique_ptr<double[]>> arr;
            for (size_t sz : sizes) { arr.emplace_back(new double[sz]); for (size_t i = 0; i < sz; i++) arr.back()[i] = std::nan(""); }
            icet_pose_graph_step so{};
            so.J = arr[0].get(); so.res = arr[1].get(); so.chi_start = arr[2].get(); so.chi_trial = arr[3].get(); so.D = arr[4].get(); so.B = arr[5].get(); so.A = arr[6].get();
            so.g = arr[7].get(); so.x = arr[8].get(); so.Pt = arr[9].get(); so.q = arr[10].get(); so.cg_scalars = arr[11].get(); so.cg_capacity = cap;
            if (!pg_debug_step(be, a, o, graph.c_offband, K, p.data(), &so)) { printf("the hook failed\n"); return 1; }
            printf("graph %d: n %d C %d (%d off the band): factor %d, cg %d, %d band solves of %d, end %d, chi2 %.6e -> %.6e, max dx %.3e\n", gix, n, C, so.c_offband,
                   so.factor_status, so.cg_status, so.band_solves, so.cap, so.cg_end, so.chi2_start, so.chi2_trial, so.max_dx);
            const int32_t oh[8] = {so.factor_status, so.cg_status, so.band_solves, so.cg_end, so.cap, so.c_offband, so.trial, 0};
            const double od[3] = {so.chi2_start, so.chi2_trial, so.max_dx};
            if (!wr(out, oh, 8) || !wr(out, od, 3)) { printf("write failed\n"); return 2; }
            for (int i = 0; i < 12; i++) if (!wr(out, arr[(size_t)i].get(), sizes[i])) { printf("write failed\n"); return 2; }
            continue;
        }
        icet_pose_graph_result res{};
        if (!pg_optimise(be, a, o, graph.c_offband, &res)) { printf("the driver failed\n"); return 1; }
        printf("graph %d: n %d C %d (%d off the band) status %d, %d iterations, %d band solves, chi2 %.6e -> %.6e, max dx %.3e, %ld launches\n", gix, n, C, graph.c_offband,
               res.status, res.gn_iterations, res.pcg_iterations, res.chi2_initial, res.chi2_final, res.max_dx, be.launches);
        const int32_t oh[4] = {res.status, res.gn_iterations, res.pcg_iterations, 0};
        const double od[3] = {res.chi2_initial, res.chi2_final, res.max_dx};
        if (!wr(out, oh, 4) || !wr(out, od, 3) || !wr(out, h_out.get(), N * 16) || !wr(out, h_p64.get(), N * 12) || !wr(out, h_chi.get(), 2 * E)) { printf("write failed\n"); return 2; }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("OK\n");
    return 0;
}
