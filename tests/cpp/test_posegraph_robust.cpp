// tests/cpp/test_posegraph_robust.cpp -- the pose-graph optimiser under a ROBUST KERNEL on the host: pg_optimise_robust of icet_amd/csrc/icet_posegraph_driver.h
// over the bodies of icet_posegraph_robust.h and icet_posegraph_body.h, through the backend of posegraph_robust_host.h.  Every array is a heap block of its
// exact size.  Plain build: a "workgroup" is one thread; with -DICET_PG_EMU -pthread four real threads and a barrier; the two must write the same bytes.
// Build: g++ -std=c++17 -I <repo root> (also with -fsanitize=address,undefined).
// Usage: test_posegraph_robust IN OUT.  IN: int32 count, then per run the graph record of test_posegraph_optimize.cpp and int32 kind, flags, direct, 0 |
// double scale.  OUT per run: int32 status, gn_iterations, pcg_iterations, solver, downweighted, 0 | double chi2_initial, chi2_final, max_dx, cost_initial,
// cost_final | float poses[n x 16] | double poses64[n x 12], edge_chi2[2 x E], edge_weight[E].
// A run with kind 0 is also made through pg_optimise / pg_optimise_direct on a backend WITHOUT the robust bodies: the two must write the same bytes.
// Before the runs: the checks of a caller's struct that need no graph (pg_robust_args) and the sizes of the two structs.  Prints OK.
#include "posegraph_robust_host.h"

static bool same(const void* a, const void* b, size_t bytes) { return bytes == 0 || memcmp(a, b, bytes) == 0; }

static bool argument_checks() {
    static_assert(sizeof(icet_pose_graph_robust) == 16 && sizeof(icet_pose_graph_robust_result) == 64, "the robust structs' sizes");
    static_assert(sizeof(icet_pose_graph_options) == 32 && sizeof(icet_pose_graph_result) == 40, "the optimiser's structs' sizes");
    PgRobust r;
    const double inf = HUGE_VAL, nan = std::nan("");
    const icet_pose_graph_robust good[] = {{0, 0, 0.0}, {0, 1, nan}, {1, 0, 16.8119}, {2, 1, 1e-300}, {3, 0, 1e300}};
    const icet_pose_graph_robust bad[] = {{-1, 0, 1.0}, {4, 0, 1.0}, {1, 2, 1.0}, {0, 2, 1.0}, {2, -1, 1.0}, {1, 0, 0.0}, {2, 0, -1.0}, {3, 0, inf}, {1, 0, nan}, {3, 1, -inf}};
    if (!pg_robust_args(nullptr, &r) || r.kind != 0) return false;
    for (const auto& g : good) if (!pg_robust_args(&g, &r) || r.kind != g.kind || r.flags != g.flags) return false;
    for (const auto& b : bad) if (pg_robust_args(&b, &r)) return false;
    return ICET_PG_ROBUST_DEFAULT_SCALE == pg::kRobustDefaultScale && ICET_PG_ROBUST_ODOMETRY == pg::kRobustOdometry && ICET_PG_ROBUST_GEMAN_MCCLURE == pg::kRobustGemanMcClure;
}

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: %s IN OUT\n", argv[0]); return 2; }
    if (!argument_checks()) { printf("the argument checks failed\n"); return 1; }
    pg_host_start();
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { printf("cannot open the files\n"); return 2; }
    int32_t count = 0, kind0 = 0;
    if (fread(&count, 4, 1, in) != 1) return 2;
    for (int gix = 0; gix < count; gix++) {
        HostGraph g;
        if (!g.read(in)) return 2;
        int32_t hd[4]; double scale = 0.0;
        if (fread(hd, 4, 4, in) != 4 || fread(&scale, 8, 1, in) != 1) { printf("short run\n"); return 2; }
        const icet_pose_graph_robust rob{hd[0], hd[1], scale};
        const bool direct = hd[2] != 0;
        const size_t N = g.N, E = g.E;
        RobustHostBound b(g, direct, &rob);
        if (!b.ok) { printf("run %d: bad robust arguments\n", gix); return 2; }
        RobustHostBackend be;
        icet_pose_graph_robust_result res{};
        if (!pg_optimise_robust(be, b.a, b.dir, direct, g.o, g.graph.c_offband, b.rb, &res)) { printf("the driver failed\n"); return 1; }
        printf("run %d: n %d C %d kind %d flags %d %s: status %d, %d iterations, %d band solves, chi2 %.6e -> %.6e, F %.6e -> %.6e, %d downweighted, %ld launches\n", gix, g.n, g.C,
               rob.kind, rob.flags, direct ? "direct" : "cg", res.base.status, res.base.gn_iterations, res.base.pcg_iterations, res.base.chi2_initial, res.base.chi2_final,
               res.cost_initial, res.cost_final, res.downweighted, be.launches);
        if (rob.kind == 0) {
            // the plain driver on a backend that has no robust bodies
            HostBound pb(g, direct, true);
            HostBackend pbe;
            icet_pose_graph_result pres{};
            if (!(direct ? pg_optimise_direct(pbe, pb.a, pb.dir, g.o, &pres) : pg_optimise(pbe, pb.a, g.o, g.graph.c_offband, &pres))) { printf("the plain driver failed\n"); return 1; }
            bool ok = same(&pres, &res.base, sizeof(pres)) && same(&res.cost_initial, &pres.chi2_initial, 8) && same(&res.cost_final, &pres.chi2_final, 8) && res.downweighted == 0;
            ok = ok && same(pb.poses_out.get(), b.poses_out.get(), 4 * N * 16) && same(pb.poses64.get(), b.poses64.get(), 8 * N * 12) && same(pb.edge_chi2.get(), b.edge_chi2.get(), 16 * E);
            for (size_t e = 0; e < E; e++) ok = ok && b.edge_weight[e] == 1.0;
            ok = ok && be.launches == pbe.launches + 1;          // (the robust run's only launch of its own: kPgRobustFinish)
            if (!ok) { printf("run %d: kind 0 differs from the plain driver\n", gix); return 1; }
            kind0++;
        }
        const int32_t oh[6] = {res.base.status, res.base.gn_iterations, res.base.pcg_iterations, res.base.solver, res.downweighted, 0};
        const double od[5] = {res.base.chi2_initial, res.base.chi2_final, res.base.max_dx, res.cost_initial, res.cost_final};
        if (!wr(out, oh, 6) || !wr(out, od, 5) || !wr(out, b.poses_out.get(), N * 16) || !wr(out, b.poses64.get(), N * 12) || !wr(out, b.edge_chi2.get(), 2 * E) ||
            !wr(out, b.edge_weight.get(), E)) { printf("write failed\n"); return 2; }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("kind 0 as the plain driver: %d runs\nOK\n", kind0);
    return 0;
}
