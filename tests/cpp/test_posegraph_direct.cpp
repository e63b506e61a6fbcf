// tests/cpp/test_posegraph_direct.cpp -- the pose-graph optimiser with its DIRECT solve on the host: pg_optimise_direct and pg_debug_direct_step of
// icet_amd/csrc/icet_posegraph_driver.h over the bodies of icet_posegraph_body.h and icet_posegraph_direct.h, through a backend that loops where the device
// launches.  Every work array is a heap block of its exact size (pg_bind, pg_bind_direct), so the address sanitizer sees any index the device would take out of
// bounds.  Plain build: a "workgroup" is one thread.  With -DICET_PG_EMU -pthread: four real threads and a barrier; the two must write the same bytes.
// Build: g++ -std=c++17 -I <repo root> (also with -fsanitize=address,undefined).
// Usage: test_posegraph_direct IN OUT.  IN as tests/cpp/test_posegraph_optimize.cpp reads it.  OUT per graph: int32 status, gn_iterations, pcg_iterations, solver |
//     double chi2_initial, chi2_final, max_dx | float poses[n x 16] | double poses64[n x 12] | double edge_chi2[2 x E].  A graph with more end nodes than
//     kPgDirectMaxEnds is an error.  Prints OK.
// Usage: test_posegraph_direct step IN OUT: pg_debug_direct_step.  IN with, behind every graph, int32 K | double p[K x n x 6].  OUT per graph: int32 m,
//     factor_status, wm_status, ks_status, band_solves, trial, 0, 0 | double chi2_start, chi2_trial, max_dx | int32 ends[m] | double D[n x 36], B[n x 36], A[C x 36],
//     g[n x 6], Z[6n x q], Wm, L, Ks, Lk [q x q], x0[n x 6], x[n x 6], Pt[n x 12], chi_trial[E], q[K x n x 6] (NaN where the run wrote nothing).
#include "posegraph_host.h"

int main(int argc, char** argv) {
    const bool step = argc == 4 && strcmp(argv[1], "step") == 0;
    if (argc != 3 && !step) { printf("usage: %s [step] IN OUT\n", argv[0]); return 2; }
    if (step) { argv++; argc--; }
    pg_host_start();
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { printf("cannot open the files\n"); return 2; }
    int32_t count = 0;
    if (fread(&count, 4, 1, in) != 1) return 2;
    for (int gix = 0; gix < count; gix++) {
        HostGraph g;
        if (!g.read(in)) return 2;
        const int n = g.n, C = g.C;
        const size_t N = g.N, Cc = g.Cc, E = g.E, m = g.graph.ends.size(), q = 6 * m;
        if (m > (size_t)kPgDirectMaxEnds) { printf("graph %d has %zu end nodes: above the limit\n", gix, m); return 2; }
        HostBound b(g, true, true);
        HostBackend be;
        if (step) {
            int32_t K = 0;
            std::vector<double> p;
            if (fread(&K, 4, 1, in) != 1 || K < 0 || !rd(in, p, (size_t)K * N * 6)) { printf("short vectors\n"); return 2; }
            // every output at its exact size, NaN where the run writes nothing
            const size_t sizes[14] = {N * 36, N * 36, Cc * 36, N * 6, N * 6 * q, q * q, q * q, q * q, q * q, N * 6, N * 6, N * 12, E, (size_t)K * N * 6};
            std::vector<std::unique_ptr<double[]>> arr;
            for (size_t sz : sizes) arr.push_back(nan_block(sz));
            std::unique_ptr<int32_t[]> ends(new int32_t[m]);
            icet_pose_graph_direct_step so{};
            so.D = arr[0].get(); so.B = arr[1].get(); so.A = arr[2].get(); so.g = arr[3].get(); so.Z = arr[4].get(); so.Wm = arr[5].get(); so.L = arr[6].get(); so.Ks = arr[7].get();
            so.Lk = arr[8].get(); so.x0 = arr[9].get(); so.x = arr[10].get(); so.Pt = arr[11].get(); so.chi_trial = arr[12].get(); so.q = arr[13].get();
            so.ends = ends.get(); so.ends_capacity = (int32_t)m;
            if (!pg_debug_direct_step(be, b.a, b.dir, g.o, K, p.data(), &so)) { printf("the hook failed\n"); return 1; }
            printf("graph %d: n %d C %d, %d end nodes: factor %d, Wm %d, Ks %d, %d band solves, chi2 %.6e -> %.6e, max dx %.3e, %ld launches\n", gix, n, C, so.m, so.factor_status,
                   so.wm_status, so.ks_status, so.band_solves, so.chi2_start, so.chi2_trial, so.max_dx, be.launches);
            const int32_t oh[8] = {so.m, so.factor_status, so.wm_status, so.ks_status, so.band_solves, so.trial, 0, 0};
            const double od[3] = {so.chi2_start, so.chi2_trial, so.max_dx};
            if (!wr(out, oh, 8) || !wr(out, od, 3) || !wr(out, ends.get(), m)) { printf("write failed\n"); return 2; }
            for (int i = 0; i < 14; i++) if (!wr(out, arr[(size_t)i].get(), sizes[i])) { printf("write failed\n"); return 2; }
            continue;
        }
        icet_pose_graph_result res{};
        if (!pg_optimise_direct(be, b.a, b.dir, g.o, &res)) { printf("the driver failed\n"); return 1; }
        printf("graph %d: n %d C %d, %zu end nodes: status %d, %d iterations, %d band solves, chi2 %.6e -> %.6e, max dx %.3e, %ld launches\n", gix, n, C, m,
               res.status, res.gn_iterations, res.pcg_iterations, res.chi2_initial, res.chi2_final, res.max_dx, be.launches);
        const int32_t oh[4] = {res.status, res.gn_iterations, res.pcg_iterations, res.solver};
        const double od[3] = {res.chi2_initial, res.chi2_final, res.max_dx};
        if (!wr(out, oh, 4) || !wr(out, od, 3) || !wr(out, b.poses_out.get(), N * 16) || !wr(out, b.poses64.get(), N * 12) || !wr(out, b.edge_chi2.get(), 2 * E)) { printf("write failed\n"); return 2; }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("OK\n");
    return 0;
}
