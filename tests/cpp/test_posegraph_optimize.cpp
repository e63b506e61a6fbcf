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
        const int n = g.n, C = g.C, c_offband = g.graph.c_offband;
        const size_t N = g.N, Cc = g.Cc, E = g.E;
        HostBound b(g, false, true);
        HostBackend be;
        if (step) {
            int32_t K = 0;
            std::vector<double> p;
            if (fread(&K, 4, 1, in) != 1 || K < 0 || !rd(in, p, (size_t)K * N * 6)) { printf("short vectors\n"); return 2; }
            // every output at its exact size, NaN where the run writes nothing
            const int cap = pg_cg_cap(c_offband, g.o);
            const size_t sizes[12] = {E * 72, E * 6, E, E, N * 36, N * 36, Cc * 36, N * 6, N * 6, N * 12, (size_t)K * N * 6, (size_t)cap * 2};
            std::vector<std::unique_ptr<double[]>> arr;
            for (size_t sz : sizes) arr.push_back(nan_block(sz));
            icet_pose_graph_step so{};
            so.J = arr[0].get(); so.res = arr[1].get(); so.chi_start = arr[2].get(); so.chi_trial = arr[3].get(); so.D = arr[4].get(); so.B = arr[5].get(); so.A = arr[6].get();
            so.g = arr[7].get(); so.x = arr[8].get(); so.Pt = arr[9].get(); so.q = arr[10].get(); so.cg_scalars = arr[11].get(); so.cg_capacity = cap;
            if (!pg_debug_step(be, b.a, g.o, c_offband, K, p.data(), &so)) { printf("the hook failed\n"); return 1; }
            printf("graph %d: n %d C %d (%d off the band): factor %d, cg %d, %d band solves of %d, end %d, chi2 %.6e -> %.6e, max dx %.3e\n", gix, n, C, so.c_offband,
                   so.factor_status, so.cg_status, so.band_solves, so.cap, so.cg_end, so.chi2_start, so.chi2_trial, so.max_dx);
            const int32_t oh[8] = {so.factor_status, so.cg_status, so.band_solves, so.cg_end, so.cap, so.c_offband, so.trial, 0};
            const double od[3] = {so.chi2_start, so.chi2_trial, so.max_dx};
            if (!wr(out, oh, 8) || !wr(out, od, 3)) { printf("write failed\n"); return 2; }
            for (int i = 0; i < 12; i++) if (!wr(out, arr[(size_t)i].get(), sizes[i])) { printf("write failed\n"); return 2; }
            continue;
        }
        icet_pose_graph_result res{};
        if (!pg_optimise(be, b.a, g.o, c_offband, &res)) { printf("the driver failed\n"); return 1; }
        printf("graph %d: n %d C %d (%d off the band) status %d, %d iterations, %d band solves, chi2 %.6e -> %.6e, max dx %.3e, %ld launches\n", gix, n, C, c_offband,
               res.status, res.gn_iterations, res.pcg_iterations, res.chi2_initial, res.chi2_final, res.max_dx, be.launches);
        const int32_t oh[4] = {res.status, res.gn_iterations, res.pcg_iterations, 0};
        const double od[3] = {res.chi2_initial, res.chi2_final, res.max_dx};
        if (!wr(out, oh, 4) || !wr(out, od, 3) || !wr(out, b.poses_out.get(), N * 16) || !wr(out, b.poses64.get(), N * 12) || !wr(out, b.edge_chi2.get(), 2 * E)) { printf("write failed\n"); return 2; }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("OK\n");
    return 0;
}
