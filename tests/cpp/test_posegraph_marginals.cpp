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
#include "posegraph_host.h"

int main(int argc, char** argv) {
    const bool blocks = argc == 4 && strcmp(argv[1], "blocks") == 0;
    if (argc != 3 && !blocks) { printf("usage: %s [blocks] IN OUT\n", argv[0]); return 2; }
    if (blocks) { argv++; argc--; }
    pg_host_start();
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { printf("cannot open the files\n"); return 2; }
    int32_t count = 0;
    if (fread(&count, 4, 1, in) != 1) return 2;
    for (int gix = 0; gix < count; gix++) {
        HostGraph g;
        if (!g.read(in)) return 2;
        const int n = g.n, C = g.C;
        const size_t N = g.N, Cc = g.Cc, m = g.graph.ends.size();
        if (m > (size_t)kPgDirectMaxEnds) { printf("graph %d has %zu end nodes: above the limit\n", gix, m); return 2; }
        HostBound b(g, true, false);
        PgArgs& a = b.a;
        PgMarg mg{};
        pg_bind_marg(a, b.dir, mg, b.al, true);
        for (size_t i = 0; i < N * 36; i++) { mg.cov[i] = std::nan(""); mg.band_cov[i] = std::nan(""); }
        // the hook's outputs at their exact sizes, NaN where the run writes nothing
        const size_t sizes[4] = {N * 36, N * 36, Cc * 36, N * 36};
        std::vector<std::unique_ptr<double[]>> arr;
        for (size_t sz : sizes) arr.push_back(nan_block(sz));
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
        if (!pg_marginals(be, a, b.dir, mg, &res, &tap, blocks)) { printf("the driver failed\n"); return 1; }
        printf("graph %d: n %d C %d, %d end nodes: status %d (factor %d, Wm %d, Ks %d), %ld launches\n", gix, n, C, res.m, res.status, res.factor_status, res.wm_status,
               res.ks_status, be.launches);
        const int32_t oh[6] = {res.status, res.m, res.factor_status, res.wm_status, res.ks_status, res.reserved};
        if (!wr(out, oh, 6) || !wr(out, g.graph.ends.data(), m)) { printf("write failed\n"); return 2; }
        for (int i = 0; i < 4; i++) if (!wr(out, arr[(size_t)i].get(), sizes[i])) { printf("write failed\n"); return 2; }
        if (!wr(out, mg.cov, N * 36)) { printf("write failed\n"); return 2; }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("OK\n");
    return 0;
}
