// tests/cpp/test_posegraph_cross.cpp -- the pose graph's COVARIANCE COLUMNS and GATE on the host: pg_columns and pg_gate of
// icet_amd/csrc/icet_posegraph_driver.h over the bodies of icet_posegraph_body.h, icet_posegraph_direct.h, icet_posegraph_marginals.h and
// icet_posegraph_cross.h, through a backend that loops where the device launches.  Every work array is a heap block of its exact size (pg_bind, pg_bind_direct,
// pg_bind_marg, pg_bind_cross, pg_bind_gate), so the address sanitizer sees any index the device would take out of bounds.
// Plain build: a "workgroup" is one thread.  With -DICET_PG_EMU -pthread: four real threads and a barrier; the two must write the same bytes.
// Build: g++ -std=c++17 -ffp-contract=off -I <repo root> (also with -fsanitize=address,undefined).
// Usage: test_posegraph_cross [blocks] IN OUT.  IN: int32 count, then per graph the record tests/cpp/test_posegraph_optimize.cpp reads (the options are not
//     used) | int32 T, targets[T] | int32 n_cand, gi[n_cand], gj[n_cand], float X[n_cand x 6], cov[n_cand x 36], double threshold | with `blocks` double
//     D[n x 36], B[n x 36], A[C x 36]: the columns run starts at the band's factor on these blocks (a device's own).
// OUT per graph: int32 status, m, factor_status, wm_status, ks_status, 0 | int32 ends[m] | double D[n x 36], B[n x 36], A[C x 36], band_cov[n x 36], cov[n x 36],
//     cols[T x n x 36] (NaN where the run wrote nothing) | with n_cand > 0, from a gate run of its own: int32 status, n_targets, rejected | double d2[n_cand],
//     S[n_cand x 36] | int32 cand_status[n_cand].  Prints OK.
#include "posegraph_cross_host.h"

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
        int32_t T = 0, n_cand = 0;
        std::vector<int32_t> targets, gi, gj;
        std::vector<float> cX, ccov;
        double threshold = 0.0;
        if (fread(&T, 4, 1, in) != 1 || T < 1 || T > kPgCrossMaxTargets || !rd(in, targets, (size_t)T)) { printf("bad targets\n"); return 2; }
        for (int32_t t : targets) if (t < 0 || t >= n) { printf("a target is out of range\n"); return 2; }
        if (fread(&n_cand, 4, 1, in) != 1 || n_cand < 0 || n_cand > kPgGateMaxCand || !rd(in, gi, (size_t)n_cand) || !rd(in, gj, (size_t)n_cand) ||
            !rd(in, cX, (size_t)n_cand * 6) || !rd(in, ccov, (size_t)n_cand * 36) || fread(&threshold, 8, 1, in) != 1) { printf("bad candidates\n"); return 2; }
        // ---- the columns ----
        {
            HostBound b(g, true, false);
            PgArgs& a = b.a;
            PgMarg mg{};
            PgCross x{};
            pg_bind_marg(a, b.dir, mg, b.al, true);
            const PgCrossDev xd = pg_bind_cross(a, b.dir, x, b.al, T, true);
            memcpy(xd.targets, targets.data(), 4 * (size_t)T);
            for (size_t i = 0; i < N * 36; i++) { mg.cov[i] = std::nan(""); mg.band_cov[i] = std::nan(""); }
            for (size_t i = 0; i < (size_t)T * N * 36; i++) x.cols[i] = std::nan("");
            const size_t sizes[4] = {N * 36, N * 36, Cc * 36, N * 36};
            std::vector<std::unique_ptr<double[]>> arr;
            for (size_t sz : sizes) arr.push_back(nan_block(sz));
            PgMargTap tap;
            tap.D = arr[0].get(); tap.B = arr[1].get(); tap.A = arr[2].get(); tap.band_cov = arr[3].get();
            CrossHostBackend be;
            icet_pose_graph_marginals_result res{};
            if (blocks) {
                std::vector<double> bD, bB, bA;
                if (!rd(in, bD, N * 36) || !rd(in, bB, N * 36) || !rd(in, bA, Cc * 36)) { printf("short blocks\n"); return 2; }
                memcpy(a.D, bD.data(), 8 * N * 36); memcpy(a.B, bB.data(), 8 * N * 36);
                if (Cc) memcpy(a.A, bA.data(), 8 * Cc * 36);
                for (size_t i = 0; i < N * 6; i++) a.g[i] = 0.0;
                for (int i = 0; i < kPgScalars; i++) a.sc[i] = 0.0;
            }
            if (!pg_columns(be, a, b.dir, mg, x, &res, &tap, blocks)) { printf("the driver failed\n"); return 1; }
            printf("graph %d: n %d C %d, %d end nodes, %d targets: status %d (factor %d, Wm %d, Ks %d), %ld launches\n", gix, n, C, res.m, (int)T, res.status,
                   res.factor_status, res.wm_status, res.ks_status, be.launches);
            const int32_t oh[6] = {res.status, res.m, res.factor_status, res.wm_status, res.ks_status, res.reserved};
            if (!wr(out, oh, 6) || !wr(out, g.graph.ends.data(), m)) { printf("write failed\n"); return 2; }
            for (int i = 0; i < 4; i++) if (!wr(out, arr[(size_t)i].get(), sizes[i])) { printf("write failed\n"); return 2; }
            if (!wr(out, mg.cov, N * 36) || !wr(out, x.cols, (size_t)T * N * 36)) { printf("write failed\n"); return 2; }
        }
        // ---- the gate, a run of its own ----
        if (n_cand > 0) {
            std::vector<int32_t> gt, tcol;
            if (!pg_gate_targets(n, n_cand, gi.data(), gj.data(), gt, tcol) || gt.size() > (size_t)kPgCrossMaxTargets) { printf("bad candidates\n"); return 2; }
            HostBound b(g, true, false);
            PgArgs& a = b.a;
            PgMarg mg{};
            PgCross x{};
            PgGate gate{};
            pg_bind_marg(a, b.dir, mg, b.al, true);
            const PgCrossDev xd = pg_bind_cross(a, b.dir, x, b.al, (int)gt.size(), true);
            const PgGateDev gd = pg_bind_gate(gate, b.al, n_cand, true, true);
            memcpy(xd.targets, gt.data(), 4 * gt.size());
            memcpy(gd.gi, gi.data(), 4 * (size_t)n_cand); memcpy(gd.gj, gj.data(), 4 * (size_t)n_cand); memcpy(gd.tcol, tcol.data(), 4 * (size_t)n_cand);
            std::unique_ptr<float[]> hX(new float[(size_t)n_cand * 6]), hcov(new float[(size_t)n_cand * 36]);
            memcpy(hX.get(), cX.data(), 4 * (size_t)n_cand * 6); memcpy(hcov.get(), ccov.data(), 4 * (size_t)n_cand * 36);
            gate.X = hX.get(); gate.cov = hcov.get();
            CrossHostBackend be;
            icet_pose_graph_gate_result res{};
            if (!pg_gate(be, a, b.dir, mg, x, gate, threshold > 0.0 ? threshold : pg::kRobustDefaultScale, &res)) { printf("the driver failed\n"); return 1; }
            printf("graph %d: %d candidates, %d targets, %d rejected, %ld launches\n", gix, (int)n_cand, res.n_targets, res.rejected, be.launches);
            const int32_t oh[3] = {res.marg.status, res.n_targets, res.rejected};
            if (!wr(out, oh, 3) || !wr(out, gate.d2, (size_t)n_cand) || !wr(out, gate.S, (size_t)n_cand * 36) || !wr(out, gate.status, (size_t)n_cand)) { printf("write failed\n"); return 2; }
        }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("OK\n");
    return 0;
}
