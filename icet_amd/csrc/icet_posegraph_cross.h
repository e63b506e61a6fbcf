// icet_amd/csrc/icet_posegraph_cross.h -- the kernel bodies of the pose graph's COVARIANCE COLUMNS and of the COVARIANCE GATE (DESIGN.md section 20 "Covariance
// columns and the gate"): block (k, t) of H^-1 for every node k and each of T target nodes t, and the Mahalanobis test of a candidate closure under the
// covariance of the relative pose of its two ends.  HIP-free, behind the macros of icet_posegraph_body.h: device code under hipcc, one host thread under a host
// compiler, four with a barrier under ICET_PG_EMU (tests/cpp/test_posegraph_cross.cpp).  icet_posegraph.hip has the launches, icet_posegraph_driver.h
// (pg_columns, pg_gate) the order they run in.
//
// With the marginals' H^-1 = M^-1 - P P^T + Q Q^T (icet_posegraph_marginals.h):
//     block (k, t) of H^-1 = [M^-1](k, t) - P_k P_t^T + Q_k Q_t^T
// [M^-1](., t) are the band solves for the target's six unit columns, Zt = M^-1 E_T: pg_z with the targets in the place of the end nodes.  P_t and Q_t of the
// targets are formed once (one workgroup per target, pg_marg_forward) and kept in global memory; one workgroup per node k then forms P_k, then Q_k, in LDS in
// place and writes its 36 T entries.  The block at k = t is the marginals' own, copied.  A fixed node carries the identity in M and no coupling: every block
// that touches one is zero, whatever Zt holds there.
// No atomics, no block waits on another, every loop is bounded by N, q, T or 6, no per-thread array takes a run-time index, every output entry is one thread's
// sum in a fixed order.
#pragma once
#include "icet_posegraph_marginals.h"

namespace icet {

constexpr int kPgCrossMaxTargets = ICET_PG_MAX_TARGETS;      // 32: a node's 36 T products fit in LDS beside its rows of Z (9 KB)
constexpr int kPgGateMaxCand = 512;

// The columns' own arrays (pg_bind_cross), beside PgArgs, PgDirect and PgMarg.  nq is the direct solve's q.
struct PgCross {
    int T;                          // targets
    const int32_t* targets;         // T: the target nodes, distinct
    double *Zt;                     // 6N x 6T: M^-1 E_T, [row][col], column 6 t + c is component c of target t
    double *Pt, *Qt;                // T x 6 x nq: the targets' six rows of P and of Q
    double *cols;                   // T x N x 36: the result, block (k, targets[t]) at [t][k]
};

// The gate's candidates (pg_bind_gate): n closures that are not in the graph
struct PgGate {
    int n;
    const int32_t *gi, *gj;         // n: keyframe node, live node
    const int32_t *tcol;            // n: the index of gj among the targets
    const float *X, *cov;           // n x 6, n x 36
    double *d2;                     // n
    double *S;                      // n x 36, or null
    int32_t* status;                // n
};

enum PgCrossGroupKernel { kPgCrossTarget = 0, kPgCrossNode, kPgGateCand };

struct PgCrossShared { double z[6 * kPgMargCols]; double pp[36 * kPgCrossMaxTargets]; };
struct PgGateShared { double Sg[144], J[72], K[72], S[36], L[36], e[6], y[6]; };

// One workgroup per target: its six rows of Z become P_t, then Q_t, in LDS in place; both go to global memory.  A fixed target's rows are zero.
ICET_PG_DEV void pg_group_cross_target(const PgArgs& a, const PgDirect& d, const PgMarg& mg, const PgCross& x, int tt, PgMargShared& sh) {
    const int t = ICET_PG_TID, q = d.nq;
    if (q == 0 || pg_direct_failed(a)) return;          // (the same for every thread)
    const int tg = x.targets[tt];
    double* Pt = x.Pt + (size_t)tt * 6 * (size_t)q;
    double* Qt = x.Qt + (size_t)tt * 6 * (size_t)q;
    if (pg_fixed(a, tg)) {
        for (int i = t; i < 6 * q; i += kPgThreads) { Pt[i] = 0.0; Qt[i] = 0.0; }
        return;
    }
    const double* Zk = d.Z + (size_t)tg * 6 * (size_t)q;
    for (int i = t; i < 6 * q; i += kPgThreads) sh.z[i] = Zk[i];
    ICET_PG_SYNC();
    pg_marg_forward(q, mg.Lt, d.rdw, sh.z);
    for (int i = t; i < 6 * q; i += kPgThreads) Pt[i] = sh.z[i];
    ICET_PG_SYNC();
    pg_marg_forward(q, mg.Lkt, d.rdk, sh.z);
    for (int i = t; i < 6 * q; i += kPgThreads) Qt[i] = sh.z[i];
    ICET_PG_SYNC();
}

// entry e = (r, c) of zk zt^T, over the columns in ascending order
ICET_PG_DEV double pg_cross_dot(int q, const double* zk, const double* zt, int e) {
    const double* zr = zk + (size_t)(e / 6) * q; const double* zc = zt + (size_t)(e % 6) * q;
    double s = 0.0;
    for (int j = 0; j < q; j++) s += zr[j] * zc[j];
    return s;
}

// One workgroup per node k: the T blocks (k, targets[t]) = Zt(k, t) - P_k P_t^T + Q_k Q_t^T, rows node k's tangent, columns the target's.  With q = 0 a block
// is Zt(k, t).  The block at k = targets[t] is the marginals' (mg.cov, written by an earlier launch).  A block that touches a fixed node is zero; behind a
// failed factorisation every other block is quiet NaN.
ICET_PG_DEV void pg_group_cross_node(const PgArgs& a, const PgDirect& d, const PgMarg& mg, const PgCross& x, int k, PgCrossShared& sh) {
    const int t = ICET_PG_TID, q = d.nq, T = x.T, nt = 36 * x.T;
    const size_t N = (size_t)a.N;
    const bool kfixed = pg_fixed(a, k);
    if (kfixed || pg_direct_failed(a)) {          // (the same for every thread)
        for (int i = t; i < nt; i += kPgThreads) {
            const int tt = i / 36;
            x.cols[((size_t)tt * N + (size_t)k) * 36 + i % 36] = (kfixed || pg_fixed(a, x.targets[tt])) ? 0.0 : pg_quiet_nan();
        }
        return;
    }
    if (q > 0) {
        const double* Zk = d.Z + (size_t)k * 6 * (size_t)q;
        for (int i = t; i < 6 * q; i += kPgThreads) sh.z[i] = Zk[i];
        ICET_PG_SYNC();
        pg_marg_forward(q, mg.Lt, d.rdw, sh.z);
        for (int i = t; i < nt; i += kPgThreads) sh.pp[i] = pg_cross_dot(q, sh.z, x.Pt + (size_t)(i / 36) * 6 * (size_t)q, i % 36);
        ICET_PG_SYNC();
        pg_marg_forward(q, mg.Lkt, d.rdk, sh.z);
    }
    for (int i = t; i < nt; i += kPgThreads) {
        const int tt = i / 36, e = i % 36, tg = x.targets[tt];
        double v;
        if (pg_fixed(a, tg)) v = 0.0;
        else if (tg == k) v = mg.cov[(size_t)k * 36 + e];
        else {
            v = x.Zt[((size_t)k * 6 + (size_t)(e / 6)) * (size_t)(6 * T) + (size_t)(6 * tt + e % 6)];
            if (q > 0) v = (v - sh.pp[i]) + pg_cross_dot(q, sh.z, x.Qt + (size_t)tt * 6 * (size_t)q, e);
        }
        x.cols[((size_t)tt * N + (size_t)k) * 36 + e] = v;
    }
    ICET_PG_SYNC();
}

// One workgroup per candidate c, behind the columns: the optimiser's residual e and central-difference Jacobians J = [J_i | J_j] of edge (gi, gj) at the poses
// (pg::residual, pg::jacobian_column: what pg_chi and pg_linearise run), S = J Sigma J^T + 0.5 (cov + cov^T) with Sigma the 12 x 12 joint covariance of the two
// nodes (its diagonal blocks the marginals', Sigma_ij the column of target gj at row gi), entry (r, c) taken at (max, min); then thread 0 factors S = L L^T and
// d2 = |L^-1 e|^2.  A pivot at or below kPivotRel x its diagonal entry: status kNotPositiveDefinite; one that is not finite: kNonFinite; d2 is then quiet NaN,
// as it is behind a failed factorisation of the graph.
ICET_PG_DEV void pg_group_gate(const PgArgs& a, const PgMarg& mg, const PgCross& x, const PgGate& g, int c, PgGateShared& sh) {
    const int t = ICET_PG_TID;
    const int i = g.gi[c], j = g.gj[c];
    const size_t N = (size_t)a.N;
    const double* Pi = a.P + (size_t)i * 12; const double* Pj = a.P + (size_t)j * 12;
    const double* Sii = mg.cov + (size_t)i * 36; const double* Sjj = mg.cov + (size_t)j * 36;
    const double* Sij = x.cols + ((size_t)g.tcol[c] * N + (size_t)i) * 36;
    const float* cv = g.cov + (size_t)c * 36;
    for (int n = t; n < 144; n += kPgThreads) {
        const int r = n / 12, s = n % 12;
        sh.Sg[n] = r < 6 ? (s < 6 ? Sii[r * 6 + s] : Sij[r * 6 + (s - 6)]) : (s < 6 ? Sij[s * 6 + (r - 6)] : Sjj[(r - 6) * 6 + (s - 6)]);
    }
    for (int col = t; col < 12; col += kPgThreads) {
        double jc[6];
        pg::jacobian_column(Pi, Pj, col, jc);
ICET_PG_UNROLL
        for (int m = 0; m < 6; m++) sh.J[m * 12 + col] = jc[m];
    }
    if (t == 0) {
        double r6[6];
        pg::residual(Pi, Pj, g.X + (size_t)c * 6, r6);
ICET_PG_UNROLL
        for (int m = 0; m < 6; m++) sh.e[m] = r6[m];
    }
    ICET_PG_SYNC();
    for (int n = t; n < 72; n += kPgThreads) {          // K = J Sigma
        const int m = n / 12, s = n % 12;
        double v = 0.0;
        for (int r = 0; r < 12; r++) v += sh.J[m * 12 + r] * sh.Sg[r * 12 + s];
        sh.K[n] = v;
    }
    ICET_PG_SYNC();
    for (int n = t; n < 36; n += kPgThreads) {
        const int r = n / 6, s = n % 6;
        const int rr = r > s ? r : s, cc = r > s ? s : r;
        double v = 0.0;
        for (int m = 0; m < 12; m++) v += sh.K[rr * 12 + m] * sh.J[cc * 12 + m];
        sh.S[n] = v + 0.5 * ((double)cv[rr * 6 + cc] + (double)cv[cc * 6 + rr]);
    }
    ICET_PG_SYNC();
    if (t == 0) {
        int st = 0;
        for (int n = 0; n < 6 && st == 0; n++)
            for (int m = n; m < 6; m++) {
                double s = sh.S[m * 6 + n];
                for (int r = 0; r < n; r++) s -= sh.L[m * 6 + r] * sh.L[n * 6 + r];
                if (m == n) {
                    if (s != s || fabs(s) > 1.7e308) { st = pg::kNonFinite; break; }
                    if (!(s > pg::kPivotRel * fabs(sh.S[n * 6 + n]))) { st = pg::kNotPositiveDefinite; break; }
                    sh.L[n * 6 + n] = sqrt(s);
                } else {
                    sh.L[m * 6 + n] = s / sh.L[n * 6 + n];
                }
            }
        double d2 = 0.0;
        if (st == 0) {
            for (int m = 0; m < 6; m++) {
                double s = sh.e[m];
                for (int r = 0; r < m; r++) s -= sh.L[m * 6 + r] * sh.y[r];
                sh.y[m] = s / sh.L[m * 6 + m];
                d2 += sh.y[m] * sh.y[m];
            }
        }
        g.d2[c] = (st != 0 || pg_direct_failed(a)) ? pg_quiet_nan() : d2;
        g.status[c] = st;
    }
    if (g.S) for (int n = t; n < 36; n += kPgThreads) g.S[(size_t)c * 36 + n] = sh.S[n];
    ICET_PG_SYNC();
}

}  // namespace icet
