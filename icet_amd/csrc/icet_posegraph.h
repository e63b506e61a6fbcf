// icet_amd/csrc/icet_posegraph.h -- the RULE of the pose-graph optimiser (include/icet_hip.h icet_pose_graph_optimize_device), in one
// place: the predicted measurement of an edge from two poses, the angle wrap, the right update T <- T Exp(delta), the residual and its central-difference
// Jacobians, the numbering of the edges and the incidence lists.  HIP-free C++: the kernel of icet_posegraph.hip, the host entry points and the CPU test
// (tests/cpp/test_posegraph.cpp) compile this text.
//
// POSE (device state): 12 doubles, R row-major 3 x 3 then t; p_world = R p + t.  An edge (i, j) measures keyframe i from live scan j:
// R(X) = R_j^T R_i, X_t = R_j^T (t_j - t_i), the angles by euler_of_R (icet_closure.h): the store's START POSE rule, here without the rounding to float32.
// EDGES: edge e < N - 1 is the odometry edge (e, e + 1); edge N - 1 + c is closure c.
// INCIDENCE: per node the items 2 e + side (side 0: the node is the edge's end i, 1: its end j) of its free edges in ascending order -- every per-node sum
// walks them in that order, so it has one order whatever the launch.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ICET_PG_HD __host__ __device__
#else
#define ICET_PG_HD
#endif

namespace icet_pg_rule {

constexpr int kMaxNodes = 4096;
constexpr int kMaxClosures = 512;
constexpr int kPgDirectMaxEnds = 128;       // the direct solve (icet_posegraph_direct.h): end nodes of closures off the band; 6 x 128 = 768 columns, one workgroup factors them
constexpr double kPi = 3.14159265358979323846;
constexpr double kJacStep = 1e-6;            // central differences, fixed step
constexpr double kPivotRel = 1e-13;          // a Cholesky pivot at or below this fraction of its diagonal entry: not positive definite

enum Status { kConverged = 0, kIterationCap = 1, kNotPositiveDefinite = 2, kNonFinite = 3, kStalled = 4 };

// a into (-pi, pi]
ICET_PG_HD inline double wrap_pi(double a) {
    const double w = a - 2.0 * kPi * ceil((a - kPi) / (2.0 * kPi));
    return w > kPi ? kPi : (w <= -kPi ? kPi : w);      // (rounding at the seam)
}

ICET_PG_HD inline void pose_from_float(const float T[16], double P[12]) {
    for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) P[3 * a + b] = (double)T[4 * a + b]; P[9 + a] = (double)T[4 * a + 3]; }
}
ICET_PG_HD inline void pose_to_float(const double P[12], float T[16]) {
    for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) T[4 * a + b] = (float)P[3 * a + b]; T[4 * a + 3] = (float)P[9 + a]; }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

// The predicted measurement of edge (i, j): x = (X_t, phi, theta, psi).
ICET_PG_HD inline void xof(const double Pi[12], const double Pj[12], double x[6]) {
    double RX[9], d[3];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) RX[3 * a + b] = Pj[0 + a] * Pi[0 + b] + Pj[3 + a] * Pi[3 + b] + Pj[6 + a] * Pi[6 + b];
    for (int c = 0; c < 3; c++) d[c] = Pj[9 + c] - Pi[9 + c];
    for (int a = 0; a < 3; a++) x[a] = Pj[0 + a] * d[0] + Pj[3 + a] * d[1] + Pj[6 + a] * d[2];
    const double s = RX[6] > 1.0 ? 1.0 : (RX[6] < -1.0 ? -1.0 : RX[6]);
    x[3] = atan2(-RX[7], RX[8]);
    x[4] = asin(s);
    x[5] = atan2(-RX[3], RX[0]);
}

// e = xof - X, the angles wrapped
ICET_PG_HD inline void residual(const double Pi[12], const double Pj[12], const float X[6], double e[6]) {
    double x[6];
    xof(Pi, Pj, x);
    for (int a = 0; a < 3; a++) e[a] = x[a] - (double)X[a];
    for (int a = 3; a < 6; a++) e[a] = wrap_pi(x[a] - (double)X[a]);
}

// Q = P Exp(delta), delta = (rho, omega): Exp = [Rodrigues(omega) | V(omega) rho], the exponential of se(3).
ICET_PG_HD inline void exp_update(const double P[12], const double delta[6], double Q[12]) {
    const double wx = delta[3], wy = delta[4], wz = delta[5];
    const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    double A, B, Cc;
    if (th < 1e-4) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; Cc = 1.0 / 6.0 - th2 / 120.0; }
    else { A = sin(th) / th; B = (1.0 - cos(th)) / th2; Cc = (th - sin(th)) / (th2 * th); }
    const double K[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double K2[9], E[9], V[9];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) K2[3 * a + b] = K[3 * a + 0] * K[0 + b] + K[3 * a + 1] * K[3 + b] + K[3 * a + 2] * K[6 + b];
    for (int k = 0; k < 9; k++) { const double I = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0; E[k] = I + A * K[k] + B * K2[k]; V[k] = I + B * K[k] + Cc * K2[k]; }
    double u[3];
    for (int a = 0; a < 3; a++) u[a] = V[3 * a + 0] * delta[0] + V[3 * a + 1] * delta[1] + V[3 * a + 2] * delta[2];
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) Q[3 * a + b] = P[3 * a + 0] * E[0 + b] + P[3 * a + 1] * E[3 + b] + P[3 * a + 2] * E[6 + b];
        Q[9 + a] = P[9 + a] + (P[3 * a + 0] * u[0] + P[3 * a + 1] * u[1] + P[3 * a + 2] * u[2]);
    }
}

// Column `col` (0 .. 5: a perturbation of node i, 6 .. 11: of node j) of the edge's 6 x 12 Jacobian by central differences.
ICET_PG_HD inline void jacobian_column(const double Pi[12], const double Pj[12], int col, double out[6]) {
    double dp[6] = {0, 0, 0, 0, 0, 0}, dm[6] = {0, 0, 0, 0, 0, 0}, Q[12], xp[6], xm[6];
    dp[col % 6] = kJacStep; dm[col % 6] = -kJacStep;
    if (col < 6) { exp_update(Pi, dp, Q); xof(Q, Pj, xp); exp_update(Pi, dm, Q); xof(Q, Pj, xm); }
    else         { exp_update(Pj, dp, Q); xof(Pi, Q, xp); exp_update(Pj, dm, Q); xof(Pi, Q, xm); }
    for (int a = 0; a < 3; a++) out[a] = (xp[a] - xm[a]) / (2.0 * kJacStep);
    for (int a = 3; a < 6; a++) out[a] = wrap_pi(xp[a] - xm[a]) / (2.0 * kJacStep);
}

// ---- robust kernels (DESIGN.md section 20 "Robust kernels") --------------------------------------------------------------------------------------------------
// Per edge s = e^T Omega e, c > 0 the threshold in chi2 units: the objective is F = sum rho(s), an edge's weight in H and g is w(s) = rho'(s).  Where !(s > 0)
// every kind has rho = s and w = 1 (a NaN s stays a NaN cost).  tests/pose_graph_robust_model.py restates each expression in this order of operations.
enum RobustKind { kRobustNone = 0, kRobustHuber = 1, kRobustCauchy = 2, kRobustGemanMcClure = 3 };
constexpr int kRobustOdometry = 1;                    // flag bit 0 (ICET_PG_ROBUST_ODOMETRY): the odometry edges take the kind too
constexpr double kRobustDefaultScale = 16.8119;       // the 99 % quantile of chi2 with six degrees of freedom

ICET_PG_HD inline double robust_rho(int kind, double c, double s) {
    if (!(s > 0.0)) return s;
    if (kind == kRobustHuber) return s <= c ? s : 2.0 * sqrt(c * s) - c;
    if (kind == kRobustCauchy) return c * log1p(s / c);
    if (kind == kRobustGemanMcClure) return c * s / (c + s);
    return s;
}
ICET_PG_HD inline double robust_weight(int kind, double c, double s) {
    if (!(s > 0.0)) return 1.0;
    if (kind == kRobustHuber) return s <= c ? 1.0 : sqrt(c / s);
    if (kind == kRobustCauchy) return 1.0 / (1.0 + s / c);
    if (kind == kRobustGemanMcClure) { const double t = c / (c + s); return t * t; }
    return 1.0;
}
// The kind edge e of a chain of N nodes takes: the closures always, the odometry edges (e < N - 1) only under kRobustOdometry
ICET_PG_HD inline int robust_kind_of_edge(int kind, int flags, int N, int e) { return (e >= N - 1 || (flags & kRobustOdometry)) ? kind : (int)kRobustNone; }
// (host) true for a (kind, flags, scale) the optimiser takes: kind 0 .. 3, no flag bit but bit 0, and with a kind a scale that is finite and positive
inline bool robust_ok(int kind, int flags, double scale) {
    if (kind < kRobustNone || kind > kRobustGemanMcClure || (flags & ~kRobustOdometry) != 0) return false;
    return kind == kRobustNone || (scale > 0.0 && scale <= 1.7976931348623157e308);
}

ICET_PG_HD inline int edge_count(int N, int C) { return N - 1 + C; }

// (host) true when the closure list is one the optimiser takes: indices in range, i != j
inline bool closures_ok(int N, int C, const int32_t* ci, const int32_t* cj) {
    for (int c = 0; c < C; c++)
        if (ci[c] < 0 || ci[c] >= N || cj[c] < 0 || cj[c] >= N || ci[c] == cj[c]) return false;
    return true;
}

// The ends of every edge (ei, ej: E entries) and the incidence lists: off (N + 1 entries), items (off[N] entries).  A fixed node (node 0 always; fixed[k] != 0)
// has an empty list: nothing is summed for it.  Items ascend within a node because the edges are visited in ascending order.
template <class VecI>
inline void build_incidence(int N, int C, const int32_t* ci, const int32_t* cj, const uint8_t* fixed, VecI& ei, VecI& ej, VecI& off, VecI& items) {
    const int E = edge_count(N, C);
    ei.assign((size_t)E, 0); ej.assign((size_t)E, 0);
    for (int e = 0; e < N - 1; e++) { ei[e] = e; ej[e] = e + 1; }
    for (int c = 0; c < C; c++) { ei[N - 1 + c] = ci[c]; ej[N - 1 + c] = cj[c]; }
    auto is_fixed = [&](int k) { return k == 0 || (fixed && fixed[k]); };
    off.assign((size_t)N + 1, 0);
    for (int e = 0; e < E; e++) { if (!is_fixed(ei[e])) off[ei[e] + 1]++; if (!is_fixed(ej[e])) off[ej[e] + 1]++; }
    for (int k = 0; k < N; k++) off[k + 1] += off[k];
    items.assign((size_t)off[N], 0);
    VecI fill(off.begin(), off.end() - 1);
    for (int e = 0; e < E; e++) {
        if (!is_fixed(ei[e])) items[fill[ei[e]]++] = 2 * e;
        if (!is_fixed(ej[e])) items[fill[ej[e]]++] = 2 * e + 1;
    }
}

}  // namespace icet_pg_rule
