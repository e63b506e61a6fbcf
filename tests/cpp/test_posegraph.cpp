// tests/cpp/test_posegraph.cpp -- the host side of the pose-graph optimiser (icet_amd/csrc/icet_posegraph.h: the predicted measurement, Exp, the angle wrap, the
// incidence lists) and, as a "workgroup" of one thread, the body the device runs (icet_posegraph_body.h): the band factorisation and sweeps held to their
// backward error, a singular block.  Build: g++ -std=c++17 -I <repo root> (also with -fsanitize=address,undefined).  Prints OK.
#include "icet_amd/csrc/icet_posegraph_body.h"
#include "icet_amd/csrc/icet_closure.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace pg = icet_pg_rule;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static void ident(double P[12]) { for (int i = 0; i < 12; i++) P[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0; }

static void test_wrap() {
    CHECK(pg::wrap_pi(pg::kPi) == pg::kPi);
    CHECK(pg::wrap_pi(-pg::kPi) == pg::kPi);
    CHECK(pg::wrap_pi(std::nextafter(pg::kPi, 4.0)) < 0 && pg::wrap_pi(std::nextafter(pg::kPi, 4.0)) > -pg::kPi - 1e-15);
    CHECK(std::fabs(std::fabs(pg::wrap_pi(std::nextafter(-pg::kPi, 0.0))) - pg::kPi) < 1e-15);       // (either end of the seam)
    CHECK(pg::wrap_pi(0.25) == 0.25 && pg::wrap_pi(-0.25) == -0.25);
    CHECK(std::fabs(pg::wrap_pi(3 * pg::kPi) - pg::kPi) < 1e-14);
    CHECK(std::fabs(pg::wrap_pi(2 * pg::kPi + 0.5) - 0.5) < 1e-14 && std::fabs(pg::wrap_pi(-2 * pg::kPi - 0.5) + 0.5) < 1e-14);
    for (double a = -20; a < 20; a += 0.37) { const double w = pg::wrap_pi(a); CHECK(w > -pg::kPi && w <= pg::kPi && std::fabs(std::remainder(w - a, 2 * pg::kPi)) < 1e-12); }
    // a residual across the seam: psi of the prediction just above -pi, of the measurement just below pi
    double Pi[12], Pj[12], e[6]; ident(Pi); ident(Pj);
    const double d0[6] = {0, 0, 0, 0, 0, -(pg::kPi - 0.01)};          // psi of R_j^T R_i = -(pi - 0.01) (the library's R(X) turns by -psi about z)
    pg::exp_update(Pi, d0, Pj);
    const float X[6] = {0, 0, 0, 0, 0, (float)(pg::kPi - 0.01)};
    pg::residual(Pi, Pj, X, e);
    CHECK(std::fabs(std::fabs(e[5]) - 0.02) < 1e-6);
}

static void test_xof_and_exp() {
    // xof agrees with the store's START POSE rule and inverts pose_step_from_X
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    for (int rep = 0; rep < 50; rep++) {
        float X[6] = {3 * u(rng), 3 * u(rng), u(rng), 0.3f * u(rng), 0.3f * u(rng), 3.0f * u(rng)}, S[16], T0[16], T1[16];
        icet_closure_rule::pose_step_from_X(X, S);
        const float X0[6] = {u(rng), u(rng), u(rng), 0.2f * u(rng), 0.2f * u(rng), u(rng)};
        icet_closure_rule::pose_step_from_X(X0, T0);
        for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) { double s = 0; for (int m = 0; m < 4; m++) s += (double)T0[4 * a + m] * (double)S[4 * m + b]; T1[4 * a + b] = (float)s; }
        double P0[12], P1[12], x[6]; float x0[6];
        pg::pose_from_float(T0, P0); pg::pose_from_float(T1, P1);
        pg::xof(P0, P1, x);
        icet_closure_rule::start_pose_T(T1, T0, x0);
        for (int a = 0; a < 6; a++) { CHECK(std::fabs(x[a] - (double)x0[a]) < 1e-6); CHECK(std::fabs(x[a] - (double)X[a]) < 2e-5); }
    }
    // Exp: a rotation, orthonormal; Exp(d) Exp(-d) = I; the small-angle branch joins the other
    double P[12], Q[12], R[12]; ident(P);
    const double d[6] = {0.3, -0.2, 0.5, 0.4, -0.7, 1.1}, md[6] = {-0.3, 0.2, -0.5, -0.4, 0.7, -1.1};
    pg::exp_update(P, d, Q); pg::exp_update(Q, md, R);
    for (int i = 0; i < 12; i++) CHECK(std::fabs(R[i] - P[i]) < 1e-14);
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) { double s = 0; for (int m = 0; m < 3; m++) s += Q[3 * m + a] * Q[3 * m + b]; CHECK(std::fabs(s - (a == b)) < 1e-14); }
    const double z[6] = {1, 2, 3, 0, 0, 0};
    pg::exp_update(Q, z, R);          // a pure translation moves t by R z
    for (int a = 0; a < 3; a++) CHECK(std::fabs(R[9 + a] - (Q[9 + a] + Q[3 * a] * 1 + Q[3 * a + 1] * 2 + Q[3 * a + 2] * 3)) < 1e-14);
    const double s1[6] = {0.1, 0.2, 0.3, 0.99e-4 / std::sqrt(3.0), 0.99e-4 / std::sqrt(3.0), 0.99e-4 / std::sqrt(3.0)}, s2[6] = {0.1, 0.2, 0.3, 1.01e-4 / std::sqrt(3.0), 1.01e-4 / std::sqrt(3.0), 1.01e-4 / std::sqrt(3.0)};
    pg::exp_update(P, s1, Q); pg::exp_update(P, s2, R);
    for (int i = 0; i < 12; i++) CHECK(std::fabs(Q[i] - R[i]) < 3e-6);
    // the Jacobian of an identity pair: d x_t / d rho_j = I, d x_t / d rho_i = -I
    double Pi[12], Pj[12], jc[6]; ident(Pi); ident(Pj);
    for (int c = 0; c < 3; c++) { pg::jacobian_column(Pi, Pj, c, jc); CHECK(std::fabs(jc[c] + 1) < 1e-8); pg::jacobian_column(Pi, Pj, 6 + c, jc); CHECK(std::fabs(jc[c] - 1) < 1e-8); }
}

static void test_incidence() {
    // 6 nodes; closures: a repeat, an adjacent one, a reversed one, one ending on the fixed node 0, one ending on the fixed node 4
    const int N = 6, C = 6;
    const int32_t ci[C] = {1, 1, 2, 5, 0, 4}, cj[C] = {5, 5, 3, 2, 3, 1};
    uint8_t fixed[N] = {0, 0, 0, 0, 1, 0};
    std::vector<int32_t> ei, ej, off, items;
    CHECK(pg::closures_ok(N, C, ci, cj));
    pg::build_incidence(N, C, ci, cj, fixed, ei, ej, off, items);
    const int E = N - 1 + C;
    CHECK((int)ei.size() == E && (int)off.size() == N + 1);
    CHECK(off[0] == 0 && off[1] == 0);                    // node 0: fixed, empty
    CHECK(off[5] == off[4]);                              // node 4: fixed, empty
    int count = 0;
    for (int k = 0; k < N; k++)
        for (int it = off[k]; it < off[k + 1]; it++) {
            const int e = items[it] >> 1, side = items[it] & 1;
            CHECK((side ? ej[e] : ei[e]) == k);
            if (it > off[k]) CHECK(items[it] > items[it - 1]);
            count++;
        }
    int want = 0;
    for (int e = 0; e < E; e++) { want += (ei[e] != 0 && ei[e] != 4); want += (ej[e] != 0 && ej[e] != 4); }
    CHECK(count == want && (int)items.size() == want);
    // node 1: odometry edges 0 (as j) and 1 (as i), closures 5, 6 (as i) and 10 (as j)
    const int32_t n1[] = {2 * 0 + 1, 2 * 1, 2 * 5, 2 * 6, 2 * 10 + 1};
    CHECK(off[2] - off[1] == 5);
    for (int q = 0; q < 5 && off[2] - off[1] == 5; q++) CHECK(items[off[1] + q] == n1[q]);
    const int32_t bi[1] = {2}, bj[1] = {2}, oi[1] = {0}, oj[1] = {6};
    CHECK(!pg::closures_ok(N, 1, bi, bj) && !pg::closures_ok(N, 1, oi, oj) && !pg::closures_ok(N, 1, oj, oi) && pg::closures_ok(N, 0, nullptr, nullptr));
}

// ---- the device's body as one thread ---------------------------------------------------------------------------------------------------------------------
static void test_band(int N, double cond) {
    std::mt19937 rng(100 + N);
    std::normal_distribution<double> g(0, 1);
    // a chain Laplacian of SPD blocks: M = sum_k E_k^T K_k E_k, E_k x = x_k - x_{k-1} (x_{-1} = 0)
    std::vector<double> D((size_t)N * 36, 0.0), B((size_t)N * 36, 0.0), rhs((size_t)N * 6), x((size_t)N * 6), G((size_t)N * 36), W((size_t)N * 36), u((size_t)N * 6);
    for (int k = 0; k < N; k++) {
        double A[36], K[36];
        for (int i = 0; i < 36; i++) A[i] = g(rng);
        for (int r = 0; r < 6; r++) for (int c = 0; c < 6; c++) { double s = 0; for (int m = 0; m < 6; m++) s += A[r * 6 + m] * std::pow(cond, m / 5.0 - 1.0) * A[c * 6 + m]; K[r * 6 + c] = s; }
        for (int i = 0; i < 36; i++) { D[(size_t)k * 36 + i] += K[i]; if (k > 0) { D[(size_t)(k - 1) * 36 + i] += K[i]; B[(size_t)k * 36 + i] = -K[i]; } }
        for (int r = 0; r < 6; r++) rhs[(size_t)k * 6 + r] = g(rng);
    }
    int32_t status = -1;
    static icet::PgShared sh;
    icet::pg_block_tridiag(N, D.data(), B.data(), rhs.data(), x.data(), G.data(), W.data(), u.data(), &status, sh);
    CHECK(status == 0);
    double rn = 0, bn = 0, mn = 0, xn = 0;
    for (size_t i = 0; i < D.size(); i++) mn += D[i] * D[i] + 2 * B[i] * B[i];
    for (size_t i = 0; i < x.size(); i++) xn += x[i] * x[i];
    for (int k = 0; k < N; k++)
        for (int r = 0; r < 6; r++) {
            double s = -rhs[(size_t)k * 6 + r];
            for (int c = 0; c < 6; c++) {
                s += D[(size_t)k * 36 + r * 6 + c] * x[(size_t)k * 6 + c];
                if (k > 0) s += B[(size_t)k * 36 + r * 6 + c] * x[(size_t)(k - 1) * 6 + c];
                if (k < N - 1) s += B[(size_t)(k + 1) * 36 + c * 6 + r] * x[(size_t)(k + 1) * 6 + c];
            }
            rn += s * s; bn += rhs[(size_t)k * 6 + r] * rhs[(size_t)k * 6 + r];
        }
    CHECK(std::sqrt(rn) <= 1e-14 * (std::sqrt(mn) * std::sqrt(xn) + std::sqrt(bn)));      // backward stable: the residual against |M| |x| + |b|
    // a singular block is reported, never divided by
    for (int i = 0; i < 6; i++) { D[i * 6 + 2] = 0; D[2 * 6 + i] = 0; }
    if (N > 1) for (int i = 0; i < 6; i++) B[36 + i * 6 + 2] = 0;
    icet::pg_block_tridiag(N, D.data(), B.data(), rhs.data(), x.data(), G.data(), W.data(), u.data(), &status, sh);
    CHECK(status == pg::kNotPositiveDefinite);
}

int main() {
    test_wrap();
    test_xof_and_exp();
    test_incidence();
    for (int N : {1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 257}) test_band(N, 1e8);
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("OK\n");
    return 0;
}
