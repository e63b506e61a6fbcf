// tests/cpp/test_node_tail.cpp -- icet_amd/csrc/icet_node_tail.h on the inputs a frame's tail must survive without touching memory it does not own (g++ only, no
// GPU): singular matrices into inverse3_lu, NaN and inf in X, a pose of zeros, and a few ordinary ones.  Prints every result as the bits of its floats (a NaN as
// "nan": which NaN an operation returns is not part of the contract).  Build: g++ -std=c++17 -I <repo root>, plain and with -fsanitize=address,undefined; both
// builds must print the same bytes (tests/test_node_tail.py).
#include "icet_amd/csrc/icet_node_tail.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

namespace {

void show(const char* what, const float* v, int n) {
    std::printf("%s", what);
    for (int i = 0; i < n; i++) {
        if (std::isnan(v[i])) { std::printf(" nan"); continue; }
        uint32_t b; std::memcpy(&b, &v[i], sizeof(b));
        std::printf(" %08x", (unsigned)b);
    }
    std::printf("\n");
}

// the compiler must not fold the cases at build time (a folded NaN or a folded libm call need not be the run-time one)
void launder(float* v, int n) { volatile float* p = v; for (int i = 0; i < n; i++) { const float x = p[i]; p[i] = x; } }

void inverse_case(const char* what, const float A_in[9]) {
    float A[9], inv[9];
    std::memcpy(A, A_in, sizeof(A)); launder(A, 9);
    icet_node_tail::inverse3_lu(A, inv);
    show(what, inv, 9);
}

void tail_case(const char* what, const float X_in[6], const float pose_in[16]) {
    float X[6], pose[16], R[9], Ri[9], P[16], q[4];
    std::memcpy(X, X_in, sizeof(X)); std::memcpy(pose, pose_in, sizeof(pose)); launder(X, 6); launder(pose, 16);
    icet_node_tail::tail_scalars(X, pose, R, Ri, P, q);
    std::printf("%s\n", what);
    show("  R   ", R, 9); show("  Rinv", Ri, 9); show("  pose", P, 16); show("  quat", q, 4);
}

}  // namespace

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, Z4[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // ---- inverse3_lu: singular and nearly singular matrices (the `== 0` skip, divisions by a zero pivot), a permutation (every pivot search swaps)
    { const float A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; inverse_case("inverse zeros      ", A); }
    { const float A[9] = {1, 2, 3, 2, 4, 6, 3, 6, 9}; inverse_case("inverse rank one   ", A); }
    { const float A[9] = {1, 0, 0, 0, 0, 0, 0, 0, 1}; inverse_case("inverse zero row   ", A); }
    { const float A[9] = {0, 1, 2, 0, 3, 4, 0, 5, 6}; inverse_case("inverse zero column", A); }
    { const float A[9] = {0, 0, 1, 1, 0, 0, 0, 1, 0}; inverse_case("inverse permutation", A); }
    { const float A[9] = {nan, 0, 0, 0, 1, 0, 0, 0, 1}; inverse_case("inverse nan entry  ", A); }
    { const float A[9] = {inf, 0, 0, 0, 1, 0, 0, 0, 1}; inverse_case("inverse inf entry  ", A); }
    { const float A[9] = {1e-45f, 0, 0, 0, 1e-45f, 0, 0, 0, 1e-45f}; inverse_case("inverse denormal   ", A); }
    // ---- the whole tail
    { const float X[6] = {0, 0, 0, 0, 0, 0}; tail_case("tail X = 0, identity pose", X, I4); }
    { const float X[6] = {0.3f, -0.12f, 0.04f, 0.02f, -0.015f, 0.04f}; tail_case("tail ordinary X, identity pose", X, I4); }
    { const float X[6] = {0.3f, -0.12f, 0.04f, 0.02f, -0.015f, 0.04f}; tail_case("tail ordinary X, pose of zeros", X, Z4); }
    { const float X[6] = {0, 0, 0, 0, 0, 0}; tail_case("tail X = 0, pose of zeros", X, Z4); }
    { const float X[6] = {nan, 0, 0, 0, 0, 0}; tail_case("tail nan translation", X, I4); }
    { const float X[6] = {0, 0, 0, nan, 0, 0}; tail_case("tail nan angle", X, I4); }
    { const float X[6] = {inf, -inf, 0, 0, 0, 0}; tail_case("tail inf translation", X, I4); }
    { const float X[6] = {0, 0, 0, inf, 0.1f, -inf}; tail_case("tail inf angles", X, I4); }
    { const float X[6] = {nan, nan, nan, nan, nan, nan}; tail_case("tail all nan, pose of zeros", X, Z4); }
    { const float X[6] = {1, 2, 3, 1.5707964f, 1.5707964f, 3.1415927f};
      const float P[16] = {inf, 0, 0, 0, 0, nan, 0, 0, 0, 0, -inf, 0, 0, 0, 0, 1}; tail_case("tail quarter turns, pose of inf and nan", X, P); }
    // ---- quat_of alone: every branch on a matrix that is no rotation at all
    { float q[4]; float P[16]; std::memcpy(P, Z4, sizeof(P)); P[0] = -1; P[5] = -1; P[10] = -1; launder(P, 16); icet_node_tail::quat_of(P, q); show("quat of -I            ", q, 4); }
    { float q[4]; float P[16]; std::memcpy(P, Z4, sizeof(P)); P[0] = -3; P[5] = 1; P[10] = 1; launder(P, 16); icet_node_tail::quat_of(P, q); show("quat of diag(-3, 1, 1)", q, 4); }
    std::printf("OK\n");
    return 0;
}
