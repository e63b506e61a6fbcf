// icet_amd/csrc/icet_map_shape.h -- the RULE of the voxel map's shape (include/icet_hip.h icet_voxel_map_enable_shape / icet_voxel_map_extract_shape*; DESIGN.md
// section 25), in one place: what a kept row adds to the nine moment words of its cell, a cell's covariance from its integer moments, and the eigenvalues and
// the normal of that covariance.  HIP-free C++: the kernels and the host code of icet_map.hip and the CPU test (tests/cpp/test_map_shape_rule.cpp) compile this text.
//
// ARITHMETIC: as icet_map.h -- IEEE double, one rounding per operation, nothing contracted, division and square root correctly rounded.  What a row ADDS is
// integers only: with q_a the 32-bit offset of step 4 of the map's rule, h_a = q_a >> 16 (0 .. 65535), S_a += sign h_a and M_ab += sign h_a h_b in 64-bit
// two's-complement words.  h_a h_b < 2^32, so a cell holds 2^32 rows, as its offset sums do, and the words depend on the multiset of (row, pose, sign) only.
#pragma once
#include "icet_map.h"

namespace icet_map_shape_rule {

constexpr int kWords = 9;          // S_x S_y S_z M_xx M_xy M_xz M_yy M_yz M_zz
constexpr int kSweeps = 6;         // cyclic Jacobi sweeps.  On the 624 cells of a noisy plane (tests/test_map_shape_model.py) the largest off-diagonal entry over the
                                   // largest eigenvalue is 7e-16 after 3 sweeps, 3e-64 after 4 and exactly 0 after 6

// k2 = ((double)cell 2^-16)^2: a unit of h, squared, in metres.
struct Consts { double k2; };
inline Consts make_consts(float cell) {
    Consts c;
    const double k = (double)cell * (1.0 / 65536.0);
    c.k2 = k * k;
    return c;
}

// What one kept row adds: S[a] = h_a, M = h_x h_x, h_x h_y, h_x h_z, h_y h_y, h_y h_z, h_z h_z (each below 2^32).
ICET_CLOSURE_HD inline void row_moments(const uint32_t q[3], uint32_t S[3], uint32_t M[6]) {
    const uint32_t h0 = q[0] >> 16, h1 = q[1] >> 16, h2 = q[2] >> 16;
    S[0] = h0; S[1] = h1; S[2] = h2;
    M[0] = h0 * h0; M[1] = h0 * h1; M[2] = h0 * h2; M[3] = h1 * h1; M[4] = h1 * h2; M[5] = h2 * h2;
}

// The covariance of a cell of count n >= 1 with the words w, in the world frame: C = xx, xy, xz, yy, yz, zz.  No quantisation correction.
ICET_CLOSURE_HD inline void cov(const Consts& k, int64_t n, const uint64_t w[kWords], double C[6]) {
    ICET_CLOSURE_NO_CONTRACT
    const double nd = (double)n;
    double m[3];
    for (int a = 0; a < 3; a++) m[a] = (double)w[a] / nd;
    int j = 0;
    for (int a = 0; a < 3; a++) {
        for (int b = a; b < 3; b++, j++) {
            const double e = (double)w[3 + j] / nd;
            const double mm = m[a] * m[b];
            const double d = e - mm;
            C[j] = d * k.k2;
        }
    }
}

// One rotation of the pair (p, q), r the third index: A <- J^T A J, V <- V J.
ICET_CLOSURE_HD inline void rotate(double A[3][3], double V[3][3], int p, int q, int r) {
    ICET_CLOSURE_NO_CONTRACT
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double diff = A[q][q] - A[p][p];
    const double den = 2.0 * apq;
    const double theta = diff / den;                 // may be infinite: t = 0 then
    const double tt = theta * theta;
    const double root = sqrt(tt + 1.0);
    const double sum = fabs(theta) + root;
    const double inv = 1.0 / sum;
    const double t = theta < 0.0 ? -inv : inv;
    const double t2 = t * t;
    const double c = 1.0 / sqrt(t2 + 1.0);
    const double s = t * c;
    const double ta = t * apq;
    A[p][p] = A[p][p] - ta;
    A[q][q] = A[q][q] + ta;
    A[p][q] = 0.0; A[q][p] = 0.0;
    const double arp = A[r][p], arq = A[r][q];
    const double cp = c * arp, sq = s * arq, sp = s * arp, cq = c * arq;
    const double np_ = cp - sq, nq_ = sp + cq;
    A[r][p] = np_; A[p][r] = np_;
    A[r][q] = nq_; A[q][r] = nq_;
    for (int i = 0; i < 3; i++) {
        const double vp = V[i][p], vq = V[i][q];
        const double a0 = c * vp, a1 = s * vq, b0 = s * vp, b1 = c * vq;
        V[i][p] = a0 - a1;
        V[i][q] = b0 + b1;
    }
}

// The eigenvalues of C ascending, as computed (a tiny negative one stays negative), and the eigenvector of the smallest: ties go to the lowest column of V; the
// sign makes the float32 component of largest magnitude positive, the lowest axis winning a tie.  C = 0 gives zeros and (1, 0, 0).
ICET_CLOSURE_HD inline void eigen(const double C[6], float evals[3], float normal[3]) {
    ICET_CLOSURE_NO_CONTRACT
    double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < kSweeps; sweep++) {
        rotate(A, V, 0, 1, 2);
        rotate(A, V, 0, 2, 1);
        rotate(A, V, 1, 2, 0);
    }
    const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
    // a stable sort of three: (value, column) pairs, a later column moves in front of an earlier one only when it is smaller
    double e0 = d0, e1 = d1, e2 = d2; int i0 = 0;                      // i0: the column of the smallest
    if (e1 < e0) { const double x = e0; e0 = e1; e1 = x; i0 = 1; }
    if (e2 < e1) {
        const double x = e1; e1 = e2; e2 = x;
        if (e1 < e0) { const double y = e0; e0 = e1; e1 = y; i0 = 2; }
    }
    evals[0] = (float)e0; evals[1] = (float)e1; evals[2] = (float)e2;
    float v[3];
    for (int i = 0; i < 3; i++) v[i] = (float)(i0 == 0 ? V[i][0] : i0 == 1 ? V[i][1] : V[i][2]);
    int j = 0;
    if (fabsf(v[1]) > fabsf(v[0])) j = 1;
    if (fabsf(v[2]) > fabsf(j == 0 ? v[0] : v[1])) j = 2;
    const float lead = j == 0 ? v[0] : j == 1 ? v[1] : v[2];
    const bool flip = lead < 0.f;
    for (int i = 0; i < 3; i++) normal[i] = flip ? -v[i] : v[i];
}

}  // namespace icet_map_shape_rule
