// icet_amd/csrc/icet_node_tail.h -- the scalars of a frame's tail (icet_nodes.hip frame_tail): the frame's rotation from its Euler angles, the inverse the row passes
// apply, the pose chain and the quaternion a node publishes.  Pure C++ (no HIP, no state), so that the degenerate inputs can run under a host sanitizer in a program of
// their own (tests/cpp/test_node_tail.cpp) and the library's one compiled copy (node_tail_scalars in icet_nodes.hip) can be held to a model (tests/node_tail_model.py).
// Every expression is written in the order it is evaluated in; nothing here may be contracted or reassociated (the host build has no fused multiply-add to contract into).
#pragma once
#include <cmath>
#include <cstring>
#include <utility>

namespace icet_node_tail {

// utils::R (src/utils.cpp:144-152) in host float arithmetic, as the nodes evaluate it (odometry.cpp:85)
inline void euler_R_host(float phi, float theta, float psi, float* R) {
    const float cph = std::cos(phi), sph = std::sin(phi), cth = std::cos(theta), sth = std::sin(theta), cps = std::cos(psi), sps = std::sin(psi);
    R[0] = cth * cps;  R[1] = sps * cph + sph * sth * cps;  R[2] = sph * sps - sth * cph * cps;
    R[3] = -sps * cth; R[4] = cph * cps - sph * sth * sps;  R[5] = sph * cps + sth * sps * cph;
    R[6] = sth;        R[7] = -sph * cth;                   R[8] = cph * cth;
}

// MatrixXf::inverse() of a dynamic matrix goes through PartialPivLU (Eigen/src/LU/InverseImpl.h): LU with row pivoting,
// then the two triangular solves against the permuted identity.
inline void inverse3_lu(const float* A, float* inv) {
    float lu[9]; std::memcpy(lu, A, sizeof(lu));
    int perm[3] = {0, 1, 2};
    for (int k = 0; k < 3; k++) {
        int piv = k; float best = std::fabs(lu[k * 3 + k]);
        for (int r = k + 1; r < 3; r++) if (std::fabs(lu[r * 3 + k]) > best) { best = std::fabs(lu[r * 3 + k]); piv = r; }
        if (piv != k) { for (int c = 0; c < 3; c++) std::swap(lu[k * 3 + c], lu[piv * 3 + c]); std::swap(perm[k], perm[piv]); }
        if (lu[k * 3 + k] == 0.f) continue;
        for (int r = k + 1; r < 3; r++) {
            lu[r * 3 + k] /= lu[k * 3 + k];
            for (int c = k + 1; c < 3; c++) lu[r * 3 + c] -= lu[r * 3 + k] * lu[k * 3 + c];
        }
    }
    for (int col = 0; col < 3; col++) {
        float b[3];
        for (int r = 0; r < 3; r++) b[r] = (perm[r] == col) ? 1.f : 0.f;
        for (int r = 1; r < 3; r++) for (int c = 0; c < r; c++) b[r] -= lu[r * 3 + c] * b[c];
        for (int r = 2; r >= 0; r--) { for (int c = r + 1; c < 3; c++) b[r] -= lu[r * 3 + c] * b[c]; b[r] /= lu[r * 3 + r]; }
        for (int r = 0; r < 3; r++) inv[r * 3 + col] = b[r];
    }
}

// X_homo = X_homo * X_homo_i (odometry.cpp:91-98): P = pose * [R t; 0 1], 4 x 4 row-major, each entry accumulated over k = 0 .. 3 in order
inline void pose_chain(const float* pose, const float* R, const float* t, float* P) {
    const float Hi[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1};
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { float acc = 0.f; for (int k = 0; k < 4; k++) acc += pose[r * 4 + k] * Hi[k * 4 + c]; P[r * 4 + c] = acc; }
}

// Eigen::Quaternionf(Matrix3f) (Eigen/src/Geometry/Quaternion.h, Shoemake's method); q = x, y, z, w
inline void quat_of(const float* P /* 4x4 row-major */, float q[4]) {
    const float m00 = P[0], m01 = P[1], m02 = P[2], m10 = P[4], m11 = P[5], m12 = P[6], m20 = P[8], m21 = P[9], m22 = P[10];
    const float m[3][3] = {{m00, m01, m02}, {m10, m11, m12}, {m20, m21, m22}};
    float t = m00 + m11 + m22;
    if (t > 0.f) {
        t = std::sqrt(t + 1.0f); q[3] = 0.5f * t; t = 0.5f / t;
        q[0] = (m21 - m12) * t; q[1] = (m02 - m20) * t; q[2] = (m10 - m01) * t;
    } else {
        int i = 0;
        if (m11 > m00) i = 1;
        if (m22 > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0f);
        q[i] = 0.5f * t; t = 0.5f / t;
        q[3] = (m[k][j] - m[j][k]) * t; q[j] = (m[j][i] + m[i][j]) * t; q[k] = (m[k][i] + m[i][k]) * t;
    }
}

// The four steps of a frame's tail in the order frame_tail needs them: R from X[3..5], its inverse, P = pose_in * [R X[0..2]; 0 1] and P's quaternion.
// P may not alias pose_in.
inline void tail_scalars(const float X[6], const float pose_in[16], float R[9], float Rinv[9], float P[16], float quat[4]) {
    euler_R_host(X[3], X[4], X[5], R);
    inverse3_lu(R, Rinv);
    pose_chain(pose_in, R, X, P);
    quat_of(P, quat);
}

}  // namespace icet_node_tail
