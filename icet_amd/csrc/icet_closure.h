// icet_amd/csrc/icet_closure.h -- the RULE of the keyframe store's loop-closure query (include/icet_hip.h icet_keyframe_store_close_device; DESIGN.md
// section 16), in one place: the candidate distance and its sort key, the eligibility test, the start pose X0 of a registration from two stored poses, and
// the step of a pose chain from a registration result.  HIP-free C++: the kernels of icet_closure.hip, the host helper icet_pose_step_from_x and the CPU test
// (tests/cpp/test_closure.cpp) compile this text.
//
// POSE: the physical sensor pose in a world frame, 4 x 4 row-major float32 T = [R | t; 0 0 0 1], p_world = R p + t.  The solver's model is
// q = R(X)^T (p + X_t) (src/icet.cpp:375-378: p a scan-2 point, q the same point in the keyframe's frame), so for a keyframe pose (R_j, t_j) and a live pose
// (R_q, t_q):  R(X) = R_q^T R_j  and  X_t = R_q^T (t_q - t_j).  The rotation of a stored pose is taken as orthonormal (its inverse is its transpose).
// ARITHMETIC: the distance in float32, one rounding per operation, nothing contracted; the start pose in double from the float32 inputs, sums left to right,
// nothing contracted, each of the six values rounded to float32 once (the shared arithmetic rule).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ICET_CLOSURE_HD __host__ __device__
#else
#define ICET_CLOSURE_HD
#endif
// (g++ builds this header with -ffp-contract=off; clang -- the device compiler, whose default for HIP is to contract -- is told per function)
#if defined(__clang__)
#define ICET_CLOSURE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ICET_CLOSURE_NO_CONTRACT
#endif

namespace icet_closure_rule {

constexpr uint64_t kNoKey = ~(uint64_t)0;      // "no candidate": above every key

// d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), dx = fl(q.x - s.x)
ICET_CLOSURE_HD inline float dist2(float qx, float qy, float qz, float sx, float sy, float sz) {
    ICET_CLOSURE_NO_CONTRACT
    const float dx = qx - sx, dy = qy - sy, dz = qz - sz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float s = xx + yy;
    return s + zz;
}

// |a - b| >= gap in 64-bit integers (the difference of two int64 fits a uint64); gap <= 0: always
ICET_CLOSURE_HD inline bool stamp_gap_ok(int64_t a, int64_t b, int64_t gap) {
    if (gap <= 0) return true;
    const uint64_t d = a >= b ? (uint64_t)a - (uint64_t)b : (uint64_t)b - (uint64_t)a;
    return d >= (uint64_t)gap;
}

// The order of the candidates: (d2, slot) ascending.  d2 is not negative, so its bit pattern is monotone; the keys of distinct slots are distinct.
ICET_CLOSURE_HD inline uint64_t make_key(float d2, int32_t slot) {
    uint32_t b; memcpy(&b, &d2, 4);
    return ((uint64_t)b << 32) | (uint32_t)slot;
}
ICET_CLOSURE_HD inline int32_t key_slot(uint64_t key) { return key == kNoKey ? -1 : (int32_t)(uint32_t)key; }
ICET_CLOSURE_HD inline float key_d2(uint64_t key) { const uint32_t b = (uint32_t)(key >> 32); float f; memcpy(&f, &b, 4); return f; }

// The key of slot `slot` for a query, or kNoKey when the slot is not eligible: a slot without a pose holds NaN translations, and a NaN anywhere
// fails d2 <= r2.  r2 = fl(radius x radius).
ICET_CLOSURE_HD inline uint64_t candidate_key(float qx, float qy, float qz, int64_t q_stamp, float sx, float sy, float sz, int64_t s_stamp,
                                              float r2, int64_t min_stamp_gap, int32_t slot) {
    const float d2 = dist2(qx, qy, qz, sx, sy, sz);
    if (!(d2 <= r2)) return kNoKey;
    if (!stamp_gap_ok(q_stamp, s_stamp, min_stamp_gap)) return kNoKey;
    return make_key(d2, slot);
}
ICET_CLOSURE_HD inline float radius2(float radius) {
    ICET_CLOSURE_NO_CONTRACT
    const float r2 = radius * radius;
    return r2;
}

// Euler angles of a rotation written as euler_R_host writes it (icet_nodes.hip; src/utils.cpp R = Rx Ry Rz of the reference): row-major R, double.
ICET_CLOSURE_HD inline void euler_of_R(const double R[9], double ang[3]) {
    const double s = R[6] > 1.0 ? 1.0 : (R[6] < -1.0 ? -1.0 : R[6]);
    ang[0] = atan2(-R[7], R[8]);           // phi
    ang[1] = asin(s);                      // theta
    ang[2] = atan2(-R[3], R[0]);           // psi
}
ICET_CLOSURE_HD inline void euler_R(double phi, double theta, double psi, double R[9]) {
    ICET_CLOSURE_NO_CONTRACT
    const double cph = cos(phi), sph = sin(phi), cth = cos(theta), sth = sin(theta), cps = cos(psi), sps = sin(psi);
    R[0] = cth * cps;  R[1] = sps * cph + sph * sth * cps;  R[2] = sph * sps - sth * cph * cps;
    R[3] = -sps * cth; R[4] = cph * cps - sph * sth * sps;  R[5] = sph * cps + sth * sps * cph;
    R[6] = sth;        R[7] = -sph * cth;                   R[8] = cph * cth;
}

// X0 of the registration of a live scan at pose (Rq, tq) against a keyframe at pose (Rj, tj): rotations row-major 3 x 3.
ICET_CLOSURE_HD inline void start_pose(const float Rq[9], const float tq[3], const float Rj[9], const float tj[3], float x0[6]) {
    ICET_CLOSURE_NO_CONTRACT
    double RX[9], d[3];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const double m0 = (double)Rq[0 + a] * (double)Rj[0 + b], m1 = (double)Rq[3 + a] * (double)Rj[3 + b], m2 = (double)Rq[6 + a] * (double)Rj[6 + b];
            const double s = m0 + m1;
            RX[3 * a + b] = s + m2;
        }
    for (int c = 0; c < 3; c++) d[c] = (double)tq[c] - (double)tj[c];
    for (int a = 0; a < 3; a++) {
        const double m0 = (double)Rq[0 + a] * d[0], m1 = (double)Rq[3 + a] * d[1], m2 = (double)Rq[6 + a] * d[2];
        const double s = m0 + m1;
        x0[a] = (float)(s + m2);
    }
    double ang[3];
    euler_of_R(RX, ang);
    for (int k = 0; k < 3; k++) x0[3 + k] = (float)ang[k];
}
// The same for 4 x 4 row-major poses.
ICET_CLOSURE_HD inline void start_pose_T(const float Tq[16], const float Tj[16], float x0[6]) {
    float Rq[9], Rj[9], tq[3], tj[3];
    for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) { Rq[3 * a + b] = Tq[4 * a + b]; Rj[3 * a + b] = Tj[4 * a + b]; } tq[a] = Tq[4 * a + 3]; tj[a] = Tj[4 * a + 3]; }
    start_pose(Rq, tq, Rj, tj, x0);
}

// One step of a pose chain from a registration result X (keyframe = the previous frame): T = [R(X)^T | R(X)^T X_t], T_world,k = T_world,k-1 * T.
// In double from the float32 X, every entry rounded to float32 once.
ICET_CLOSURE_HD inline void pose_step_from_X(const float X[6], float T[16]) {
    ICET_CLOSURE_NO_CONTRACT
    double R[9];
    euler_R((double)X[3], (double)X[4], (double)X[5], R);
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) T[4 * a + b] = (float)R[3 * b + a];
        const double m0 = R[0 + a] * (double)X[0], m1 = R[3 + a] * (double)X[1], m2 = R[6 + a] * (double)X[2];
        const double s = m0 + m1;
        T[4 * a + 3] = (float)(s + m2);
    }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

}  // namespace icet_closure_rule
