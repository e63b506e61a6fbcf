// icet_amd/csrc/icet_deskew.h -- the RULE of the deskewer (include/icet_hip.h icet_deskew_*), in one place: what the motion of a sweep does
// to one row of a scan -- its class, its time, its coordinates in the frame of the reference instant --, and the two maps between a pose and a twist.
// HIP-free C++: the kernels and the host code of icet_deskew.hip and the CPU test (tests/cpp/test_deskew_rule.cpp) compile this text.
//
// MOTION: a twist xi = (rho, phi), six doubles.  T(s) = exp(s xi) = [exp(s phi^) | V(s phi) s rho] is the sensor's pose at sweep fraction s in the sensor frame
// at s = 0 (the store's POSE convention, icet_closure.h: p_0 = R p_s + t).  exp is a one-parameter group, so a row taken at s is carried into the frame at
// s_ref by p' = exp((s - s_ref) xi) p, and nothing else is needed.
// ARITHMETIC of a row: IEEE double, one rounding per operation, nothing contracted, no transcendental: sin t / t, (1 - cos t) / t^2 and (t - sin t) / t^3 are
// polynomials of degree 9 in u = t^2 <= 1 (truncation below 1 / 21!), so a NumPy model reproduces every bit.  The two pose <-> twist maps use libm and agree
// with another math library to its last bits only.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "icet_closure.h"

namespace icet_deskew_rule {

enum RowClass { kRowMoved = 0, kRowZero = 1, kRowNonfinite = 2, kRowBadTime = 3, kRowOutOfRange = 4, kRowClasses = 5 };
enum TimeMode { kTimeArray = 0, kTimeColumnFast = 1, kTimeColumnSlow = 2 };      // ICET_DESKEW_TIME_*

// What a scan's rows share.
struct Motion {
    double t0, inv_span, s_ref;
    double xi[6];                  // rho | phi
    int32_t mode, period;
};

inline bool mode_ok(int32_t mode, int32_t period) { return mode == kTimeArray || ((mode == kTimeColumnFast || mode == kTimeColumnSlow) && period > 0); }
// A scan's shape: n >= 0, both leading dimensions >= n and below 2^30.
inline bool shape_ok(int64_t n, int64_t ld, int64_t ld_out) {
    const int64_t lim = (int64_t)1 << 30;
    return n >= 0 && ld >= n && ld_out >= n && ld < lim && ld_out < lim;
}
// dst against src, as byte ranges of three columns each: 0 apart, 1 identical (same pointer, same ld: the in-place form), 2 overlapping otherwise.
inline int overlap(const float* src, int64_t ld, const float* dst, int64_t ld_out, int64_t n) {
    if (n <= 0) return 0;
    if (src == dst && ld == ld_out) return 1;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(src), a1 = a0 + 4 * (uintptr_t)(2 * ld + n);
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(dst), b1 = b0 + 4 * (uintptr_t)(2 * ld_out + n);
    return (a0 < b1 && b0 < a1) ? 2 : 0;
}

// The three series in u = theta^2, by Horner from the highest coefficient: the doubles nearest to (-1)^k / (2k + 1)!, / (2k + 2)!, / (2k + 3)!, k = 9 .. 0
// (every factorial up to 21! is a double, so each quotient is rounded once).
ICET_CLOSURE_HD inline double series_a(double u) {      // sin t / t
    ICET_CLOSURE_NO_CONTRACT
    double r = -1.0 / 121645100408832000.0;
    r = r * u + 1.0 / 355687428096000.0;
    r = r * u + -1.0 / 1307674368000.0;
    r = r * u + 1.0 / 6227020800.0;
    r = r * u + -1.0 / 39916800.0;
    r = r * u + 1.0 / 362880.0;
    r = r * u + -1.0 / 5040.0;
    r = r * u + 1.0 / 120.0;
    r = r * u + -1.0 / 6.0;
    r = r * u + 1.0;
    return r;
}
ICET_CLOSURE_HD inline double series_b(double u) {      // (1 - cos t) / t^2
    ICET_CLOSURE_NO_CONTRACT
    double r = -1.0 / 2432902008176640000.0;
    r = r * u + 1.0 / 6402373705728000.0;
    r = r * u + -1.0 / 20922789888000.0;
    r = r * u + 1.0 / 87178291200.0;
    r = r * u + -1.0 / 479001600.0;
    r = r * u + 1.0 / 3628800.0;
    r = r * u + -1.0 / 40320.0;
    r = r * u + 1.0 / 720.0;
    r = r * u + -1.0 / 24.0;
    r = r * u + 1.0 / 2.0;
    return r;
}
ICET_CLOSURE_HD inline double series_c(double u) {      // (t - sin t) / t^3
    ICET_CLOSURE_NO_CONTRACT
    double r = -1.0 / 51090942171709440000.0;
    r = r * u + 1.0 / 121645100408832000.0;
    r = r * u + -1.0 / 355687428096000.0;
    r = r * u + 1.0 / 1307674368000.0;
    r = r * u + -1.0 / 6227020800.0;
    r = r * u + 1.0 / 39916800.0;
    r = r * u + -1.0 / 362880.0;
    r = r * u + 1.0 / 5040.0;
    r = r * u + -1.0 / 120.0;
    r = r * u + 1.0 / 6.0;
    return r;
}

ICET_CLOSURE_HD inline void cross3(const double a[3], const double b[3], double c[3]) {
    ICET_CLOSURE_NO_CONTRACT
    const double yz = a[1] * b[2], zy = a[2] * b[1], zx = a[2] * b[0], xz = a[0] * b[2], xy = a[0] * b[1], yx = a[1] * b[0];
    c[0] = yz - zy; c[1] = zx - xz; c[2] = xy - yx;
}

// Row i of a scan: (x, y, z), and in array mode its time tval.  Returns the class; out[] is written for a moved row only -- every other class keeps the row's bits,
// which is the caller's copy.
ICET_CLOSURE_HD inline int deskew_row(const Motion& m, int32_t i, float tval, float x, float y, float z, float out[3]) {
    ICET_CLOSURE_NO_CONTRACT
    if (!(fabsf(x) <= 3.402823466e+38f) || !(fabsf(y) <= 3.402823466e+38f) || !(fabsf(z) <= 3.402823466e+38f)) return kRowNonfinite;
    if (x == 0.f && y == 0.f && z == 0.f) return kRowZero;
    double tau;
    if (m.mode == kTimeArray) {
        tau = (double)tval;
        if (!(fabs(tau) <= 1.7976931348623157e308)) return kRowBadTime;
    } else {
        const uint32_t c = m.mode == kTimeColumnFast ? (uint32_t)i % (uint32_t)m.period : (uint32_t)i / (uint32_t)m.period;      // (0 <= i < 2^30, period > 0)
        tau = (double)c + 0.5;
    }
    const double dt = tau - m.t0;
    const double s = dt * m.inv_span;
    const double d = s - m.s_ref;
    double th[3], sg[3];
    for (int a = 0; a < 3; a++) th[a] = d * m.xi[3 + a];
    const double txx = th[0] * th[0], tyy = th[1] * th[1], tzz = th[2] * th[2];
    const double uxy = txx + tyy;
    const double u = uxy + tzz;
    if (!(u <= 1.0)) return kRowOutOfRange;
    const double A = series_a(u), B = series_b(u), C = series_c(u);
    for (int a = 0; a < 3; a++) sg[a] = d * m.xi[a];
    const double p[3] = {(double)x, (double)y, (double)z};
    double c1[3], c2[3], r1[3], r2[3];
    cross3(th, p, c1); cross3(th, c1, c2); cross3(th, sg, r1); cross3(th, r1, r2);
    for (int a = 0; a < 3; a++) {
        const double ac1 = A * c1[a], bc2 = B * c2[a], br1 = B * r1[a], cr2 = C * r2[a];
        const double rot1 = p[a] + ac1;
        const double rot = rot1 + bc2;
        const double tr1 = sg[a] + br1;
        const double tr = tr1 + cr2;
        const double o = rot + tr;
        out[a] = (float)o;
    }
    return kRowMoved;
}

// ---- pose <-> twist, double with libm.  T: 4 x 4 row-major, [R | t; 0 0 0 1] -------------------------------------------------------------------------------

// sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3 for any u = t^2 >= 0: the series up to u = 1, the closed forms above.
ICET_CLOSURE_HD inline void abc_of(double u, double& A, double& B, double& C) {
    if (u <= 1.0) { A = series_a(u); B = series_b(u); C = series_c(u); return; }
    const double t = sqrt(u), sn = sin(t), cs = cos(t);
    A = sn / t; B = (1.0 - cs) / u; C = (t - sn) / (u * t);
}

// T = exp(s xi).
ICET_CLOSURE_HD inline void pose_from_twist(const double xi[6], double s, double T[16]) {
    double th[3], sg[3];
    for (int a = 0; a < 3; a++) { sg[a] = s * xi[a]; th[a] = s * xi[3 + a]; }
    const double u = (th[0] * th[0] + th[1] * th[1]) + th[2] * th[2];
    double A, B, C;
    abc_of(u, A, B, C);
    for (int j = 0; j < 3; j++) {                                      // column j of R: e_j + A th x e_j + B th x (th x e_j)
        double e[3] = {0.0, 0.0, 0.0}, c1[3], c2[3];
        e[j] = 1.0;
        cross3(th, e, c1); cross3(th, c1, c2);
        for (int a = 0; a < 3; a++) T[4 * a + j] = (e[a] + A * c1[a]) + B * c2[a];
    }
    double r1[3], r2[3];
    cross3(th, sg, r1); cross3(th, r1, r2);
    for (int a = 0; a < 3; a++) T[4 * a + 3] = (sg[a] + B * r1[a]) + C * r2[a];
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

// xi = log(T), for rotation angles below 3 rad.  The angle is atan2(|w|, (tr - 1) / 2), w the axial vector of (R - R^T) / 2, which stays accurate as the angle
// goes to 0 (acos of a cosine near 1 does not); rho solves V(phi) rho = t by the adjugate.  A rotation that is exactly symmetric gives phi = 0 exactly.
ICET_CLOSURE_HD inline void twist_from_pose(const double T[16], double xi[6]) {
    const double w[3] = {0.5 * (T[9] - T[6]), 0.5 * (T[2] - T[8]), 0.5 * (T[4] - T[1])};
    const double sn = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    const double cs = 0.5 * (((T[0] + T[5]) + T[10]) - 1.0);
    const double t = atan2(sn, cs);
    const double f = sn > 1e-5 ? t / sn : 1.0 + t * t * (1.0 / 6.0 + t * t * (7.0 / 360.0));      // t / sin t
    double th[3];
    for (int a = 0; a < 3; a++) th[a] = f * w[a];
    const double u = (th[0] * th[0] + th[1] * th[1]) + th[2] * th[2];
    double A, B, C;
    abc_of(u, A, B, C);
    double V[9];
    for (int j = 0; j < 3; j++) {
        double e[3] = {0.0, 0.0, 0.0}, c1[3], c2[3];
        e[j] = 1.0;
        cross3(th, e, c1); cross3(th, c1, c2);
        for (int a = 0; a < 3; a++) V[3 * a + j] = (e[a] + B * c1[a]) + C * c2[a];
    }
    const double tv[3] = {T[3], T[7], T[11]};
    const double c00 = V[4] * V[8] - V[5] * V[7], c01 = V[5] * V[6] - V[3] * V[8], c02 = V[3] * V[7] - V[4] * V[6];
    const double det = (V[0] * c00 + V[1] * c01) + V[2] * c02;
    const double inv[9] = {c00, V[2] * V[7] - V[1] * V[8], V[1] * V[5] - V[2] * V[4],
                           c01, V[0] * V[8] - V[2] * V[6], V[2] * V[3] - V[0] * V[5],
                           c02, V[1] * V[6] - V[0] * V[7], V[0] * V[4] - V[1] * V[3]};
    for (int a = 0; a < 3; a++) xi[a] = ((inv[3 * a] * tv[0] + inv[3 * a + 1] * tv[1]) + inv[3 * a + 2] * tv[2]) / det;
    for (int a = 0; a < 3; a++) xi[3 + a] = th[a];
}

// The motion between two consecutive float32 poses, as a twist: scale log(T0^-1 T1), the inverse of a pose taken as the transpose of its rotation (the store's
// and the map query's convention).  Identical poses give an exactly symmetric R0^T R0 and t = 0: the twist is exactly zero.
ICET_CLOSURE_HD inline void twist_between(const float* T0, const float* T1, double scale, double xi[6]) {
    double D[16];
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++)
            D[4 * a + b] = ((double)T0[a] * (double)T1[b] + (double)T0[4 + a] * (double)T1[4 + b]) + (double)T0[8 + a] * (double)T1[8 + b];
        const double d0 = (double)T1[3] - (double)T0[3], d1 = (double)T1[7] - (double)T0[7], d2 = (double)T1[11] - (double)T0[11];
        D[4 * a + 3] = ((double)T0[a] * d0 + (double)T0[4 + a] * d1) + (double)T0[8 + a] * d2;
    }
    D[12] = 0.0; D[13] = 0.0; D[14] = 0.0; D[15] = 1.0;
    twist_from_pose(D, xi);
    for (int a = 0; a < 6; a++) xi[a] = scale * xi[a];
}

}  // namespace icet_deskew_rule
