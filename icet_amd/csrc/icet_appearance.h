// icet_amd/csrc/icet_appearance.h -- the RULE of the keyframe store's appearance search (include/icet_hip.h icet_keyframe_store_close_appearance_device;
// DESIGN.md section 17), in one place: the cell and the height code of a point, the column weight, the distance of two descriptors at a column shift, the
// eligibility test and the start pose of a shift.  HIP-free C++: the kernels of icet_appearance.hip, the host code of icet_store.hip and the CPU test
// (tests/cpp/test_appearance.cpp) compile this text.
//
// DESCRIPTOR: rings x sectors bytes D[ring][sector], the largest height code of the points of a cell (0: empty), in the sensor frame; a rotation of the
// sensor about z shifts its columns.  A maximum does not depend on the order of the points, so the descriptor does not depend on the launch shape.
// ARITHMETIC: float32, one rounding per operation, nothing contracted; atan2, the weight and the mean in double, rounded to float32 once (the shared
// arithmetic rule).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "icet_closure.h"

namespace icet_appearance_rule {

using icet_closure_rule::kNoKey;

constexpr double kTwoPi = 6.283185307179586;       // 2 pi, correctly rounded

// What enable fixes.  kr = rings / rho_max, ka = sectors / 2 pi, kz = 254 / (z_hi - z_lo): each taken in double and rounded to float32 once, by the host.
struct Consts {
    int32_t A, Rn;
    float z_lo, z_hi, kr, ka, kz;
};

inline bool params_ok(int32_t sectors, int32_t rings, float rho_max, float z_lo, float z_hi) {
    if (sectors < 8 || sectors > 360 || (sectors & 1)) return false;
    if (rings < 1 || rings > 64) return false;
    if (!(rho_max > 0.f) || !isfinite(rho_max) || !isfinite(z_lo) || !isfinite(z_hi) || !(z_hi > z_lo)) return false;
    return true;
}
inline Consts make_consts(int32_t sectors, int32_t rings, float rho_max, float z_lo, float z_hi) {
    Consts c;
    c.A = sectors; c.Rn = rings; c.z_lo = z_lo; c.z_hi = z_hi;
    c.kr = (float)((double)rings / (double)rho_max);
    c.ka = (float)((double)sectors / kTwoPi);
    c.kz = (float)(254.0 / ((double)z_hi - (double)z_lo));
    return c;
}

// The cell (ring, sector) and the height code q (1 .. 255) of a point; false: the point does not count (not finite, an exact-zero row, beyond rho_max).
ICET_CLOSURE_HD inline bool cell_of(const Consts& c, float x, float y, float z, int& ring, int& sector, int& q) {
    ICET_CLOSURE_NO_CONTRACT
    const float xx = x * x, yy = y * y;
    const float rho2 = xx + yy;
    if (!(fabsf(x) <= 3.402823466e+38f) || !(fabsf(y) <= 3.402823466e+38f) || !(fabsf(z) <= 3.402823466e+38f)) return false;
    if (!(rho2 > 0.f)) return false;
    const float rho = sqrtf(rho2);
    const float t = rho * c.kr;
    if (!(t < (float)c.Rn)) return false;
    ring = (int)floorf(t);
    const float az = (float)atan2((double)y, (double)x);
    const float ua = az * c.ka;
    const float u = ua + (float)(c.A / 2);
    int s = (int)floorf(u);
    if (s >= c.A) s -= c.A;
    if (s < 0) s = 0;
    sector = s;
    const float zc = fminf(fmaxf(z, c.z_lo), c.z_hi);
    const float zd = zc - c.z_lo;
    const float zq = zd * c.kz;
    int h = 1 + (int)floorf(zq);
    q = h < 1 ? 1 : (h > 255 ? 255 : h);
    return true;
}

// The weight of a column of energy n = sum_r D[r][j]^2 (an integer): 1 / sqrt(n) in double, rounded once; an empty column weighs 0.
ICET_CLOSURE_HD inline float column_weight(uint32_t n) { return n ? (float)(1.0 / sqrt((double)n)) : 0.f; }

ICET_CLOSURE_HD inline int min_columns(int A) { return (A + 3) / 4; }

// One column's term: fl(fl((float)G wq) wc), G the exact integer product of the two columns.
ICET_CLOSURE_HD inline float column_term(uint32_t G, float wq, float wc) {
    ICET_CLOSURE_NO_CONTRACT
    const float a = (float)G * wq;
    return a * wc;
}
// The distance of a shift from the double sum of its valid columns' terms (ascending j) and their number m.
ICET_CLOSURE_HD inline float shift_distance(double sum, int m, int A) {
    ICET_CLOSURE_NO_CONTRACT
    if (m < min_columns(A)) return INFINITY;
    const double mean = sum / (double)m;
    const float d = (float)(1.0 - mean);
    return d < 0.f ? 0.f : d;
}
// (bits(d), shift): its minimum over the shifts is the slot's distance, ties to the lowest shift.  d is not negative and never NaN.
ICET_CLOSURE_HD inline uint64_t shift_key(float d, int shift) { return icet_closure_rule::make_key(d, shift); }

// The whole distance on the host: descriptors row-major D[ring][sector], weights per column.  Returns the distance; *shift gets the best shift.
inline float distance(const uint8_t* Dq, const float* wq, const uint8_t* Dc, const float* wc, int A, int Rn, int* shift) {
    uint64_t best = kNoKey;
    for (int s = 0; s < A; s++) {
        double sum = 0.0; int m = 0;
        for (int j = 0; j < A; j++) {
            const int jj = j + s >= A ? j + s - A : j + s;
            if (!(wq[j] > 0.f && wc[jj] > 0.f)) continue;
            uint32_t G = 0;
            for (int r = 0; r < Rn; r++) G += (uint32_t)Dq[r * A + j] * (uint32_t)Dc[r * A + jj];
            sum += (double)column_term(G, wq[j], wc[jj]);
            m++;
        }
        const uint64_t k = shift_key(shift_distance(sum, m, A), s);
        if (k < best) best = k;
    }
    if (shift) *shift = (int)(uint32_t)best;
    return icet_closure_rule::key_d2(best);
}

// The key of a slot whose distance is d, or kNoKey when it is not eligible (the caller has checked "occupied, has a descriptor").  A NaN fails d <= max.
ICET_CLOSURE_HD inline uint64_t candidate_key(float d, float max_distance, int64_t q_stamp, int64_t s_stamp, int64_t min_stamp_gap, int32_t slot) {
    if (!(d <= max_distance)) return kNoKey;
    if (!icet_closure_rule::stamp_gap_ok(q_stamp, s_stamp, min_stamp_gap)) return kNoKey;
    return icet_closure_rule::make_key(d, slot);
}

// The yaw of the start pose of shift s: live sector j corresponds to keyframe sector j + s, psi of R(X0) = R_q^T R_j.
ICET_CLOSURE_HD inline float shift_yaw(int s, int A) {
    ICET_CLOSURE_NO_CONTRACT
    const double step = kTwoPi / (double)A;
    double a = (double)s * step;
    if (a > 3.141592653589793) a = a - kTwoPi;
    return (float)a;
}

}  // namespace icet_appearance_rule
