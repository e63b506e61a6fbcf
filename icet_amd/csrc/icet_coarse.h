// icet_amd/csrc/icet_coarse.h -- the RULE of the keyframe store's coarse alignment (include/icet_hip.h icet_keyframe_store_coarse_align_device; DESIGN.md
// section 18), in one place: the cell and the height code of a point, which cells span, the transform of a yaw hypothesis, the score of a shift, the order
// of the winners and the start pose of one.  HIP-free C++: the kernels of icet_coarse.hip, the host code of icet_store.hip and the CPU test
// (tests/cpp/test_coarse.cpp) compile this text.
//
// GRID: G rows (ix) of G / 32 words, bit iy & 31 of word iy >> 5; a bird's-eye bit per cell that holds vertical structure.  Everything between the cells and
// the winner is integers, and minima, maxima, ORs and the maximum of a key do not depend on order, so nothing depends on the launch shape.
// ARITHMETIC: float32, one rounding per operation, nothing contracted; the constants, the rotation of a hypothesis and the start pose in double, each value
// rounded to float32 once (the shared arithmetic rule).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "icet_closure.h"

namespace icet_coarse_rule {

constexpr double kPi = 3.141592653589793;
constexpr int kMaxWindow = 32, kMaxYaw = 8;

// What enable fixes.  kc = 1 / cell, kz = 254 / (z_hi - z_lo): in double, rounded to float32 once; span_codes = ceil(min_span (254 / (z_hi - z_lo))) in double.
struct Consts {
    int32_t G, W;                 // cells per side; words per row, G / 32
    int32_t span_codes;
    float z_lo, z_hi, kc, kz;
    float cell;
};

inline bool params_ok(int32_t cells, float cell, float z_lo, float z_hi, float min_span) {
    if (cells < 64 || cells > 512 || (cells & 31)) return false;
    if (!(cell > 0.f) || !isfinite(cell) || !isfinite(z_lo) || !isfinite(z_hi) || !(z_hi > z_lo) || !(min_span > 0.f) || !isfinite(min_span)) return false;
    return true;
}
inline Consts make_consts(int32_t cells, float cell, float z_lo, float z_hi, float min_span) {
    Consts c;
    c.G = cells; c.W = cells / 32; c.z_lo = z_lo; c.z_hi = z_hi; c.cell = cell;
    c.kc = (float)(1.0 / (double)cell);
    const double kz = 254.0 / ((double)z_hi - (double)z_lo);
    c.kz = (float)kz;
    const double sc = ceil((double)min_span * kz);
    c.span_codes = sc > 1.0e9 ? 1000000000 : (int32_t)sc;
    return c;
}

// The cell index of one coordinate: u = fl(fl(v kc) + G / 2); inside when u >= 0 and u < G (a NaN is outside), index floor(u).
ICET_CLOSURE_HD inline bool coord_cell(const Consts& c, float v, int& i) {
    ICET_CLOSURE_NO_CONTRACT
    const float s = v * c.kc;
    const float u = s + (float)(c.G / 2);
    if (!(u >= 0.f && u < (float)c.G)) return false;
    i = (int)floorf(u);
    return true;
}

// A point of a scan in the sensor frame: does it count, and its cell (ix, iy) and height code q.
ICET_CLOSURE_HD inline bool count_point(const Consts& c, float x, float y, float z, int& ix, int& iy, int& q) {
    ICET_CLOSURE_NO_CONTRACT
    const float xx = x * x, yy = y * y;
    const float rho2 = xx + yy;
    if (!(fabsf(x) <= 3.402823466e+38f) || !(fabsf(y) <= 3.402823466e+38f) || !(fabsf(z) <= 3.402823466e+38f)) return false;
    if (!(rho2 > 0.f)) return false;
    if (!coord_cell(c, x, ix) || !coord_cell(c, y, iy)) return false;
    const float zc = fminf(fmaxf(z, c.z_lo), c.z_hi);
    const float zd = zc - c.z_lo;
    const float zq = zd * c.kz;
    q = (int)floorf(zq);
    return true;
}

// A cell spans when the largest minus the smallest code of its counting points reaches span_codes.
ICET_CLOSURE_HD inline bool cell_spans(const Consts& c, int q_min, int q_max) { return q_max - q_min >= c.span_codes; }

// The hypotheses of a search: h = f (2 Y + 1) + (y + Y), y = -Y .. Y, f = 0 / 1 (1 only with half_turn).
ICET_CLOSURE_HD inline int n_hypotheses(int Y, int half_turn) { return (half_turn ? 2 : 1) * (2 * Y + 1); }
ICET_CLOSURE_HD inline void hypothesis_of(int h, int Y, int& y, int& f) { f = h / (2 * Y + 1); y = h % (2 * Y + 1) - Y; }

// R_h = R(X0) Rz(delta_h) in double, delta_h = (double)y yaw_step + f pi; Rz(delta) is the solver's R(0, 0, delta).  Row-major, sums left to right.
ICET_CLOSURE_HD inline void hypothesis_rotation(const float X0[6], int y, int f, float yaw_step, double Rh[9]) {
    ICET_CLOSURE_NO_CONTRACT
    double R0[9], Rz[9];
    const double dy = (double)y * (double)yaw_step, df = (double)f * kPi;
    const double delta = dy + df;
    icet_closure_rule::euler_R((double)X0[3], (double)X0[4], (double)X0[5], R0);
    icet_closure_rule::euler_R(0.0, 0.0, delta, Rz);
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const double m0 = R0[3 * a + 0] * Rz[0 + b], m1 = R0[3 * a + 1] * Rz[3 + b], m2 = R0[3 * a + 2] * Rz[6 + b];
            const double s = m0 + m1;
            Rh[3 * a + b] = s + m2;
        }
}
// The float32 transform of a hypothesis: m = the first two rows of M = R_h^T (m[0..2] the row of x', m[3..5] the row of y'), each entry rounded once.
ICET_CLOSURE_HD inline void hypothesis_rows(const double Rh[9], float m[6]) {
    for (int b = 0; b < 3; b++) { m[b] = (float)Rh[3 * b + 0]; m[3 + b] = (float)Rh[3 * b + 1]; }
}
// u = fl(p + X0_t); x' = fl(fl(fl(m0 ux) + fl(m1 uy)) + fl(m2 uz)), y' likewise with m3 .. m5.
ICET_CLOSURE_HD inline void transform_xy(const float m[6], const float t[3], float x, float y, float z, float& xo, float& yo) {
    ICET_CLOSURE_NO_CONTRACT
    const float ux = x + t[0], uy = y + t[1], uz = z + t[2];
    const float a0 = m[0] * ux, a1 = m[1] * uy, a2 = m[2] * uz;
    const float sa = a0 + a1;
    xo = sa + a2;
    const float b0 = m[3] * ux, b1 = m[4] * uy, b2 = m[5] * uz;
    const float sb = b0 + b1;
    yo = sb + b2;
}

// The order of the winners as ONE key whose maximum is the winner: largest score; then smallest a^2 + b^2; then smallest h, a, b.  0: "no shift at all".
ICET_CLOSURE_HD inline uint64_t shift_key(uint32_t score, int a, int b, int h) {
    const uint32_t r2 = (uint32_t)(a * a + b * b);                     // <= 2048
    const uint32_t low = ((4095u - r2) << 20) | ((63u - (uint32_t)h) << 14) | ((uint32_t)(kMaxWindow - a) << 7) | (uint32_t)(kMaxWindow - b);
    return ((uint64_t)score << 32) | low;
}
ICET_CLOSURE_HD inline void key_decode(uint64_t key, uint32_t& score, int& a, int& b, int& h) {
    score = (uint32_t)(key >> 32);
    const uint32_t low = (uint32_t)key;
    h = 63 - (int)((low >> 14) & 63u);
    a = kMaxWindow - (int)((low >> 7) & 127u);
    b = kMaxWindow - (int)(low & 127u);
}
// The word of reserved1[1] of a closure record: h | (a + 32) << 8 | (b + 32) << 16.
ICET_CLOSURE_HD inline int32_t shift_code(int a, int b, int h) { return (int32_t)((uint32_t)h | ((uint32_t)(a + kMaxWindow) << 8) | ((uint32_t)(b + kMaxWindow) << 16)); }

// The start pose of the winner (a, b) of hypothesis R_h: R(X) = R_h, X_t = X0_t + R_h d, d = ((double)a cell, (double)b cell, 0); the angles wrapped into
// (-pi, pi]; in double, sums left to right, each of the six values rounded once.  Where nothing moves the value is X0's own, so that no zero changes its sign
// on the way through the matrix: the translation when a = b = 0, the angles when y = 0 and f = 0 (R_h is R(X0) then).
ICET_CLOSURE_HD inline void start_pose(const Consts& c, const float X0[6], const double Rh[9], int a, int b, int y, int f, float X[6]) {
    ICET_CLOSURE_NO_CONTRACT
    const double d0 = (double)a * (double)c.cell, d1 = (double)b * (double)c.cell, d2 = 0.0;
    for (int k = 0; k < 3; k++) {
        const double m0 = Rh[3 * k + 0] * d0, m1 = Rh[3 * k + 1] * d1, m2 = Rh[3 * k + 2] * d2;
        const double s = m0 + m1;
        const double t = s + m2;
        X[k] = (a == 0 && b == 0) ? X0[k] : (float)((double)X0[k] + t);
    }
    double ang[3];
    icet_closure_rule::euler_of_R(Rh, ang);
    for (int k = 0; k < 3; k++) {
        double v = ang[k];
        if (v <= -kPi) v = v + 2.0 * kPi;
        X[3 + k] = (y == 0 && f == 0) ? X0[3 + k] : (float)v;
    }
}

// ---- the whole rule on the host (the CPU test; the kernels do the same in parallel) ----
#if !defined(__HIP_DEVICE_COMPILE__)
// The per-cell minima and maxima of a scan (n x 3, row-major points): q_min / q_max are G x G, -1 where no point counts.
inline void cell_extrema(const Consts& c, const float* p, size_t n, int32_t* q_min, int32_t* q_max) {
    for (size_t i = 0; i < (size_t)c.G * c.G; i++) { q_min[i] = -1; q_max[i] = -1; }
    for (size_t i = 0; i < n; i++) {
        int ix, iy, q;
        if (!count_point(c, p[3 * i], p[3 * i + 1], p[3 * i + 2], ix, iy, q)) continue;
        const size_t cell = (size_t)ix * c.G + iy;
        if (q_max[cell] < 0) { q_min[cell] = q; q_max[cell] = q; }
        else { if (q < q_min[cell]) q_min[cell] = q; if (q > q_max[cell]) q_max[cell] = q; }
    }
}
inline void set_bit(const Consts& c, uint32_t* grid, int ix, int iy) { grid[(size_t)ix * c.W + (iy >> 5)] |= 1u << (iy & 31); }
inline bool get_bit(const Consts& c, const uint32_t* grid, int ix, int iy) { return (grid[(size_t)ix * c.W + (iy >> 5)] >> (iy & 31)) & 1u; }
// A keyframe's grid: its spanning cells.  grid: G x W words.
inline void keyframe_grid(const Consts& c, const float* p, size_t n, uint32_t* grid) {
    const size_t cells = (size_t)c.G * c.G;
    int32_t* ext = new int32_t[2 * cells];
    cell_extrema(c, p, n, ext, ext + cells);
    memset(grid, 0, sizeof(uint32_t) * (size_t)c.G * c.W);
    for (int ix = 0; ix < c.G; ix++)
        for (int iy = 0; iy < c.G; iy++) {
            const size_t cell = (size_t)ix * c.G + iy;
            if (ext[cells + cell] >= 0 && cell_spans(c, ext[cell], ext[cells + cell])) set_bit(c, grid, ix, iy);
        }
    delete[] ext;
}
// The live grid of a scan under (m, t): the cells its structure points (those whose own cell is set in `own`, the scan's keyframe grid) hit.
inline void live_grid(const Consts& c, const float* p, size_t n, const uint32_t* own, const float m[6], const float t[3], uint32_t* grid) {
    memset(grid, 0, sizeof(uint32_t) * (size_t)c.G * c.W);
    for (size_t i = 0; i < n; i++) {
        int ix, iy, q;
        if (!count_point(c, p[3 * i], p[3 * i + 1], p[3 * i + 2], ix, iy, q) || !get_bit(c, own, ix, iy)) continue;
        float xo, yo;
        transform_xy(m, t, p[3 * i], p[3 * i + 1], p[3 * i + 2], xo, yo);
        int jx, jy;
        if (coord_cell(c, xo, jx) && coord_cell(c, yo, jy)) set_bit(c, grid, jx, jy);
    }
}
// S(a, b): the live cells (i, j) whose keyframe cell (i + a, j + b) is set; cells shifted off the grid are dropped.
inline uint32_t shift_score(const Consts& c, const uint32_t* live, const uint32_t* key, int a, int b) {
    uint32_t s = 0;
    for (int i = 0; i < c.G; i++) {
        if (i + a < 0 || i + a >= c.G) continue;
        for (int j = 0; j < c.G; j++) {
            if (!live[(size_t)i * c.W + (j >> 5)]) { j |= 31; continue; }      // (an empty word of the live row)
            if (j + b < 0 || j + b >= c.G) continue;
            if (get_bit(c, live, i, j) && get_bit(c, key, i + a, j + b)) s++;
        }
    }
    return s;
}
inline uint32_t grid_bits(const Consts& c, const uint32_t* grid) {
    uint32_t s = 0;
    for (size_t i = 0; i < (size_t)c.G * c.W; i++) s += (uint32_t)__builtin_popcount(grid[i]);
    return s;
}
// The best key of one hypothesis over the window.
inline uint64_t best_shift(const Consts& c, const uint32_t* live, const uint32_t* key, int window, int h) {
    uint64_t best = 0;
    for (int a = -window; a <= window; a++)
        for (int b = -window; b <= window; b++) {
            const uint64_t k = shift_key(shift_score(c, live, key, a, b), a, b, h);
            if (k > best) best = k;
        }
    return best;
}
#endif

}  // namespace icet_coarse_rule
