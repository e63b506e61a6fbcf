// icet_amd/csrc/icet_map.h -- the RULE of the voxel map (include/icet_hip.h icet_voxel_map_*), in one place: what a row of a scan at a
// pose does to the map -- is it kept, its cell key and its three fixed-point offsets --, the key's cells, and the centroid of a cell from its integer sums.
// HIP-free C++: the kernels and the host code of icet_map.hip and the CPU test (tests/cpp/test_map_rule.cpp) compile this text.
//
// POSE: 4 x 4 row-major float32 T = [R | t; 0 0 0 1], p_world = R p + t (the store's convention, icet_closure.h).
// ARITHMETIC: IEEE double, one rounding per operation, nothing contracted.  Products of two float32 values are exact in double; the sums, the product with
// inv_cell and the offset are where a contraction would show.  What a row ADDS is integers only (a count and three 32-bit offsets into 64-bit sums), so the
// contents of a map depend on the multiset of (row, pose, sign) and on nothing else: not on order, call boundaries, launch shape or aggregation.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "icet_closure.h"

namespace icet_map_rule {

constexpr uint64_t kEmpty = ~(uint64_t)0;      // no cell: every key is below 2^63
constexpr int32_t kCellLimit = 1 << 20;        // |c| < 2^20 on every axis
constexpr double kTwo32 = 4294967296.0;
enum RowClass { kRowKept = 0, kRowNonfinite = 1, kRowRange = 2, kRowOutside = 3 };

// What create fixes.  inv_cell = 1 / (double)cell, min2 / max2 the squares of the limits in double.
struct Consts {
    double inv_cell, min2, max2;
    float cell;
    int32_t has_max;
};

inline bool params_ok(float cell, float min_range, float max_range, int32_t table_log2, int32_t flags) {
    if (!(cell > 0.f) || !isfinite(cell) || !isfinite(min_range) || !isfinite(max_range)) return false;
    return table_log2 >= 10 && table_log2 <= 30 && flags == 0;
}
inline bool sign_ok(int32_t sign) { return sign == 1 || sign == -1; }
inline Consts make_consts(float cell, float min_range, float max_range) {
    Consts c;
    c.cell = cell; c.inv_cell = 1.0 / (double)cell;
    c.min2 = (double)min_range * (double)min_range;
    c.max2 = (double)max_range * (double)max_range;
    c.has_max = max_range > 0.f;
    return c;
}

struct Point { uint64_t key; uint32_t q[3]; };

// One coordinate: s = w inv_cell, c = floor(s), u = s - c, q = min(floor(u 2^32), 2^32 - 1).  False when |c| >= 2^20 or w is not a number.
ICET_CLOSURE_HD inline bool axis_cell(const Consts& k, double w, int32_t& c, uint32_t& q) {
    ICET_CLOSURE_NO_CONTRACT
    const double s = w * k.inv_cell;
    const double cf = floor(s);
    if (!(fabs(cf) < (double)kCellLimit)) return false;
    const double u = s - cf;
    const double f = floor(u * kTwo32);        // 0 .. 2^32: u rounds to exactly 1 for a tiny negative s
    c = (int32_t)cf;
    q = f >= kTwo32 ? 0xFFFFFFFFu : (uint32_t)f;
    return true;
}

ICET_CLOSURE_HD inline uint64_t make_key(int32_t cx, int32_t cy, int32_t cz) {
    return ((uint64_t)(uint32_t)(cx + kCellLimit) << 42) | ((uint64_t)(uint32_t)(cy + kCellLimit) << 21) | (uint64_t)(uint32_t)(cz + kCellLimit);
}
ICET_CLOSURE_HD inline void key_cells(uint64_t key, int32_t c[3]) {
    c[0] = (int32_t)((key >> 42) & 0x1FFFFF) - kCellLimit; c[1] = (int32_t)((key >> 21) & 0x1FFFFF) - kCellLimit; c[2] = (int32_t)(key & 0x1FFFFF) - kCellLimit;
}

// The row (x, y, z) of a scan at the pose whose first three rows are T[0 .. 11] (row a: R[a][0 .. 2], t[a]).
ICET_CLOSURE_HD inline int classify(const Consts& k, const float* T, float x, float y, float z, Point& o) {
    ICET_CLOSURE_NO_CONTRACT
    if (!(fabsf(x) <= 3.402823466e+38f) || !(fabsf(y) <= 3.402823466e+38f) || !(fabsf(z) <= 3.402823466e+38f)) return kRowNonfinite;
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double sxy = xx + yy;
    const double d2 = sxy + zz;
    if (!(d2 > k.min2)) return kRowRange;
    if (k.has_max && !(d2 <= k.max2)) return kRowRange;
    int32_t c[3];
    for (int a = 0; a < 3; a++) {
        const double p0 = (double)T[4 * a] * dx, p1 = (double)T[4 * a + 1] * dy, p2 = (double)T[4 * a + 2] * dz;
        const double s01 = p0 + p1;
        const double s012 = s01 + p2;
        const double w = s012 + (double)T[4 * a + 3];
        if (!axis_cell(k, w, c[a], o.q[a])) return kRowOutside;
    }
    o.key = make_key(c[0], c[1], c[2]);
    return kRowKept;
}

// The centroid coordinate of a cell with index c, offset sum `sum` and count n >= 1.
ICET_CLOSURE_HD inline float centroid(const Consts& k, int32_t c, uint64_t sum, int64_t n) {
    ICET_CLOSURE_NO_CONTRACT
    const double den = (double)n * kTwo32;
    const double off = (double)sum / den;
    const double pos = (double)c + off;
    const double m = pos * (double)k.cell;
    return (float)m;
}

// Where a key's probe run starts: a 64-bit mix (splitmix64's finaliser).  It shows in no output.
ICET_CLOSURE_HD inline uint64_t mix(uint64_t v) {
    v ^= v >> 30; v *= 0xBF58476D1CE4E5B9ull;
    v ^= v >> 27; v *= 0x94D049BB133111EBull;
    return v ^ (v >> 31);
}

}  // namespace icet_map_rule
