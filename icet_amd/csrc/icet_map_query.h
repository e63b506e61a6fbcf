// icet_amd/csrc/icet_map_query.h -- the RULE of a voxel map's query (include/icet_hip.h icet_voxel_map_query_*), in one place: is a pose
// usable, does a cell of the map take part in the sub-map around a pose, the cell's row in the pose's own frame, and the run of x cells a query can reach.
// HIP-free C++ like icet_map.h: the kernels and the host code of icet_map.hip and the CPU test (tests/cpp/test_map_query_rule.cpp) compile this text.
//
// POSE: the map's (icet_map.h): 4 x 4 row-major float32 T = [R | t], p_world = R p + t.  The inverse is taken as [R^T | -R^T t]: R is the caller's, not checked.
// ARITHMETIC: IEEE double, one rounding per operation, nothing contracted.  The differences d_a = m_a - t_a are rounded (two float32 values need not differ by a
// double), so are their squares: the order written here is the rule.
#pragma once
#include "icet_map.h"

namespace icet_map_query_rule {

constexpr int32_t kFlagWorld = 1;              // ICET_VOXEL_MAP_QUERY_WORLD
constexpr int32_t kKnownFlags = kFlagWorld;
constexpr int32_t kMaxQueries = 256;

// What a call fixes for all of its queries.  The squares are taken in double from the float32 parameters, as icet_map_rule::make_consts takes the map's.
struct Consts {
    double min2, max2, inv_cell;
    float max_range;
    int32_t has_max, min_points, world;
};

inline bool params_ok(float min_range, float max_range, int32_t flags, const int32_t reserved[4]) {
    if (!isfinite(min_range) || !isfinite(max_range) || (flags & ~kKnownFlags)) return false;
    return !(reserved[0] | reserved[1] | reserved[2] | reserved[3]);
}
inline bool submap_ok(const void* xyz, int64_t ld, int64_t cap_rows) { return cap_rows >= 0 && ld >= cap_rows && (cap_rows == 0 || xyz != nullptr); }
inline Consts make_consts(float cell, float min_range, float max_range, int32_t min_points, int32_t flags) {
    Consts c;
    c.min2 = (double)min_range * (double)min_range;
    c.max2 = (double)max_range * (double)max_range;
    c.inv_cell = 1.0 / (double)cell;
    c.max_range = max_range;
    c.has_max = max_range > 0.f;
    c.min_points = min_points > 1 ? min_points : 1;
    c.world = (flags & kFlagWorld) != 0;
    return c;
}

// Step 1: the 12 entries of [R | t] are numbers.  (The last row of T is never read.)
ICET_CLOSURE_HD inline bool pose_ok(const float* T) {
    bool ok = true;
    for (int j = 0; j < 12; j++) ok = ok && fabsf(T[j]) <= 3.402823466e+38f;
    return ok;
}

// Steps 2 and 3: the cell of count n and centroid m takes part, and lies in the shell around t.  d: m - t, for row().
ICET_CLOSURE_HD inline bool keep(const Consts& k, const float* T, float m0, float m1, float m2, long long n, double d[3]) {
    ICET_CLOSURE_NO_CONTRACT
    d[0] = (double)m0 - (double)T[3]; d[1] = (double)m1 - (double)T[7]; d[2] = (double)m2 - (double)T[11];
    const double s0 = d[0] * d[0], s1 = d[1] * d[1], s2 = d[2] * d[2];
    const double s01 = s0 + s1;
    const double d2 = s01 + s2;
    if (n < (long long)k.min_points) return false;
    if (!(d2 > k.min2)) return false;
    return !k.has_max || d2 <= k.max2;
}

// Step 4: coordinate a of R^T d.
ICET_CLOSURE_HD inline float row(const float* T, const double d[3], int a) {
    ICET_CLOSURE_NO_CONTRACT
    const double p0 = (double)T[a] * d[0], p1 = (double)T[4 + a] * d[1], p2 = (double)T[8 + a] * d[2];
    const double s01 = p0 + p1;
    const double s = s01 + p2;
    return (float)s;
}

// PRUNING.  Keys sort x-major, so the cells a query can keep lie in a run of x cells.  A kept cell has |m_0 - t_0| <= max_range; its centroid m_0 is
// (float)((c + u) cell) with 0 <= u < 1, at most one cell off floor(m_0 / cell) after the roundings (|c| < 2^20: a float32 is good to 2^-4 of a cell there, the
// doubles below to 2^-30).  So [floor((t_0 - max_range) / cell) - 1, floor((t_0 + max_range) / cell) + 1] holds every cell the test could keep; without
// a max_range it is every cell.  The ends are clamped to what a key can hold.  An unusable pose has the empty interval (lo > hi).
ICET_CLOSURE_HD inline void x_interval(const Consts& k, const float* T, bool prune, int32_t& lo, int32_t& hi) {
    ICET_CLOSURE_NO_CONTRACT
    const int32_t lim = icet_map_rule::kCellLimit;
    if (!pose_ok(T)) { lo = lim; hi = -lim; return; }
    lo = -lim; hi = lim;
    if (!prune || !k.has_max) return;
    const double a = floor(((double)T[3] - (double)k.max_range) * k.inv_cell) - 1.0;
    const double b = floor(((double)T[3] + (double)k.max_range) * k.inv_cell) + 1.0;
    if (a > (double)-lim) lo = a < (double)lim ? (int32_t)a : lim;
    if (b < (double)lim) hi = b > (double)-lim ? (int32_t)b : -lim;
}
ICET_CLOSURE_HD inline int32_t key_x(uint64_t key) { return (int32_t)((key >> 42) & 0x1FFFFF) - icet_map_rule::kCellLimit; }

}  // namespace icet_map_query_rule
