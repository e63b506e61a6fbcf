// icet_amd/csrc/icet_map_register.h -- the RULE of the registration against a shaped voxel map (include/icet_hip.h icet_voxel_map_register_*; DESIGN.md section
// 26), in one place: a cell's Gaussian from its integer words, what one row of a scan at a pose adds to the cost F, the gradient g and the Gauss-Newton matrix H,
// the damped 6 x 6 solve, the retraction, and the Levenberg-Marquardt state machine of one query.  HIP-free C++: the kernels and the host code of
// icet_map_register.hip and the CPU test (tests/cpp/test_map_register_rule.cpp) compile this text; tests/map_register_model.py restates it in NumPy.
//
// ARITHMETIC: as icet_map.h and icet_map_shape.h -- IEEE double, one rounding per operation, nothing contracted, division and square root correctly rounded, no
// transcendental (the rotation of a step is the deskewer's series).  This header is the authority on the order of the operations.
// POSE: P = (R, t), twelve doubles, R row-major; p_world = R p + t.  TANGENT: world-aligned at the sensor origin, delta = (rho, om): w' = w + rho + om x r with
// r = R p, so J = [I | -[r]x] and the weight matrix W of a cell is never rotated.  RETRACTION: R <- E(om) R, t <- t + rho.
// SUMS: a thread, a chunk, a query add terms in a fixed order (icet_map_register.hip); F, g and H of a query are sums of per-row terms and nothing else.
#pragma once
#include "icet_map_shape.h"
#include "icet_posegraph.h"
#include "icet_deskew.h"

namespace icet_map_register_rule {

namespace mrule = icet_map_rule;
namespace srule = icet_map_shape_rule;
namespace pg = icet_pg_rule;
namespace dk = icet_deskew_rule;

constexpr int kMaxQueries = 256;
constexpr int kMaxIters = 64;
constexpr int kChunkRows = 2048;             // the rows of one partial sum: one block of the row pass
constexpr int kSums = 28;                    // F | g[6] | H[21] (the upper triangle by rows)
constexpr double kLambdaMin = 1e-9;
constexpr double kLambdaMax = 1e9;
constexpr double kLambdaStep = 10.0;
constexpr int kSolveTries = 8;               // damped solves inside one step before the query is STALLED
constexpr double kDblMax = 1.7976931348623157e308;

// a query's status.  kIterationCap is also what a query that is still running carries: a terminal query has any other value
enum Status { kConverged = 0, kIterationCap = 1, kStalled = 2, kNoOverlap = 3, kBadPose = 4 };

struct Consts {
    mrule::Consts map;                       // the map's cell, the CALL's ranges
    srule::Consts shape;
    double sigma2;                           // sigma_min^2
    double c;                                // the robust scale: a miss costs c
    double tol_t2, tol_r2;                   // squares of the tolerances
    double lambda0;
    int32_t min_points, min_matched, max_iters, pad;
};
inline Consts make_consts(float cell, float min_range, float max_range, double sigma_min, double scale, double tol_t, double tol_r, double lambda0,
                          int32_t min_points, int32_t min_matched, int32_t max_iters) {
    Consts k;
    k.map = mrule::make_consts(cell, min_range, max_range);
    k.shape = srule::make_consts(cell);
    k.sigma2 = sigma_min * sigma_min;
    k.c = scale;
    k.tol_t2 = tol_t * tol_t; k.tol_r2 = tol_r * tol_r;
    k.lambda0 = lambda0;
    k.min_points = min_points < 1 ? 1 : min_points; k.min_matched = min_matched; k.max_iters = max_iters; k.pad = 0;
    return k;
}
inline bool params_ok(float min_range, float max_range, double sigma_min, double scale, double tol_t, double tol_r, double lambda0, int32_t max_iters, int32_t flags) {
    if (!isfinite(min_range) || !isfinite(max_range)) return false;
    if (!(sigma_min > 0.0 && sigma_min <= kDblMax) || !(scale > 0.0 && scale <= kDblMax)) return false;
    if (!(tol_t >= 0.0 && tol_t <= kDblMax) || !(tol_r >= 0.0 && tol_r <= kDblMax) || !(lambda0 > 0.0 && lambda0 <= kDblMax)) return false;
    return max_iters >= 0 && max_iters <= kMaxIters && flags == 0;
}

ICET_CLOSURE_HD inline bool finite(double v) { return fabs(v) <= kDblMax; }

// ---- a cell's Gaussian ------------------------------------------------------------------------------------------------------------------------------------------
// 80 bytes per table entry: the mean, W = (C + sigma_min^2 I)^-1 as xx xy xz yy yz zz, and the count -- 0 for an entry that takes no part.
struct Gauss { double mu[3]; double W[6]; int64_t n; };

// The entry of `key` with count n, offset sums sum[3] and moment words w[9] (all as the table holds them).  False, and g.n = 0: unusable.
ICET_CLOSURE_HD inline bool gauss(const Consts& k, uint64_t key, int64_t n, const uint64_t sum[3], const uint64_t w[srule::kWords], Gauss& g) {
    ICET_CLOSURE_NO_CONTRACT
    g.n = 0;
    for (int a = 0; a < 3; a++) g.mu[a] = 0.0;
    for (int j = 0; j < 6; j++) g.W[j] = 0.0;
    if (n < (int64_t)k.min_points) return false;          // (min_points >= 1: an emptied entry and a negative count end here)
    int32_t c[3];
    mrule::key_cells(key, c);
    const double den = (double)n * mrule::kTwo32;
    double mu[3];
    for (int a = 0; a < 3; a++) {
        const double off = (double)sum[a] / den;
        const double pos = (double)c[a] + off;
        mu[a] = pos * (double)k.map.cell;
    }
    double C[6];
    srule::cov(k.shape, n, w, C);
    C[0] = C[0] + k.sigma2; C[3] = C[3] + k.sigma2; C[5] = C[5] + k.sigma2;
    // the adjugate of the symmetric C (xx xy xz yy yz zz = 0 .. 5), every product rounded, then the difference
    const double p00a = C[3] * C[5], p00b = C[4] * C[4];
    const double p01a = C[2] * C[4], p01b = C[1] * C[5];
    const double p02a = C[1] * C[4], p02b = C[2] * C[3];
    const double p11a = C[0] * C[5], p11b = C[2] * C[2];
    const double p12a = C[1] * C[2], p12b = C[0] * C[4];
    const double p22a = C[0] * C[3], p22b = C[1] * C[1];
    const double a00 = p00a - p00b, a01 = p01a - p01b, a02 = p02a - p02b, a11 = p11a - p11b, a12 = p12a - p12b, a22 = p22a - p22b;
    const double d0 = C[0] * a00, d1 = C[1] * a01, d2 = C[2] * a02;
    const double d01 = d0 + d1;
    const double det = d01 + d2;
    if (!(det > 0.0) || !finite(det)) return false;
    const double W[6] = {a00 / det, a01 / det, a02 / det, a11 / det, a12 / det, a22 / det};
    for (int j = 0; j < 6; j++) if (!finite(W[j])) return false;
    for (int a = 0; a < 3; a++) g.mu[a] = mu[a];
    for (int j = 0; j < 6; j++) g.W[j] = W[j];
    g.n = n;
    return true;
}

// ---- one row at a pose --------------------------------------------------------------------------------------------------------------------------------------------
struct Pose { double R[9]; double t[3]; };

ICET_CLOSURE_HD inline void pose_from_float(const float* T, Pose& P) {
    for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) P.R[3 * a + b] = (double)T[4 * a + b]; P.t[a] = (double)T[4 * a + 3]; }
}
ICET_CLOSURE_HD inline bool pose_finite(const Pose& P) {
    bool ok = true;
    for (int j = 0; j < 9; j++) ok = ok && finite(P.R[j]);
    for (int a = 0; a < 3; a++) ok = ok && finite(P.t[a]);
    return ok;
}

// The part of the class that does not depend on the pose: kRowNonfinite, kRowRange, or kRowKept for a row that is scored (icet_map_rule::classify's tests).
ICET_CLOSURE_HD inline int row_class(const Consts& k, float x, float y, float z) {
    ICET_CLOSURE_NO_CONTRACT
    if (!(fabsf(x) <= 3.402823466e+38f) || !(fabsf(y) <= 3.402823466e+38f) || !(fabsf(z) <= 3.402823466e+38f)) return mrule::kRowNonfinite;
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double sxy = xx + yy;
    const double d2 = sxy + zz;
    if (!(d2 > k.map.min2)) return mrule::kRowRange;
    if (k.map.has_max && !(d2 <= k.map.max2)) return mrule::kRowRange;
    return mrule::kRowKept;
}
// r = R p, w = r + t, and the key of w's cell.  False: the row is outside the grid (the class is kRowOutside); r and w are written either way.
ICET_CLOSURE_HD inline bool row_world(const Consts& k, const Pose& P, float x, float y, float z, double r[3], double w[3], uint64_t& key) {
    ICET_CLOSURE_NO_CONTRACT
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    int32_t c[3]; uint32_t q;
    bool in = true;
    for (int a = 0; a < 3; a++) {
        const double p0 = P.R[3 * a] * dx, p1 = P.R[3 * a + 1] * dy, p2 = P.R[3 * a + 2] * dz;
        const double s01 = p0 + p1;
        r[a] = s01 + p2;
        w[a] = r[a] + P.t[a];
        c[a] = 0;
        if (in && !mrule::axis_cell(k.map, w[a], c[a], q)) in = false;
    }
    key = in ? mrule::make_key(c[0], c[1], c[2]) : mrule::kEmpty;
    return in;
}

// What one row adds to the running sums: v[0] = rho, v[1 .. 6] = omega J^T a, v[7 .. 27] = the upper triangle of omega J^T W J by rows.  A miss costs rho = c and
// adds nothing to the sums: the misses are COUNTED, and the cost of a pose is the matched rows' sum + c x the misses (cost_of), so that a miss costs exactly c
// whatever the order of the rows.
struct Terms { double s, omega, rho; double v[kSums]; };

ICET_CLOSURE_HD inline void miss_terms(const Consts& k, Terms& o) {
    o.s = 0.0; o.omega = 0.0; o.rho = k.c;
    for (int j = 0; j < kSums; j++) o.v[j] = 0.0;
}
ICET_CLOSURE_HD inline void match_terms(const Consts& k, const Gauss& G, const double r[3], const double w[3], Terms& o) {
    ICET_CLOSURE_NO_CONTRACT
    const double* W = G.W;
    double d[3];
    for (int a = 0; a < 3; a++) d[a] = w[a] - G.mu[a];
    // a = W d
    const double m00 = W[0] * d[0], m01 = W[1] * d[1], m02 = W[2] * d[2];
    const double m10 = W[1] * d[0], m11 = W[3] * d[1], m12 = W[4] * d[2];
    const double m20 = W[2] * d[0], m21 = W[4] * d[1], m22 = W[5] * d[2];
    const double s0 = m00 + m01, s1 = m10 + m11, s2 = m20 + m21;
    const double a[3] = {s0 + m02, s1 + m12, s2 + m22};
    const double q0 = d[0] * a[0], q1 = d[1] * a[1], q2 = d[2] * a[2];
    const double q01 = q0 + q1;
    const double s = q01 + q2;
    const double om = pg::robust_weight(pg::kRobustGemanMcClure, k.c, s);
    o.s = s; o.omega = om; o.rho = pg::robust_rho(pg::kRobustGemanMcClure, k.c, s);
    o.v[0] = o.rho;
    double ra[3];
    dk::cross3(r, a, ra);                             // J^T a = (a, r x a)
    for (int i = 0; i < 3; i++) { o.v[1 + i] = om * a[i]; o.v[4 + i] = om * ra[i]; }
    // M = W B, B = -[r]x: M_i0 = W_i2 r1 - W_i1 r2, M_i1 = W_i0 r2 - W_i2 r0, M_i2 = W_i1 r0 - W_i0 r1
    const double Wf[3][3] = {{W[0], W[1], W[2]}, {W[1], W[3], W[4]}, {W[2], W[4], W[5]}};
    double M[3][3];
    for (int i = 0; i < 3; i++) {
        const double a0 = Wf[i][2] * r[1], b0 = Wf[i][1] * r[2];
        const double a1 = Wf[i][0] * r[2], b1 = Wf[i][2] * r[0];
        const double a2 = Wf[i][1] * r[0], b2 = Wf[i][0] * r[1];
        M[i][0] = a0 - b0; M[i][1] = a1 - b1; M[i][2] = a2 - b2;
    }
    // RR = B^T M: RR_0k = r1 M_2k - r2 M_1k, RR_1k = r2 M_0k - r0 M_2k, RR_2k = r0 M_1k - r1 M_0k
    double RR[3][3];
    for (int c = 0; c < 3; c++) {
        const double a0 = r[1] * M[2][c], b0 = r[2] * M[1][c];
        const double a1 = r[2] * M[0][c], b1 = r[0] * M[2][c];
        const double a2 = r[0] * M[1][c], b2 = r[1] * M[0][c];
        RR[0][c] = a0 - b0; RR[1][c] = a1 - b1; RR[2][c] = a2 - b2;
    }
    double* H = o.v + 7;
    H[0] = om * Wf[0][0]; H[1] = om * Wf[0][1]; H[2] = om * Wf[0][2]; H[3] = om * M[0][0]; H[4] = om * M[0][1]; H[5] = om * M[0][2];
    H[6] = om * Wf[1][1]; H[7] = om * Wf[1][2]; H[8] = om * M[1][0]; H[9] = om * M[1][1]; H[10] = om * M[1][2];
    H[11] = om * Wf[2][2]; H[12] = om * M[2][0]; H[13] = om * M[2][1]; H[14] = om * M[2][2];
    H[15] = om * RR[0][0]; H[16] = om * RR[0][1]; H[17] = om * RR[0][2];
    H[18] = om * RR[1][1]; H[19] = om * RR[1][2];
    H[20] = om * RR[2][2];
}

// ---- the neighbourhood of a row ---------------------------------------------------------------------------------------------------------------------------------
// A row is scored against ONE cell of its neighbourhood: the usable cell with the smallest s = d . W d, the earlier in the order on a tie.  N1: the row's own cell
// (the code above and nothing else).  N7: own, -x, +x, -y, +y, -z, +z.  N27: own, then the other 26 offsets (dx, dy, dz), dx slowest, each over -1, 0, 1.  A
// neighbour whose cell index leaves the grid is skipped; a row outside the grid has no neighbourhood.  rho is at most c and a miss exactly c whatever the
// neighbourhood, row by row rho(N27) <= rho(N7) <= rho(N1), and the cost is continuous across a face whenever the winner is among the cells on both sides.
constexpr int32_t kFlagNeighbours7 = 2, kFlagNeighbours27 = 4;      // params.flags (include/icet_hip.h ICET_VOXEL_MAP_REG_NEIGHBOURS_*)
constexpr double kInf = __builtin_huge_val();                       // +infinity

// The cells of the neighbourhood that `flags` names: 1, 7 or 27; 0 for flags that are refused (both bits, or any other bit).
inline int neighbours_of(int32_t flags) {
    return flags == 0 ? 1 : flags == kFlagNeighbours7 ? 7 : flags == kFlagNeighbours27 ? 27 : 0;
}
// Place j (0 .. K - 1) of the neighbourhood of K = 7 or 27 cells: the offset in cells.  Place 0 is the row's own cell.
ICET_CLOSURE_HD inline void neighbour_offset(int K, int j, int32_t d[3]) {
    d[0] = 0; d[1] = 0; d[2] = 0;
    if (j == 0) return;
    if (K == 7) { d[(j - 1) >> 1] = ((j - 1) & 1) ? 1 : -1; return; }
    const int i = j <= 13 ? j - 1 : j;                                // the place among all 27 offsets, the centre (13) taken out
    d[0] = i / 9 - 1; d[1] = (i / 3) % 3 - 1; d[2] = i % 3 - 1;
}
// The key of the cell at place j around the cell of `own` (a key, not kEmpty).  False: the cell is outside the grid (a key field outside 1 .. 2^21 - 1).
ICET_CLOSURE_HD inline bool neighbour_key(int K, int j, uint64_t own, uint64_t& key) {
    int32_t c[3], d[3];
    mrule::key_cells(own, c);
    neighbour_offset(K, j, d);
    bool in = true;
    for (int a = 0; a < 3; a++) { c[a] += d[a]; in = in && c[a] > -mrule::kCellLimit && c[a] < mrule::kCellLimit; }
    key = in ? mrule::make_key(c[0], c[1], c[2]) : mrule::kEmpty;
    return in;
}
// s = d . W d of the world point w against G, in match_terms' order of operations: what the selection compares.
ICET_CLOSURE_HD inline double match_s(const Gauss& G, const double w[3]) {
    ICET_CLOSURE_NO_CONTRACT
    const double* W = G.W;
    double d[3];
    for (int a = 0; a < 3; a++) d[a] = w[a] - G.mu[a];
    const double m00 = W[0] * d[0], m01 = W[1] * d[1], m02 = W[2] * d[2];
    const double m10 = W[1] * d[0], m11 = W[3] * d[1], m12 = W[4] * d[2];
    const double m20 = W[2] * d[0], m21 = W[4] * d[1], m22 = W[5] * d[2];
    const double s0 = m00 + m01, s1 = m10 + m11, s2 = m20 + m21;
    const double a[3] = {s0 + m02, s1 + m12, s2 + m22};
    const double q0 = d[0] * a[0], q1 = d[1] * a[1], q2 = d[2] * a[2];
    const double q01 = q0 + q1;
    return q01 + q2;
}
// The running selection of one row: start() before the first cell, offer() per usable cell in the order of the places.  A cell wins iff its s is below the best so
// far: a tie stays with the earlier place, and a NaN or infinite s never wins.  place < 0: no winner, the row is a miss.
struct Best { double s; int32_t place; };
ICET_CLOSURE_HD inline void best_start(Best& b) { b.s = kInf; b.place = -1; }
ICET_CLOSURE_HD inline bool best_offer(Best& b, int place, double s) {
    if (!(s < b.s)) return false;
    b.s = s; b.place = place;
    return true;
}
// The same selection with the cells offered in ANY order: the winner is the least (s, place), which is what offering them in the order of the places gives (an
// infinite s equals the start's and no place is below -1, a NaN compares false: neither wins here either).  The 27-cell row pass walks x slices with it.
ICET_CLOSURE_HD inline bool best_offer_any(Best& b, int place, double s) {
    if (!(s < b.s || (s == b.s && place < b.place))) return false;
    b.s = s; b.place = place;
    return true;
}
// The place in N27's order of the offset (dx, dy, dz), each -1, 0 or 1.
ICET_CLOSURE_HD inline int place27(int dx, int dy, int dz) {
    const int i = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1);
    return i == 13 ? 0 : i < 13 ? i + 1 : i;
}

// A running sum of rows: the 28 doubles and the two counts.
struct Acc { double v[kSums]; int32_t scored, matched; };
ICET_CLOSURE_HD inline void acc_zero(Acc& a) { for (int j = 0; j < kSums; j++) a.v[j] = 0.0; a.scored = 0; a.matched = 0; }
ICET_CLOSURE_HD inline void acc_row(Acc& a, const Terms& t, bool matched) {
    for (int j = 0; j < kSums; j++) a.v[j] = a.v[j] + t.v[j];
    a.scored++; a.matched += matched ? 1 : 0;
}
ICET_CLOSURE_HD inline void acc_add(Acc& a, const Acc& b) {
    for (int j = 0; j < kSums; j++) a.v[j] = a.v[j] + b.v[j];
    a.scored += b.scored; a.matched += b.matched;
}
// F of a query from its total: the matched rows' rho + c x the misses
ICET_CLOSURE_HD inline double cost_of(const Consts& k, const Acc& tot) {
    ICET_CLOSURE_NO_CONTRACT
    const double misses = k.c * (double)(tot.scored - tot.matched);
    return tot.v[0] + misses;
}

// ---- the damped solve and the retraction -------------------------------------------------------------------------------------------------------------------------
ICET_CLOSURE_HD inline int tri(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }      // (i <= j) the place of H_ij among the 21

// (H + lambda diag(H)) delta = -g by a 6 x 6 Cholesky.  False: a pivot is not above kPivotRel x its diagonal entry (a NaN fails the test too).
ICET_CLOSURE_HD inline bool solve_damped(const double H[21], const double g[6], double lambda, double delta[6]) {
    ICET_CLOSURE_NO_CONTRACT
    double A[6][6], L[6][6];
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) { A[i][j] = H[tri(i, j)]; A[j][i] = A[i][j]; }
    for (int i = 0; i < 6; i++) { const double e = lambda * A[i][i]; A[i][i] = A[i][i] + e; }
    for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) L[i][j] = 0.0;
    for (int j = 0; j < 6; j++) {
        double s = A[j][j];
        for (int k = 0; k < j; k++) { const double p = L[j][k] * L[j][k]; s = s - p; }
        if (!(s > pg::kPivotRel * fabs(A[j][j]))) return false;
        const double l = sqrt(s);
        L[j][j] = l;
        for (int i = j + 1; i < 6; i++) {
            double u = A[i][j];
            for (int k = 0; k < j; k++) { const double p = L[i][k] * L[j][k]; u = u - p; }
            L[i][j] = u / l;
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) {
        double u = -g[i];
        for (int k = 0; k < i; k++) { const double p = L[i][k] * y[k]; u = u - p; }
        y[i] = u / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
        double u = y[i];
        for (int k = i + 1; k < 6; k++) { const double p = L[k][i] * delta[k]; u = u - p; }
        delta[i] = u / L[i][i];
    }
    return true;
}

// E = the rotation part of icet_deskew_rule::pose_from_twist((0, om), 1), series branch only, operation for operation.  False: om . om > 1 or not a number.
ICET_CLOSURE_HD inline bool step_rotation(const double om[3], double E[9]) {
    ICET_CLOSURE_NO_CONTRACT
    const double xx = om[0] * om[0], yy = om[1] * om[1], zz = om[2] * om[2];
    const double sxy = xx + yy;
    const double u = sxy + zz;
    if (!(u <= 1.0)) return false;
    const double A = dk::series_a(u), B = dk::series_b(u);
    for (int j = 0; j < 3; j++) {
        double e[3] = {0.0, 0.0, 0.0}, c1[3], c2[3];
        e[j] = 1.0;
        dk::cross3(om, e, c1); dk::cross3(om, c1, c2);
        for (int a = 0; a < 3; a++) {
            const double t1 = A * c1[a], t2 = B * c2[a];
            const double s1 = e[a] + t1;
            E[3 * a + j] = s1 + t2;
        }
    }
    return true;
}
// Q = the pose P moved by delta = (rho, om).  False: a failed step (a non-finite entry of delta, or om . om > 1).
ICET_CLOSURE_HD inline bool retract(const Pose& P, const double delta[6], Pose& Q) {
    ICET_CLOSURE_NO_CONTRACT
    for (int j = 0; j < 6; j++) if (!finite(delta[j])) return false;
    double E[9];
    if (!step_rotation(delta + 3, E)) return false;
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) {
            const double p0 = E[3 * a] * P.R[b], p1 = E[3 * a + 1] * P.R[3 + b], p2 = E[3 * a + 2] * P.R[6 + b];
            const double s01 = p0 + p1;
            Q.R[3 * a + b] = s01 + p2;
        }
        Q.t[a] = P.t[a] + delta[a];
    }
    return true;
}
ICET_CLOSURE_HD inline double norm2(const double v[3]) {
    ICET_CLOSURE_NO_CONTRACT
    const double xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
    const double sxy = xx + yy;
    return sxy + zz;
}

// ---- the loop -----------------------------------------------------------------------------------------------------------------------------------------------------
// What a query carries between passes.  cur: the pose accepted last and its sums; trial: the pose the next row pass evaluates, reached from cur by delta.
struct State {
    Pose cur, trial;
    double v[kSums];               // F, g, H at cur
    double delta[6];
    double lambda, cost_start;
    int32_t scored, matched, iterations, accepted, status, pad;
};
// The record of a query: icet_voxel_map_registration of include/icet_hip.h, word for word.
struct Record {
    float pose[16];
    double info[21], g[6];
    double cost, cost_start, lambda;
    int32_t rows_scored, rows_matched, iterations, accepted, status, reserved;
};

// The next trial from st.cur: damped solves until one factorises and its step can be taken, lambda raised in between.  Sets kStalled when none does.
ICET_CLOSURE_HD inline void propose(State& st) {
    ICET_CLOSURE_NO_CONTRACT
    for (int tries = 0; tries < kSolveTries; tries++) {
        if (solve_damped(st.v + 7, st.v + 1, st.lambda, st.delta) && retract(st.cur, st.delta, st.trial)) return;
        st.lambda = st.lambda * kLambdaStep;
        if (st.lambda > kLambdaMax) break;
    }
    st.status = kStalled;
}
ICET_CLOSURE_HD inline void write_record(const State& st, const float* start, bool start_bits, Record& rec) {
    for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) rec.pose[4 * a + b] = (float)st.cur.R[3 * a + b]; rec.pose[4 * a + 3] = (float)st.cur.t[a]; }
    rec.pose[12] = 0.f; rec.pose[13] = 0.f; rec.pose[14] = 0.f; rec.pose[15] = 1.f;
    if (start_bits) for (int j = 0; j < 16; j++) rec.pose[j] = start[j];
    for (int j = 0; j < 21; j++) rec.info[j] = st.v[7 + j];
    for (int j = 0; j < 6; j++) rec.g[j] = st.v[1 + j];
    rec.cost = st.v[0]; rec.cost_start = st.cost_start; rec.lambda = st.lambda;
    rec.rows_scored = st.scored; rec.rows_matched = st.matched; rec.iterations = st.iterations; rec.accepted = st.accepted; rec.status = st.status; rec.reserved = 0;
}
// Pass `pass` of one query: tot is what the row pass summed at the start pose (pass 0) or at st.trial (pass >= 1).  A terminal query (pass >= 1, status other
// than kIterationCap) must not be stepped: the caller skips it.  The record is valid after every pass.
ICET_CLOSURE_HD inline void step(const Consts& k, int pass, const float* start, const Acc& tot, State& st, Record& rec) {
    ICET_CLOSURE_NO_CONTRACT
    const double F = cost_of(k, tot);
    if (pass == 0) {
        pose_from_float(start, st.cur);
        st.trial = st.cur;
        for (int j = 0; j < kSums; j++) st.v[j] = tot.v[j];
        st.v[0] = F;
        for (int j = 0; j < 6; j++) st.delta[j] = 0.0;
        st.lambda = k.lambda0; st.cost_start = F;
        st.scored = tot.scored; st.matched = tot.matched; st.iterations = 0; st.accepted = 0; st.pad = 0;
        st.status = kIterationCap;
        if (!pose_finite(st.cur)) st.status = kBadPose;
        else if (tot.matched < k.min_matched) st.status = kNoOverlap;
        else if (k.max_iters > 0) propose(st);
        write_record(st, start, true, rec);
        return;
    }
    st.iterations = pass;
    if (finite(F) && F < st.v[0]) {
        st.cur = st.trial;
        for (int j = 0; j < kSums; j++) st.v[j] = tot.v[j];
        st.v[0] = F;
        st.scored = tot.scored; st.matched = tot.matched; st.accepted++;
        const double down = st.lambda / kLambdaStep;
        st.lambda = down > kLambdaMin ? down : kLambdaMin;
        if (norm2(st.delta) <= k.tol_t2 && norm2(st.delta + 3) <= k.tol_r2) st.status = kConverged;
    } else {
        st.lambda = st.lambda * kLambdaStep;
        if (st.lambda > kLambdaMax) st.status = kStalled;
    }
    if (st.status == kIterationCap && pass < k.max_iters) propose(st);
    write_record(st, start, st.accepted == 0, rec);
}

}  // namespace icet_map_register_rule
