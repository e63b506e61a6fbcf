// icet_amd/csrc/icet_map_evidence.h -- the RULE of a voxel map's visibility evidence (include/icet_hip.h icet_voxel_map_evidence_*), in one
// place: a scan row's pixel and range word in the scan's range image, the near image, a cell of the map against one scan at a pose (miss / agree / occluded),
// and the transient decision.  HIP-free C++ like icet_map.h and icet_map_query.h: the kernels and the host code of icet_map.hip and the CPU test
// (tests/cpp/test_map_evidence_rule.cpp) compile this text.
//
// POSE: the map's (icet_map.h): 4 x 4 row-major float32 T = [R | t], p_world = R p + t; a cell is carried into a scan's frame as R^T (m - t), as a query does.
// IMAGE: W x W pixels, W = 2^image_log2, of a direction's OCTAHEDRAL map: divisions and absolute values only, no trigonometry.  A pixel is the bit pattern of a
// float32 range (positive floats and +inf order as their bits), all ones when empty; it keeps the minimum over its rows, which does not depend on order.
// ARITHMETIC: IEEE double, one rounding per operation, nothing contracted; division and square root are the correctly rounded double operations.
#pragma once
#include "icet_map_query.h"

namespace icet_map_evidence_rule {

constexpr uint32_t kEmptyPixel = 0xFFFFFFFFu;
constexpr int32_t kMaxBatch = 256;             // scans of one batch: what a block stages in LDS
enum CellClass { kNone = 0, kMiss = 1, kAgree = 2, kOccluded = 3 };

// What a call fixes.  The squares are taken in double from the float32 parameters, as the map's and the query's are.
struct Consts {
    double min2, max2, margin, half_w, inv_cell;
    float max_range;
    int32_t w_log2, width, window, min_miss, agree_factor;
};

inline bool params_ok(float min_range, float max_range, float margin, int32_t image_log2, int32_t window, int32_t min_miss, int32_t agree_factor, int32_t flags) {
    if (!isfinite(min_range) || !isfinite(max_range) || !isfinite(margin) || !(max_range > 0.f) || !(margin >= 0.f)) return false;
    return image_log2 >= 4 && image_log2 <= 10 && window >= 0 && window <= 2 && min_miss >= 0 && agree_factor >= 0 && flags == 0;
}
inline Consts make_consts(float cell, float min_range, float max_range, float margin, int32_t image_log2, int32_t window, int32_t min_miss, int32_t agree_factor) {
    Consts c;
    c.min2 = (double)min_range * (double)min_range;
    c.max2 = (double)max_range * (double)max_range;
    c.margin = (double)margin;
    c.w_log2 = image_log2; c.width = 1 << image_log2;
    c.half_w = (double)(c.width / 2);
    c.inv_cell = 1.0 / (double)cell;
    c.max_range = max_range;
    c.window = window; c.min_miss = min_miss; c.agree_factor = agree_factor;
    return c;
}

ICET_CLOSURE_HD inline uint32_t float_word(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
ICET_CLOSURE_HD inline float word_float(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

// A.3 to A.5: the pixel v W + u of the direction (x, y, z), not all zero.
ICET_CLOSURE_HD inline int32_t pixel(const Consts& k, double x, double y, double z) {
    ICET_CLOSURE_NO_CONTRACT
    const double axy = fabs(x) + fabs(y);
    const double a = axy + fabs(z);
    double px = x / a, py = y / a;
    if (z < 0.0) {
        const double fx = 1.0 - fabs(py), fy = 1.0 - fabs(px);
        const double qx = px < 0.0 ? -fx : fx, qy = py < 0.0 ? -fy : fy;      // (1 - |py|) sgn(px): a product with +-1 is the sign
        px = qx; py = qy;
    }
    const double top = (double)(k.width - 1);
    double fu = floor((px + 1.0) * k.half_w), fv = floor((py + 1.0) * k.half_w);
    fu = !(fu >= 0.0) ? 0.0 : (fu > top ? top : fu);                  // the double is clamped, then converted
    fv = !(fv >= 0.0) ? 0.0 : (fv > top ? top : fv);
    return ((int32_t)fv << k.w_log2) + (int32_t)fu;
}

// A: the row (x, y, z) of a scan in its own frame.  False: the row takes no part.
ICET_CLOSURE_HD inline bool row_pixel(const Consts& k, float x, float y, float z, int32_t& pix, uint32_t& word) {
    ICET_CLOSURE_NO_CONTRACT
    if (!(fabsf(x) <= 3.402823466e+38f) || !(fabsf(y) <= 3.402823466e+38f) || !(fabsf(z) <= 3.402823466e+38f)) return false;
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double sxy = xx + yy;
    const double d2 = sxy + zz;
    if (!(d2 > k.min2)) return false;
    pix = pixel(k, dx, dy, dz);
    word = float_word((float)sqrt(d2));
    return true;
}

// B: the minimum of the image over the window around pixel (u, v), clipped to the image.
ICET_CLOSURE_HD inline uint32_t near_word(const Consts& k, const uint32_t* img, int32_t u, int32_t v) {
    uint32_t best = kEmptyPixel;
    const int32_t v0 = v - k.window < 0 ? 0 : v - k.window, v1 = v + k.window > k.width - 1 ? k.width - 1 : v + k.window;
    const int32_t u0 = u - k.window < 0 ? 0 : u - k.window, u1 = u + k.window > k.width - 1 ? k.width - 1 : u + k.window;
    for (int32_t b = v0; b <= v1; b++)
        for (int32_t a = u0; a <= u1; a++) { const uint32_t w = img[(b << k.w_log2) + a]; best = w < best ? w : best; }
    return best;
}

// C.2 to C.4: the cell of centroid m against the scan at the usable pose T.  False: the scan takes no part for this cell.  d2: |R^T (m - t)|^2.
ICET_CLOSURE_HD inline bool cell_pixel(const Consts& k, const float* T, float m0, float m1, float m2, int32_t& pix, double& d2) {
    ICET_CLOSURE_NO_CONTRACT
    const double d0 = (double)m0 - (double)T[3], d1 = (double)m1 - (double)T[7], e2 = (double)m2 - (double)T[11];
    double p[3];
    for (int a = 0; a < 3; a++) {
        const double q0 = (double)T[a] * d0, q1 = (double)T[4 + a] * d1, q2 = (double)T[8 + a] * e2;
        const double s01 = q0 + q1;
        p[a] = s01 + q2;
    }
    const double s0 = p[0] * p[0], s1 = p[1] * p[1], s2 = p[2] * p[2];
    const double s01 = s0 + s1;
    d2 = s01 + s2;
    if (!(d2 > k.min2) || !(d2 <= k.max2)) return false;
    pix = pixel(k, p[0], p[1], p[2]);
    return true;
}

// C.5: the class of a cell at squared range d2 whose near pixel holds `near`.
ICET_CLOSURE_HD inline int cell_class(const Consts& k, double d2, uint32_t near) {
    ICET_CLOSURE_NO_CONTRACT
    if (near == kEmptyPixel) return kNone;
    const double rc = sqrt(d2), rn = (double)word_float(near);
    const double far_edge = rc + k.margin, near_edge = rc - k.margin;
    if (rn > far_edge) return kMiss;
    return rn >= near_edge ? kAgree : kOccluded;
}

// D: the decision of a cell from its two sums.
ICET_CLOSURE_HD inline bool transient(const Consts& k, int32_t miss, int32_t agree) {
    const int32_t need = k.min_miss > 1 ? k.min_miss : 1;
    return miss >= need && (int64_t)miss > (int64_t)k.agree_factor * (int64_t)agree;
}

// PRUNING, the query's (icet_map_query.h x_interval): a cell that takes part has |R^T d| <= max_range.  The query's interval bounds |d_0| by max_range, which
// follows only where R is a rotation: with G = R R^T and delta = |G - I|_F, |d| <= |R^T d| / sqrt(1 - delta), so d_0 can exceed max_range by delta max_range
// at most.  The interval's one cell of slack has 2^-4 of a cell used by the centroid's rounding; the pose is pruned only where delta max_range / cell <= 1/4.
// Any other R (it is the caller's, not checked) is tested against every chunk: same bits either way.  An unusable pose has the empty interval.
ICET_CLOSURE_HD inline void x_interval(const Consts& k, const float* T, bool prune, int32_t& lo, int32_t& hi) {
    ICET_CLOSURE_NO_CONTRACT
    icet_map_query_rule::Consts q;
    q.min2 = 0.0; q.max2 = k.max2; q.inv_cell = k.inv_cell; q.max_range = k.max_range; q.has_max = 1; q.min_points = 1; q.world = 0;
    if (prune && icet_map_query_rule::pose_ok(T)) {
        double dev = 0.0;
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                const double g = ((double)T[4 * a] * (double)T[4 * b] + (double)T[4 * a + 1] * (double)T[4 * b + 1]) + (double)T[4 * a + 2] * (double)T[4 * b + 2];
                const double r = g - (a == b ? 1.0 : 0.0);
                dev = dev + r * r;
            }
        prune = sqrt(dev) * (double)k.max_range * k.inv_cell <= 0.25;  // (a NaN compares false: not pruned)
    }
    icet_map_query_rule::x_interval(q, T, prune, lo, hi);
}

}  // namespace icet_map_evidence_rule
