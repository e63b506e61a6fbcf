// icet_amd/csrc/icet_capi.hip -- host side of the C ABI declared in include/icet_hip.h.
//
// Owns the device workspace, stages host scans into HBM, enqueues the keyframe build and the
// Gauss-Newton loop on one HIP stream and copies the 48 result floats per pair back.  No CPU
// implementation of the algorithm lives here: if the device or the kernels are unavailable every
// entry point returns ICET_ERR_NO_DEVICE / ICET_ERR_HIP.
// The keyframe store (icet_keyframe_store_*) is icet_store.hip; it registers through register_indexed, below, and shares the context with
// this file through icet_ctx.h.
#include "../../include/icet_hip.h"
#include "../../include/icet_nodes.h"
#include "icet_ctx.h"
#include "icet_layout.h"
#include "icet_closure.h"
#include "icet_appearance.h"
#include "icet_coarse.h"

#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <cstdint>
#include <new>
#include <atomic>

using namespace icet;

// The runtime behind every BufferGroup of the library (icet_buffers.h).
int icet::mem::dev_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
int icet::mem::dev_free(void* p) { return hipFree(p); }
int icet::mem::pinned_alloc(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
int icet::mem::pinned_free(void* p) { return hipHostFree(p); }

namespace {

// THE INVARIANT of every growth below: at every return, OK or not, a non-zero capacity means every pointer of its group (icet_ctx::Mem) is non-null and at least
// that large.  Where ONE capacity guards a group, grow() (icet_buffers.h) keeps it.  Four groups spell the same three steps out -- one statement releases the group
// and zeroes its capacity, the allocations follow, the capacity is set after the last -- because their capacity is more than one variable: the pair tables
// (cap_pairs, cap_V, h_cap_pairs), the registration side (cap_regs, cap_reg_V), the threshold tables (thr_T, thr_P), and scan 1 with the fit group (execbits,
// fit_items, fit_n_items; capacity cap_fit_items).  The fit group is sized from OTHER groups' capacities -- cap_pairs, cap_V, cap_n1 --, and no kernel is told its
// size: its capacity is zeroed as well wherever the pair tables or the scan-1 arrays are released, so that it is rebuilt for their new sizes by the call that grows
// them or, if that call is refused anywhere between, by the next one.  For it a non-zero capacity means: non-null and sized for the present cap_pairs, cap_V, cap_n1.

// The REGISTRATION side of the workspace (Workspace, icet_internal.h): n_regs registrations on a grid of V voxels.  Leaves the keyframe side alone.
icet_status ensure_regs(icet_ctx* c, int32_t n_regs, int V) {
    Workspace& w = c->w;
    if (n_regs <= w.cap_regs && V <= w.cap_reg_V) return ICET_OK;
    const int np = n_regs > w.cap_regs ? n_regs : w.cap_regs;
    const int VV = V > w.cap_reg_V ? V : w.cap_reg_V;
    const size_t pv = (size_t)np * VV;
    BufferGroup& g = c->mem.regs;
    HIPCHK(c, hipStreamSynchronize(c->stream));                            // (also: no replay or copy still reads the registration staging)
    w.cap_regs = w.cap_reg_V = 0, g.release();
    HIPCHK(c, g.device(w.acc, pv * kAccWords));
    HIPCHK(c, hipMemset(w.acc, 0, pv * kAccWords * sizeof(uint32_t)));
    HIPCHK(c, g.device(w.near_over_count, 2 * (size_t)np + 1));
    HIPCHK(c, hipMemset(w.near_over_count, 0, (2 * (size_t)np + 1) * sizeof(uint32_t)));
    HIPCHK(c, g.device(w.xf, (size_t)np * 48));
    HIPCHK(c, g.device(w.X, (size_t)np * 6));
    HIPCHK(c, g.device(w.desc_reg, np));
    HIPCHK(c, g.device(w.kf_of, (size_t)np + 1));
    HIPCHK(c, g.pinned(c->h_desc_reg, np));
    HIPCHK(c, g.pinned(c->h_kf_of, (size_t)np + 1));
    w.cap_regs = np; w.cap_reg_V = VV;
    c->ws_gen++;
    return ICET_OK;
}

// The scan-2 overflow list (registration side, sized by the scan-2 points of a call).
icet_status ensure_scan2(icet_ctx* c, int64_t total_n2) {
    Workspace& w = c->w;
    if (total_n2 >= (int64_t)1 << 31) { c->err = "total scan-2 points per call must be < 2^31"; return ICET_ERR_UNSUPPORTED; }
    if (total_n2 > w.cap_n2) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, grow(c->mem.scan2, w.cap_n2, total_n2, [&] { return c->mem.scan2.device(w.near_over, (size_t)total_n2); }));
        c->ws_gen++;
    }
    return ICET_OK;
}

icet_status ensure_workspace(icet_ctx* c, const icet_params* p, int32_t n_pairs, int64_t total_n1, int64_t total_n2) {
    Workspace& w = c->w;
    const int V = p->bins_phi * p->bins_theta;
    if ((int64_t)p->bins_phi * p->bins_theta > kMaxVoxels) { c->err = "bins_phi*bins_theta exceeds the voxel limit (10000: the multi-split keeps 12 B per voxel, the Gauss-Newton pass a 2-byte map entry and its look-up tables, in one block's LDS)"; return ICET_ERR_UNSUPPORTED; }
    if ((size_t)V * 12 + 8 + 4096 > (size_t)c->max_lds) { c->err = "grid too fine for this device's LDS (k_bin_scatter keeps 12 B per voxel in one block)"; return ICET_ERR_UNSUPPORTED; }
    if (total_n1 >= (int64_t)1 << 31) { c->err = "total scan-1 points per call must be < 2^31"; return ICET_ERR_UNSUPPORTED; }
    const bool grow_pairs = n_pairs > w.cap_pairs || V > w.cap_V;
    if (grow_pairs) {
        c->kf_pairs = 0;                       // the parked keyframe's tables (hotS / fitS / slot_of_voxel / n_slots) are about to be re-allocated
        const int np = n_pairs > w.cap_pairs ? n_pairs : w.cap_pairs;
        const int VV = V > w.cap_V ? V : w.cap_V;
        const size_t pv = (size_t)np * VV;
        BufferGroup& g = c->mem.pairs;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        w.cap_pairs = w.cap_V = c->h_cap_pairs = 0, w.cap_fit_items = 0, g.release();
        HIPCHK(c, g.device(w.desc, np));
        HIPCHK(c, g.device(w.seg_off, 2 * (size_t)np + 1));              // segment offsets, then (ragged throughput batches) the caller's pair of every slot
        HIPCHK(c, g.device(w.bin_count, pv));
        HIPCHK(c, g.device(w.bin_start, (size_t)np * (VV + 1)));
        HIPCHK(c, g.device(w.live_bins, pv * 4)); HIPCHK(c, g.device(w.n_live, np));
        HIPCHK(c, g.device(w.hotD, pv)); HIPCHK(c, g.device(w.fitD, pv)); HIPCHK(c, g.device(w.activeD, pv)); HIPCHK(c, g.device(w.midD, pv));
        HIPCHK(c, g.device(w.hotS, pv)); HIPCHK(c, g.device(w.fitS, pv));
        HIPCHK(c, g.device(w.slot_of_voxel, (size_t)np * ((VV + 1) & ~1)));
        HIPCHK(c, g.device(w.n_slots, np));
        HIPCHK(c, g.device(w.gn_part, (size_t)kGnPartWords));
        HIPCHK(c, g.device(w.flags, np));
        HIPCHK(c, g.device(w.zero_rows, (size_t)np * 4));
        HIPCHK(c, g.device(w.vrange, (size_t)np * 2));
        HIPCHK(c, g.device(w.splitters, (size_t)np * kRankSortMaxBuckets)); HIPCHK(c, g.device(w.n_buckets, np)); HIPCHK(c, g.device(w.bucket_start, (size_t)np * (kRankSortMaxBuckets + 1)));
        HIPCHK(c, g.pinned(c->h_desc, np));
        std::memset(c->h_desc, 0, sizeof(PairDesc) * np); c->desc_kf_valid = c->desc_reg_valid = false;
        HIPCHK(c, g.pinned(c->h_seg, 2 * (size_t)np + 1));
        c->h_cap_pairs = np;
        w.cap_pairs = np; w.cap_V = VV;
        c->ws_gen++;
    }
    { const icet_status rs = ensure_regs(c, n_pairs, V); if (rs != ICET_OK) return rs; }      // (the keyframe build clears the sums and overflow counts of its pairs)
    { const icet_status ss = ensure_scan2(c, total_n2); if (ss != ICET_OK) return ss; }
    if (total_n1 > w.cap_n1 || w.cap_fit_items == 0) {      // (cap_fit_items == 0: never built, the pair tables or scan-1 arrays moved, or its last growth was refused)
        c->ws_gen++;
        const int64_t n = total_n1 > w.cap_n1 ? total_n1 : w.cap_n1;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (n > w.cap_n1) {
            BufferGroup& g = c->mem.scan1;
            c->kf_pairs = 0;
            w.cap_n1 = 0, w.cap_fit_items = 0, g.release();
            HIPCHK(c, g.device(w.r1, n)); HIPCHK(c, g.device(w.cart1, (size_t)3 * n));
            HIPCHK(c, g.device(w.rs_pairs, n)); HIPCHK(c, g.device(w.rs_pairs_alt, n)); HIPCHK(c, g.device(w.bin16, n + 8));      /* (+ 8: k_rs_bucket_sort reads aligned groups of eight words) */ HIPCHK(c, g.device(w.binpos, n)); HIPCHK(c, g.device(w.bkt, n));
            HIPCHK(c, g.device(w.cand_row, n)); HIPCHK(c, g.device(w.cand_r, n)); HIPCHK(c, g.device(w.sorted_row, n)); HIPCHK(c, g.device(w.row_of_rank, n));
            HIPCHK(c, g.device(w.rank_of_row, n)); HIPCHK(c, g.device(w.src, n));
            w.cap_n1 = n;
        }
        // what depends on both sides; its capacity is cap_fit_items
        BufferGroup& g = c->mem.fit;
        const size_t need_items = (size_t)(w.cap_n1 / 64 + (int64_t)w.cap_pairs * (w.cap_V + 1) + 64);
        w.cap_fit_items = 0, g.release();
        HIPCHK(c, g.device(w.execbits, (size_t)(w.cap_n1 / 64 + w.cap_pairs + 2)));      // exec_word_base: off1 / 64 + pair
        HIPCHK(c, g.device_bytes(w.fit_items, need_items * 16));
        HIPCHK(c, g.device(w.fit_n_items, (size_t)w.cap_pairs));
        w.cap_fit_items = need_items;
    }
    return ICET_OK;
}

// thr[k] = smallest float32 whose reference bin index int((double)a / period * nb) (src/icet.cpp:545-546) is >= k.
void build_thresholds(int nb, double period, float* out) {
    auto bin = [&](float t) { return static_cast<long long>(((double)t / period) * nb); };
    out[0] = 0.f;
    for (int k = 1; k <= nb; k++) {
        float t = (float)(period * (double)k / (double)nb);
        while (bin(t) >= k) t = std::nextafterf(t, -INFINITY);
        while (bin(t) < k) t = std::nextafterf(t, INFINITY);
        out[k] = t;
    }
}

// Classification LUT over a monotone coordinate c in [lo, lo + range): M cells, each naming the edge nearest to its centre.
// M is the smallest power of two whose cells are narrower than 0.45 x a reference bin width -- the narrowest bin
// (quantile 0: azimuth, whose bins differ by 2x at most) or a low quantile of the widths (polar angle: in w = -cos(phi) the
// two bins at the poles are 15x narrower than those at the horizon, where the lidar's points are; sizing the table for them
// made it 8 KB of LDS and block start-up time for rows nobody visits).  A cell is usable by the fast path iff no OTHER edge
// lies between any of its points and the edge it names, nor within the guard band of the cell: then "compare with the named
// edge" yields the bin and "far from the named edge" implies far from every edge.  Cells that fail this (near the poles) get
// edge = NaN, which fails the kernel's guard test, so their points take the literal path.
struct HostCell { float edge; int32_t idx; };
int build_lut(const std::vector<double>& edges, double lo, double range, double quantile, double guard, std::vector<HostCell>& out, int max_cells = 1 << 16) {
    std::vector<double> widths;
    for (size_t k = 1; k < edges.size(); k++) widths.push_back(edges[k] - edges[k - 1]);
    std::sort(widths.begin(), widths.end());
    const double w_ref = widths.empty() ? range : widths[(size_t)(quantile * (double)(widths.size() - 1))];
    int M = 64;
    while (range / M > 0.45 * w_ref && 2 * M <= max_cells) M *= 2;     // (a cell that still holds two edges is marked ambiguous below: its points take the literal path)
    out.resize(M);
    const double cw = range / M, slack = 0.02 * cw + guard;      // the kernel's float cell index may be off by a rounding at a cell boundary
    for (int c = 0; c < M; c++) {
        const double ctr = lo + (c + 0.5) * cw;
        size_t best = 0;
        for (size_t k = 1; k < edges.size(); k++) if (std::fabs(edges[k] - ctr) < std::fabs(edges[best] - ctr)) best = k;
        const double e = edges[best];
        const double h0 = std::min(lo + c * cw - slack, e) - guard, h1 = std::max(lo + (c + 1) * cw + slack, e) + guard;
        bool ambiguous = false;
        for (size_t k = 0; k < edges.size(); k++) if (k != best && edges[k] >= h0 && edges[k] <= h1) ambiguous = true;
        out[c].edge = ambiguous ? std::nanf("") : (float)e; out[c].idx = (int32_t)best;
    }
    return M;
}

icet_status ensure_thresholds(icet_ctx* c, int T, int P) {
    Workspace& w = c->w;
    if (w.thr && w.thr_T == T && w.thr_P == P) return ICET_OK;
    BufferGroup& g = c->mem.lut;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    {
        // azimuth: diamond angle pa(theta) = y/(|x|+|y|) unfolded to [0,4]; polar: w = -cos(phi) in [-1,1]
        std::vector<double> et(T + 1), ep(P + 1);
        for (int k = 0; k <= T; k++) {
            const double th = 2 * M_PI * k / T, x = std::cos(th), y = std::sin(th), q = y / (std::fabs(x) + std::fabs(y));
            et[k] = (k == T) ? 4.0 : (k == 0 ? 0.0 : (x >= 0 ? (y >= 0 ? q : 4.0 + q) : 2.0 - q));
        }
        for (int k = 0; k <= P; k++) ep[k] = (k == 0) ? -1.0 : (k == P ? 1.0 : -std::cos(M_PI * k / P));
        // Guard bands: a few float ulps of the coordinate plus the ulp-level disagreement between the LUT's
        // true edges and the literal evaluation's float thresholds ("exact fast path").
        w.guard_t = 5e-6f * (float)c->tune.guard_scale; w.guard_p = 2.5e-6f * (float)c->tune.guard_scale;       // scale: experiments / tests only
        std::vector<HostCell> lt, lp;
        const double qp = c->tune.lut_polar_quantile;
        // Both tables live in the LDS of k_scan1_spherical and k_gn_accumulate blocks next to the voxel map.  A grid that is extremely fine in ONE direction
        // (thousands of azimuth bins on one ring) would want more cells than fit: the tables are then capped -- coarser cells hold two edges, are marked
        // ambiguous and send their points through the literal formulas: slower, same result -- and only a grid whose MINIMUM does not fit is refused.
        int cap_t = 1 << 16, cap_p = 1 << 16, Mt = 0, Mp = 0;
        for (;;) {
            Mt = build_lut(et, 0.0, 4.0, 0.0, w.guard_t, lt, cap_t); Mp = build_lut(ep, -1.0, 2.0, qp, w.guard_p, lp, cap_p);
            const size_t need_acc = acc_fixed_lds_bytes(T, P, Mt, Mp, true) + 32 * acc_row_lds_bytes();
            const size_t need_scan1 = (size_t)(Mt + Mp + 2) * sizeof(HostCell) + 4096;      // + the kernel's static tables (init_keyframe_kernels)
            if (std::max(need_acc, need_scan1) <= (size_t)c->max_lds) break;
            if (Mt <= 64 && Mp <= 64) { c->err = "grid too fine for this device's LDS (voxel map + look-up tables of one block)"; return ICET_ERR_UNSUPPORTED; }
            if (Mt >= Mp) cap_t = Mt / 2; else cap_p = Mp / 2;
        }
        // one spare cell per table: pa == 4 / w == 1 index cell M (it names the last edge, so the point goes to the literal path)
        for (HostCell& c : lp) c.idx *= T;                                 // polar cells carry the map row offset T * edge index
        std::vector<HostCell> all(lt); all.push_back(HostCell{4.0f, T}); all.insert(all.end(), lp.begin(), lp.end()); all.push_back(HostCell{1.0f, P * T});
        w.thr_T = w.thr_P = 0, g.release();                                // (a grid refused above keeps the tables of the last one)
        HIPCHK(c, g.device_bytes(w.lut, all.size() * sizeof(HostCell)));
        HIPCHK(c, hipMemcpy(w.lut, all.data(), all.size() * sizeof(HostCell), hipMemcpyHostToDevice));
        w.lut_Mt = Mt; w.lut_Mp = Mp;
        // the same edges as floats, for the keep masks of the point pass (margins of 1e-2 rad: the float rounding of an edge is far inside their slack)
        std::vector<float> ef; for (double e : et) ef.push_back((float)e); for (double e : ep) ef.push_back((float)e);
        HIPCHK(c, g.device(w.edges, ef.size()));
        HIPCHK(c, hipMemcpy(w.edges, ef.data(), ef.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    std::vector<float> h((size_t)T + P + 2);
    build_thresholds(T, 2 * M_PI, h.data());
    build_thresholds(P, M_PI, h.data() + T + 1);
    HIPCHK(c, g.device(w.thr, h.size()));
    HIPCHK(c, hipMemcpy(w.thr, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    // the voxel of an exact-zero row, by the sign bits of (y, x): r = 0, phi = acos(NaN) -> 1000, theta = atan2(+-0, +-0) (src/utils.cpp:103-116) binned as
    // sortSphericalCoordinates bins them (src/icet.cpp:545-546) -- the formulas of theta_cr / phi_cr / voxel_of (icet_device_common.h) in host arithmetic
    for (int k = 0; k < 4; k++) {
        float th = (float)std::atan2((k & 2) ? -0.0 : 0.0, (k & 1) ? -0.0 : 0.0);
        if (th < 0.0f) th = (float)((double)th + 2.0 * M_PI);
        const float ph = 1000.0f;
        const int bt = static_cast<int>(((double)th / (2.0 * M_PI)) * (double)T) % T, bp = static_cast<int>(((double)ph / M_PI) * (double)P) % P;
        w.zero_voxel[k] = T * bp + bt;
    }
    w.thr_T = T; w.thr_P = P;
    return ICET_OK;
}

icet_status ensure_out(icet_ctx* c, int32_t n_pairs) {
    if (n_pairs <= c->cap_out_pairs) return ICET_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    BufferGroup& g = c->mem.out;
    HIPCHK(c, grow(g, c->cap_out_pairs, n_pairs, [&] {
        int e = g.device(c->d_out, (size_t)n_pairs * 48);
        if (!e) e = g.device(c->d_x0, (size_t)n_pairs * 6);
        if (!e) e = g.pinned(c->h_out, (size_t)n_pairs * 48);
        if (!e) e = g.pinned(c->h_x0, (size_t)n_pairs * 6);
        return e;
    }));
    return ICET_OK;
}

// The copy stream of the host-pointer entry points and its event (created on first use).
// Uploads go through the runtime's own pageable path, one hipMemcpy2DAsync per scan: measured on the GPU box (profiles/r04_stage_probe.txt,
// scripts/hip/stage_probe.hip) it moves a 1.45 MB scan in 35 us (41 GB/s), as fast as from pinned memory; a ring of pinned chunks filled by
// copy threads -- built first -- was 3-4x SLOWER (every chunk's DMA command costs ~10 us, and this host copies 50 GB/s on one thread).
// What made the round-3 constructor path slow were the thirteen D2H copies into pageable arrays and the host loop for `points2`, not the upload.
icet_status ensure_host_path(icet_ctx* c) {
    if (!c->st_copy) HIPCHK(c, hipStreamCreateWithFlags(&c->st_copy, hipStreamNonBlocking));
    for (hipEvent_t* e : {&c->ev_s2, &c->ev_kf, &c->ev_kfd, &c->ev_prev, &c->ev_pts2})
        if (!*e) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    return ICET_OK;
}

// Column-major N x 3 host scan (leading dimension ld) -> staging buffer (leading dimension l) on `st`.
hipError_t upload_scan(float* dst, int64_t l, const float* src, int64_t n, int64_t ld, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    return hipMemcpy2DAsync(dst, l * sizeof(float), src, ld * sizeof(float), n * sizeof(float), 3, hipMemcpyHostToDevice, st);
}
// `count` dense host scans (ld == n) into the places stage_layout gave them, on `st`.
hipError_t upload_staged(const icet_dev_scan* d, const float* const* scan, int32_t count, hipStream_t st) {
    for (int k = 0; k < count; k++) {
        const hipError_t e = upload_scan(const_cast<float*>(d[k].ptr), d[k].ld, scan[k], d[k].n, d[k].n, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// n x 6 start poses through the pinned copy (ensure_out sized both); null stays null.
icet_status stage_x0(icet_ctx* c, const float* x0, int32_t n, const float** d_x0) {
    *d_x0 = nullptr;
    if (!x0) return ICET_OK;
    std::memcpy(c->h_x0, x0, sizeof(float) * 6 * n);
    HIPCHK(c, hipMemcpyAsync(c->d_x0, c->h_x0, sizeof(float) * 6 * n, hipMemcpyHostToDevice, c->stream));
    *d_x0 = c->d_x0;
    return ICET_OK;
}

// (p + t) * R over a column-major scan (src/icet.cpp:375-378) with the device's own t and R (the transform record of write_xf): the host
// half of `points2`.  Plain float arithmetic; the AVX2 + FMA build of the same loop is taken when the CPU has it.
#define ICET_POINTS2_BODY                                                                                                     \
    const float tx = xf[0], ty = xf[1], tz = xf[2];                                                                           \
    const float R00 = xf[3], R01 = xf[4], R02 = xf[5], R10 = xf[6], R11 = xf[7], R12 = xf[8], R20 = xf[9], R21 = xf[10], R22 = xf[11]; \
    const float* __restrict__ px = s; const float* __restrict__ py = s + ld; const float* __restrict__ pz = s + 2 * ld;      \
    float* __restrict__ ox = out; float* __restrict__ oy = out + n; float* __restrict__ oz = out + 2 * n;                    \
    for (int64_t i = 0; i < n; i++) {                                                                                         \
        const float a = px[i] + tx, b = py[i] + ty, c = pz[i] + tz;                                                           \
        ox[i] = a * R00 + b * R10 + c * R20; oy[i] = a * R01 + b * R11 + c * R21; oz[i] = a * R02 + b * R12 + c * R22;       \
    }
#if defined(__x86_64__)
__attribute__((target("avx2,fma"))) void host_points2_avx2(const float* xf, const float* s, int64_t ld, int64_t n, float* out) { ICET_POINTS2_BODY }
#endif
void host_points2(const float* xf, const float* s, int64_t ld, int64_t n, float* out) {
#if defined(__x86_64__)
    if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) { host_points2_avx2(xf, s, ld, n, out); return; }
#endif
    ICET_POINTS2_BODY
}
#undef ICET_POINTS2_BODY

// Word offsets (4-byte words, every table 16-byte aligned) of the single-pair result block, which exists twice with one layout: in HBM
// (d_pack) and in pinned host memory (h_pack).  [0, small_end): the 48 result floats and the per-iteration 6 / 36 / 6-float tables, written
// in HBM and copied in ONE small D2H behind the loop (written straight into pinned memory by k_gn_solve they cost every iteration a PCIe
// round trip at its end: measured on the map maker, +6 us per iteration); xf_last: the transform record of the last iteration (for
// `points2`), written ONCE, straight into the pinned copy; [bounds, kf_end): the keyframe tables, final once the keyframe is built, copied to
// the host on the copy stream while the loop runs; then the rarely requested integer tables (copied at the end).
struct AuxLayout { size_t out, xf_last, x_hist, htwh, htwdz, cond, small_end, bounds, has_fit, mu1, sigma1, evecs1, l_diag, test_points, kf_end, n1_raw, n2_raw, n2_in, ints_end, total; };
AuxLayout aux_layout(int V, int runlen) {
    AuxLayout L{}; size_t o = 0;
    auto take = [&o](size_t n) { const size_t at = o; o += (n + 3) & ~(size_t)3; return at; };
    const size_t rl = runlen > 0 ? runlen : 1, v = (size_t)V;
    L.out = take(48); L.x_hist = take(rl * 6); L.htwh = take(rl * 36); L.htwdz = take(rl * 6); L.cond = take(rl * 8); L.small_end = o; L.xf_last = take(48);
    L.bounds = take(v * 6); L.has_fit = take(v); L.mu1 = take(v * 3); L.sigma1 = take(v * 9); L.evecs1 = take(v * 9); L.l_diag = take(v * 3);
    L.test_points = take(v * 18); L.kf_end = o; L.n1_raw = take(v); L.n2_raw = take(rl * v); L.n2_in = take(rl * v); L.ints_end = o;
    L.total = o;
    return L;
}

// Device and pinned host copies of the result block for (V, runlen); c->aux_dev points into the device block.
icet_status ensure_pack(icet_ctx* c, int V, int runlen) {
    const AuxLayout L = aux_layout(V, runlen);
    if (L.total > c->cap_pack) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->aux_dev = AuxDev{}; c->aux_V = 0; c->aux_runlen = 0;
        BufferGroup& g = c->mem.pack;
        HIPCHK(c, grow(g, c->cap_pack, L.total, [&] { const int e = g.device(c->d_pack, L.total); return e ? e : g.pinned(c->h_pack, L.total); }));
    }
    if (c->aux_V != V || c->aux_runlen != runlen) {
        AuxDev& a = c->aux_dev; uint32_t* d = c->d_pack;
        auto F = [d](size_t at) { return reinterpret_cast<float*>(d + at); };
        auto I = [d](size_t at) { return reinterpret_cast<int32_t*>(d + at); };
        float* hs = reinterpret_cast<float*>(c->h_pack);                     // pinned host memory is device-accessible under the same address
        a.bounds = F(L.bounds); a.n1_raw = I(L.n1_raw); a.has_fit = I(L.has_fit); a.mu1 = F(L.mu1); a.sigma1 = F(L.sigma1); a.evecs1 = F(L.evecs1);
        a.l_diag = F(L.l_diag); a.x_hist = F(L.x_hist); a.htwh = F(L.htwh); a.htwdz = F(L.htwdz); a.cond = F(L.cond); a.n2_raw = I(L.n2_raw); a.n2_in = I(L.n2_in);
        a.test_points = F(L.test_points); a.xf_last = hs + L.xf_last;
        c->aux_V = V; c->aux_runlen = runlen;
    }
    return ICET_OK;
}

// The solve in two halves, so that a sequential caller can build the keyframe of a scan while the previous pair is still iterating
// (icet_keyframe_device / icet_register_device): enqueue_keyframe = ICET::fitScan1 (src/icet.cpp:68-107) for the scan-1 halves of the
// descriptors in c->h_desc[0..n_pairs), enqueue_loop = prepScan2 + runlen x fitScan2 (:254-277, :372-436) for their scan-2 halves
// against the tables the keyframe left in the workspace.
// THE PLAN of a call: its launch configuration, from the parameters, the options and the totals of the staging the call has laid out (lay_out_staging,
// icet_staging.h).  Pure: computed once per call -- behind ensure_thresholds, whose table sizes the keep list's LDS test reads -- and handed to the graph key and the enqueuers.
LaunchCfg make_cfg(const icet_ctx* c, const icet_params* p, int32_t n_pairs, const StagingTotals& t) {
    LaunchCfg cfg{};
    cfg.T = p->bins_theta; cfg.P = p->bins_phi; cfg.V = cfg.T * cfg.P; cfg.n = p->n; cfg.runlen = p->runlen;
    cfg.thresh = p->thresh; cfg.buff = p->buff; cfg.n_pairs = n_pairs;
    cfg.half_gap = (p->flags & ICET_FLAG_HALF_GAP_BOUNDS) ? 1 : 0;
    cfg.true_sort = (p->flags & (ICET_FLAG_TRUE_SORT | ICET_FLAG_HALF_GAP_BOUNDS)) ? 1 : 0;
    cfg.reject_moving = (p->flags & ICET_FLAG_REJECT_MOVING) ? 1 : 0;
    cfg.rt2 = (p->flags & ICET_FLAG_ROUNDTRIP_SCAN2) ? 1 : 0;
    cfg.ref_w = (p->flags & ICET_FLAG_DOUBLE_W) ? 0 : 1;
    cfg.lds_slots = c->tune.lds_slots; cfg.acc_min_pts_per_thread = c->tune.acc_pts; cfg.acc_target_blocks = c->tune.acc_blocks;
    cfg.force_exact = c->tune.force_exact; cfg.kf_pts_per_thread = c->tune.kf_pts; cfg.rs_cap = c->tune.rs_cap; cfg.rs_max_cell = c->tune.rs_max_cell; cfg.exec_bits_lds = c->tune.exec_bits_lds; cfg.exec_pairwise = c->tune.exec_pairwise; cfg.fuse_solve = c->tune.fuse_solve != 0 ? 1 : 0; cfg.lds_rank = (c->tune.lds_rank != 0 && c->lds_rank_ok) ? 1 : 0;
    cfg.gn_cond_bound2 = (float)(c->tune.gn_cond_bound * c->tune.gn_cond_bound);
    cfg.pair_user = (c->perm_active && c->perm_pairs == n_pairs) ? c->w.seg_off + n_pairs + 1 : nullptr;
    cfg.done_flag = c->done_flag;
    // the keep list of the point pass (KeepState, icet_internal.h): throughput batches only -- a small batch's point pass is a few microseconds of launch floor --,
    // never with the scan-2 round trip (a kernel of its own) nor when fewer than two passes could walk a list; same bits either way
    cfg.keep_from = c->tune.keep_from < 0 ? 0 : c->tune.keep_from; cfg.keep_bt = (float)c->tune.keep_budget_t; cfg.keep_br = (float)c->tune.keep_budget_r; cfg.keep_check_scale = (float)c->tune.keep_check_scale;
    cfg.keep = (c->tune.keep != 0 && n_pairs >= 32 && !cfg.rt2 && p->runlen >= cfg.keep_from + 3 && c->w.lut_Mt > 0 &&
                acc_fixed_lds_bytes(cfg.T, cfg.P, c->w.lut_Mt, c->w.lut_Mp, false, true) + 64 * acc_row_lds_bytes() <= (size_t)c->max_lds) ? 1 : 0;
    if (cfg.kf_pts_per_thread > kKfMaxPtsPerThread) cfg.kf_pts_per_thread = kKfMaxPtsPerThread;      // k_bin_scatter: a tile is at most 4 waves x that many rounds x 64 positions
    if (cfg.kf_pts_per_thread < 1) cfg.kf_pts_per_thread = 1;
    cfg.stage_event = c->stage_at ? c->ev_stage : nullptr; cfg.stage_at = c->stage_at;
    cfg.vec4_ok = t.vec4_ok; cfg.total_n1 = t.total_n1; cfg.max_n1 = t.max_n1; cfg.max_n2 = t.max_n2;
    const int mx1 = t.max_n1;
    // A small batch of ordinary scans leaves most CUs without a keyframe tile at the full tile size (one 120 k-row scan: 59 tiles on 256 CUs): half-size tiles
    // then (measured, single pair: keyframe 0.170 -> 0.160 ms; a 485 k-row scan keeps the full size: 0.29 vs 0.31).  Same bits either way.
    if (cfg.kf_pts_per_thread == kKfMaxPtsPerThread && kKfMaxPtsPerThread >= 8 && (int64_t)n_pairs * ((mx1 + 256 * kKfMaxPtsPerThread - 1) / (256 * kKfMaxPtsPerThread)) < 128)
        cfg.kf_pts_per_thread = kKfMaxPtsPerThread / 2;
    cfg.kf_chunks = (mx1 + 256 * cfg.kf_pts_per_thread - 1) / (256 * cfg.kf_pts_per_thread);
    if (cfg.kf_chunks < 1) cfg.kf_chunks = 1;
    // packed rows (LaunchCfg::packed_rows): the layout of pred[] / src[] for this call -- whenever the largest rank and a voxel word fit 32 bits together
    // (17 + 13 on 75 x 24 with scans up to 131 072 rows), unless the option says no
    cfg.row_shift = packed_row_shift(mx1); cfg.id_bits = bits_of((int64_t)cfg.V - 1);
    cfg.packed_rows = (c->tune.packed_rows != 0 && packed_row_bits(mx1, cfg.V) <= 32) ? 1 : 0;
    return cfg;
}
// The plan's part of a graph key (icet_ctx::GraphKey::launch): what grids, LDS sizes, template choices and by-value arguments are made from.  Not in it: what an
// option's setter un-sees the keys for (fuse_solve, gn_cond_bound) and what no captured call uses (the keep list, batch stages).
void launch_key_of(const LaunchCfg& k, int64_t (&out)[29]) {
    auto bits = [](float f) { int32_t i; std::memcpy(&i, &f, 4); return (int64_t)i; };
    const int64_t v[] = {k.T, k.P, k.V, k.n, k.runlen, bits(k.thresh), bits(k.buff), k.n_pairs, k.max_n1, k.max_n2, k.total_n1, k.lds_slots, k.acc_min_pts_per_thread,
                         k.acc_target_blocks, k.kf_chunks, k.kf_pts_per_thread, k.vec4_ok, k.true_sort, k.force_exact, k.rs_cap, k.rs_max_cell,
                         k.exec_bits_lds, k.exec_pairwise, k.lds_rank, k.reject_moving, k.half_gap, k.rt2, k.ref_w, k.packed_rows};
    static_assert(sizeof(v) == sizeof(out), "GraphKey::launch");
    std::memcpy(out, v, sizeof(v));
}

// The plan of a call over the pair staging (h_desc / h_seg), which the caller has finished writing: thresholds, layout, launch configuration -- in that order.
icet_status plan_pairs(icet_ctx* c, const icet_params* p, int32_t n_pairs, LaunchCfg* cfg) {
    ICET_TRY(ensure_thresholds(c, p->bins_theta, p->bins_phi));
    *cfg = make_cfg(c, p, n_pairs, lay_out_staging(c->h_desc, c->h_seg, n_pairs));
    return ICET_OK;
}

icet_status enqueue_keyframe(icet_ctx* c, const LaunchCfg& cfg, const AuxDev* aux, const int32_t* d_counts1 = nullptr) {
    Workspace& w = c->w;
    const int32_t n_pairs = cfg.n_pairs;
    if (c->tune.packed_rows > 0 && !cfg.packed_rows) {
        c->err = "option \"packed_rows\" is 1, but a rank and a voxel word of this call do not fit 32 bits together (" + std::to_string(packed_row_bits(cfg.max_n1, cfg.V)) + " bits)";
        return ICET_ERR_UNSUPPORTED;
    }
    c->kf_row_mask = packed_row_mask(cfg);
    {
        const size_t need = (size_t)n_pairs * cfg.kf_chunks * (cfg.V > kRankSortMaxBuckets ? cfg.V : kRankSortMaxBuckets);
        if (need > w.cap_counts) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            BufferGroup& g = c->mem.counts;
            HIPCHK(c, grow(g, w.cap_counts, need, [&] { const int e = g.device(w.counts, need); return e ? e : g.device(w.tile_base, need); }));
        }
        const size_t need_vr = (size_t)n_pairs * cfg.kf_chunks * 2;        // (its own capacity: tiles per voxel count vary with the grid)
        if (need_vr > w.cap_tile_vr) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, grow(c->mem.tile_vr, w.cap_tile_vr, need_vr, [&] { return c->mem.tile_vr.device(w.tile_vr, need_vr); }));
        }
    }
    // a small batch: k_rs_splitters, the keyframe's first kernel, takes the descriptors from the pinned staging itself
    const bool first_uploads = n_pairs <= kUploadDescMaxPairs;
    ICET_TRY(staging_upload(c, w, c->h_desc, c->h_seg, n_pairs, (size_t)n_pairs + 1 + (c->perm_active ? n_pairs : 0), first_uploads));      // (a permuted batch carries the caller's pair of every slot behind the offsets)
    if (!first_uploads) ICET_TRY(staging_mark_read(c));
    if (!c->capturing) HIPCHK(c, hipEventRecord(c->ev_a, c->stream));
    LaunchCfg kcfg = cfg; if (first_uploads) { kcfg.h_desc_up = c->h_desc; kcfg.h_seg_up = c->h_seg; }
    HIPCHK(c, launch_keyframe(w, kcfg, aux, c->stream, d_counts1));      // (d_counts1: the descriptors hold upper bounds, the device knows the row counts: patched by the first kernel)
    if (first_uploads) ICET_TRY(staging_mark_read(c));                    // (the staging has been read once these kernels have run)
    return ICET_OK;
}

// ICET_FLAG_ROUNDTRIP_SCAN2: the round-tripped copy of the scan 2s that the host descriptors `hd` name -- and `wl.desc` on the device, which the
// pre-pass reads --; on return wl's descriptors are the copy's (wl.desc = w.desc_rt), and lcfg says that the copy is 64-float aligned whatever the caller's layout was.
icet_status enqueue_rt2(icet_ctx* c, LaunchCfg& lcfg, int32_t n_pairs, const PairDesc* hd, Workspace& wl, hipEvent_t scan2_ready) {
    Workspace& w = c->w;
    int64_t tot = 0;
    for (int k = 0; k < n_pairs; k++) tot += padded_ld(hd[k].n2);
    if (tot > w.cap_rt2 || !w.desc_rt || n_pairs > c->h_cap_rt) {
        HIPCHK(c, hipStreamSynchronize(c->stream)); staging_idle(c);
        if (tot > w.cap_rt2) HIPCHK(c, grow(c->mem.rt2, w.cap_rt2, tot, [&] { return c->mem.rt2.device(w.rt2, (size_t)3 * tot); }));
        if (n_pairs > c->h_cap_rt || !w.desc_rt) {
            const int np = n_pairs > w.cap_pairs ? n_pairs : w.cap_pairs;
            BufferGroup& g = c->mem.rt_desc;
            HIPCHK(c, grow(g, c->h_cap_rt, np, [&] { const int e = g.device(w.desc_rt, np); return e ? e : g.pinned(c->h_desc_rt, np); }));
        }
    }
    ICET_TRY(staging_wait(c));
    int64_t o = 0;
    for (int k = 0; k < n_pairs; k++) {
        const int64_t l = padded_ld(hd[k].n2);
        PairDesc dr = hd[k];
        dr.s2 = w.rt2 + 3 * o; dr.ld2 = (int32_t)l;
        c->h_desc_rt[k] = dr; o += l;
    }
    HIPCHK(c, hipMemcpyAsync(w.desc_rt, c->h_desc_rt, sizeof(PairDesc) * n_pairs, hipMemcpyHostToDevice, c->stream));
    ICET_TRY(staging_mark_read(c, true));                                 // (never captured: graph_eligible refuses the round trip)
    if (scan2_ready) HIPCHK(c, hipStreamWaitEvent(c->stream, scan2_ready, 0));
    wl.desc_rt = w.desc_rt; wl.rt2 = w.rt2; wl.cap_rt2 = w.cap_rt2;
    HIPCHK(c, launch_rt2_prepare(wl, lcfg, c->stream));
    wl.desc = w.desc_rt; lcfg.vec4_ok = 1;
    return ICET_OK;
}

// One call of the Gauss-Newton loop: what enqueue_loop, the ONE function that enqueues it, is told.  Two kinds of caller fill it: the pair entries (pair_loop,
// below: the whole solve, icet_register_device_n, the host-pointer entries) and the indexed registrations (register_indexed: registration r against the keyframe
// tables of kf_of[r]; the registration-side tables -- acc, xf, X, overflow counts, tickets -- are indexed by r).
enum LoopTail { kTailNone, kTailScore, kTailDump, kTailTerms };
struct LoopCall {
    // the staging the loop reads -- h_desc / h_seg, or h_desc_reg / h_kf_of (k_init_state / k_upload_desc copy the keyframe index as their "segment" table) --, the
    // words of its segment table, and whether it goes up HERE (false: it went up with the keyframe, earlier in this call)
    PairDesc* hd = nullptr; int32_t* hs = nullptr; size_t seg_words = 0; bool upload = false;
    // what the loop's kernels see of the workspace: the keyframe tables of the context or of a store, desc or desc_reg; kf_of: set for an indexed call (LaunchCfg::kf_of)
    Workspace view; const int32_t* kf_of = nullptr;
    const float* d_x0 = nullptr; float* d_out = nullptr; const AuxDev* aux = nullptr; int iters = 0;
    // known to the DEVICE only: the scan-2 row counts (the descriptors hold upper bounds, which size the launches; k_init_state clamps them, or k_patch_counts in
    // front of the scan-2 round trip) and, for a loop-closure query, the keyframe index (copied over the staged one behind k_init_state)
    const int32_t* d_rows = nullptr; const int32_t* d_kf_of = nullptr;
    hipEvent_t scan2_ready = nullptr;      // host-pointer entries: scan 2 was uploaded on the copy stream beside the keyframe build
    float* pts2_out = nullptr;             // the device computes `points2` into this (else only the transform snapshot + its event: the host does)
    // plain: the plain point pass and solve -- no fused launch, no keep list, no pair_user, no done_flag (an indexed call: launch_gn_accumulate refuses the rest with kf_of)
    // own_timing: no keyframe build in this call, keyframe_ms = 0: ev_a is recorded here too.  An indexed call.  (icet_register_device_n leaves ev_a where its keyframe
    // call recorded it: its keyframe_ms runs from there.)
    // init_on_copy: under the scan-2 round trip k_init_state sees the descriptors of the round-tripped copy and clamps THEIR counts to d_rows.  An indexed call.  The pair
    // entries hand it the caller's descriptors and no rows (k_patch_counts has clamped those): the copy's descriptors keep the bounds of the host staging, and the loop
    // reads the copy up to them (tests/test_halves_device_rows.py pins that as it is).
    bool plain = false, own_timing = false, init_on_copy = false;
    // behind the loop: one more point pass at the final transform records (the last solve, or k_init_state, left them in w.xf), then the score, the raw sums in
    // place of it (d_dump), or the terms (d_dump and terms: enqueue_terms_tail)
    LoopTail tail = kTailNone; icet_score* d_score = nullptr; uint32_t* d_dump = nullptr; const GnTermsOut* terms = nullptr;
};
// The loop of a pair entry over h_desc / h_seg and the context's own tables, with every launch feature the plan allows.
LoopCall pair_loop(icet_ctx* c, const LaunchCfg& cfg, const float* d_x0, float* d_out, const AuxDev* aux, bool upload, hipEvent_t scan2_ready = nullptr) {
    LoopCall L;
    L.hd = c->h_desc; L.hs = c->h_seg; L.seg_words = (size_t)cfg.n_pairs + 1 + (c->perm_active ? cfg.n_pairs : 0); L.upload = upload;      // (a permuted batch carries the caller's pair of every slot behind the offsets)
    L.view = c->w; L.d_x0 = d_x0; L.d_out = d_out; L.aux = aux; L.iters = cfg.runlen; L.scan2_ready = scan2_ready;
    return L;
}

// The tail of icet_debug_gn_terms_device: the point pass, the raw records copied out and left in place, the transform record, then the production solve of
// iteration runlen - 1 on those records.  Synchronises (its scratch is freed at return).
icet_status enqueue_terms_tail(icet_ctx* c, const icet_params* p, const Workspace& wl, const LaunchCfg& lcfg, const LoopCall& L) {
    // the solve writes its sums at [registration][iteration] of arrays sized for the whole run: a scratch of that shape, and the rows of iteration runlen - 1 copied out
    const int it = p->runlen - 1, n_regs = lcfg.n_pairs;
    const size_t row = (size_t)p->runlen * 42;
    float* d_tmp = nullptr; BufferGroup g;
    HIPCHK(c, g.device(d_tmp, row * (size_t)n_regs));
    auto body = [&]() -> icet_status {
        HIPCHK(c, launch_gn_accumulate(wl, lcfg, c->stream));
        HIPCHK(c, launch_point_sums_copy(wl, lcfg, L.d_dump, c->stream));     // drains the overflow list; the records stay
        HIPCHK(c, hipMemcpyAsync(L.terms->xf, c->w.xf, sizeof(float) * 48 * (size_t)n_regs, hipMemcpyDeviceToDevice, c->stream));      // (before the solve replaces it with the next iteration's)
        AuxDev aux{};
        aux.htwh = d_tmp; aux.htwdz = d_tmp + (size_t)n_regs * p->runlen * 36;
        HIPCHK(c, launch_gn_solve(wl, lcfg, it, L.d_out, &aux, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(L.terms->htwh, 36 * sizeof(float), aux.htwh + (size_t)it * 36, (size_t)p->runlen * 36 * sizeof(float), 36 * sizeof(float), n_regs, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(L.terms->htwdz, 6 * sizeof(float), aux.htwdz + (size_t)it * 6, (size_t)p->runlen * 6 * sizeof(float), 6 * sizeof(float), n_regs, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return ICET_OK;
    };
    const icet_status ts = body();
    if (ts != ICET_OK) (void)hipStreamSynchronize(c->stream);
    return ts;
}

// prepScan2 + iters x fitScan2 (src/icet.cpp:254-277, :372-436) + the tail, for the call L under the plan `plan`, whose staging is laid out.
icet_status enqueue_loop(icet_ctx* c, const icet_params* p, const LaunchCfg& plan, const LoopCall& L) {
    const int32_t n = plan.n_pairs;
    const bool want_pts2 = L.aux && L.aux->xf_last && p->runlen > 0;
    LaunchCfg cfg = plan; cfg.kf_of = L.kf_of;
    if (L.plain) { cfg.pair_user = nullptr; cfg.done_flag = nullptr; cfg.keep = 0; cfg.fuse_solve = 0; }
    Workspace& w = c->w;
    Workspace wl = L.view;                               // what the loop kernels see: with ICET_FLAG_ROUNDTRIP_SCAN2 their scan 2 is the round-tripped copy
    // A small batch without the scan-2 round trip or the keep list: k_init_state, the first kernel below that reads a descriptor, copies the staging itself (a replayed
    // graph re-reads it then).  Otherwise it goes up in front, and the mark behind it is never skipped for a capture: a graph holds small batches without the round trip only.
    const bool init_uploads = L.upload && n <= kUploadDescMaxPairs && !cfg.rt2 && !cfg.keep;
    if (L.upload) ICET_TRY(staging_upload(c, wl, L.hd, L.hs, n, L.seg_words, init_uploads));
    if (L.upload && !init_uploads) ICET_TRY(staging_mark_read(c));
    while ((int)c->ev_acc.size() < 2 * p->runlen) { hipEvent_t e; HIPCHK(c, hipEventCreate(&e)); c->ev_acc.push_back(e); }      // the per-iteration timing events
    if (L.own_timing && !c->capturing) HIPCHK(c, hipEventRecord(c->ev_a, c->stream));
    if (!c->capturing) HIPCHK(c, hipEventRecord(c->ev_b, c->stream));      // keyframe_ms ends here: the scan-2 pre-pass of ICET_FLAG_ROUNDTRIP_SCAN2 belongs to the loop
    LaunchCfg lcfg = cfg;
    if (cfg.rt2 && L.d_rows) HIPCHK(c, launch_patch_counts(wl, cfg, nullptr, L.d_rows, c->stream));      // (the pre-pass reads the counts of the caller's descriptors; otherwise k_init_state patches them)
    if (cfg.rt2) ICET_TRY(enqueue_rt2(c, lcfg, n, L.hd, wl, L.scan2_ready));
    if (cfg.keep) {                                          // masks, list and per-pair state of the keep list (grown here: only throughput batches use them)
        int64_t tot2 = 0; for (int k = 0; k < n; k++) tot2 += L.hd[k].n2;
        const size_t need_mask = (size_t)(tot2 >> 8) + (size_t)n + 2, need_list = (size_t)(tot2 >> 2) + (size_t)n + 4;
        if (need_mask > w.cap_keep_mask || need_list > w.cap_keep_list || n > w.cap_keep_pairs) {
            if (c->capturing) { c->err = "keep list: workspace growth during capture"; return ICET_ERR_HIP; }
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (need_mask > w.cap_keep_mask) HIPCHK(c, grow(c->mem.keep_mask, w.cap_keep_mask, need_mask, [&] { return c->mem.keep_mask.device(w.keep_mask, need_mask); }));
            if (need_list > w.cap_keep_list) HIPCHK(c, grow(c->mem.keep_list, w.cap_keep_list, need_list, [&] { return c->mem.keep_list.device(w.keep_list, need_list); }));
            if (n > w.cap_keep_pairs) {
                BufferGroup& g = c->mem.keep_pairs;
                HIPCHK(c, grow(g, w.cap_keep_pairs, n, [&] { const int e = g.device(w.keep_state, (size_t)n); return e ? e : g.device(w.keep_modes, 2 * (size_t)n); }));
            }
            wl.keep_modes = w.keep_modes; wl.keep_mask = w.keep_mask; wl.keep_list = w.keep_list; wl.keep_state = w.keep_state; wl.cap_keep_mask = w.cap_keep_mask; wl.cap_keep_list = w.cap_keep_list; wl.cap_keep_pairs = w.cap_keep_pairs;
        }
    }
    // k_init_state: of the workspace it reads the descriptors, X, xf, the tickets and the keep state; of the plan n_pairs, keep and pair_user, which the round trip leaves alone
    Workspace wi = wl; const int32_t* rows = L.d_rows;
    if (cfg.rt2 && !L.init_on_copy) { wi.desc = L.view.desc; rows = nullptr; }
    HIPCHK(c, launch_init_state(wi, lcfg, L.d_x0, c->stream, want_pts2 ? L.aux->xf_last : nullptr, rows, init_uploads ? L.hd : nullptr, init_uploads ? L.hs : nullptr));
    if (L.d_kf_of) HIPCHK(c, launch_closure_apply(w.kf_of, L.d_kf_of, n, c->stream));
    if (init_uploads) ICET_TRY(staging_mark_read(c));                     // (the staging is read by THIS kernel)
    // `points2` (include/icet.h:80): scan 2 as the LAST fitScan2 transforms it (src/icet.cpp:375-378).  That transform is known as soon as the
    // solve of iteration runlen - 2 has run: k_gn_solve / k_init_state snapshot its record in aux->xf_last (pinned host memory) and ev_prev
    // marks the moment.  icet_solve_end then transforms scan 2 ON THE HOST while the last iteration still runs on the device (measured: a
    // device kernel + 1.45 MB D2H + the copy into the caller's pageable array cost 110 us behind the loop, the host pass ~25 us under it).
    // Only with ICET_FLAG_ROUNDTRIP_SCAN2, whose points2_OG exists on the device alone, the device computes it (copy stream).
    auto enqueue_points2 = [&]() -> icet_status {
        HIPCHK(c, hipEventRecord(c->ev_prev, c->stream));
        if (!L.pts2_out) return ICET_OK;
        HIPCHK(c, hipStreamWaitEvent(c->st_copy, c->ev_prev, 0));
        HIPCHK(c, launch_points2(wl, lcfg, L.aux->xf_last, c->d_pts2, c->st_copy));
        HIPCHK(c, hipMemcpyAsync(L.pts2_out, c->d_pts2, sizeof(float) * 3 * (size_t)L.hd[0].n2, hipMemcpyDeviceToHost, c->st_copy));
        HIPCHK(c, hipEventRecord(c->ev_pts2, c->st_copy));
        return ICET_OK;
    };
    if (L.scan2_ready && !cfg.rt2) HIPCHK(c, hipStreamWaitEvent(c->stream, L.scan2_ready, 0));      // (with the round trip its pre-pass has waited: enqueue_rt2)
    if (want_pts2 && p->runlen == 1) ICET_TRY(enqueue_points2());
    const bool per_iter = (p->flags & ICET_FLAG_TIMING) != 0;
    for (int it = 0; it < L.iters; it++) {
        if (per_iter) HIPCHK(c, hipEventRecord(c->ev_acc[2 * it], c->stream));
        // (per-iteration timing wants the two halves apart; otherwise a small batch runs the solve inside the point pass' launch)
        const FuseArgs fa{it, L.d_out, L.aux}; bool fused = false;
        // keep list: from iteration keep_from on the point pass is the kernel that walks a pair's list or, for a pair without a valid one, its whole scan + keep masks;
        // the solve behind it builds / checks the lists (not behind the last pass: nothing follows)
        const int keep_pass = (lcfg.keep && it >= lcfg.keep_from) ? 1 : 0;
        HIPCHK(c, launch_gn_accumulate(wl, lcfg, c->stream, (per_iter || L.plain) ? nullptr : &fa, &fused, keep_pass ? 1 + 2 * (it & 1) : 0));
        if (per_iter) HIPCHK(c, hipEventRecord(c->ev_acc[2 * it + 1], c->stream));
        if (!fused) HIPCHK(c, launch_gn_solve(wl, lcfg, it, L.d_out, L.aux, c->stream, keep_pass ? (it + 1 < L.iters ? 1 : 2) : 0));
        if (want_pts2 && it == p->runlen - 2) ICET_TRY(enqueue_points2());
    }
    if (L.tail == kTailTerms) ICET_TRY(enqueue_terms_tail(c, p, wl, lcfg, L));
    else if (L.tail != kTailNone) {
        HIPCHK(c, launch_gn_accumulate(wl, lcfg, c->stream));
        if (L.tail == kTailDump) HIPCHK(c, launch_point_sums_dump(wl, lcfg, L.d_dump, c->stream));      // (icet_debug_point_sums_device: the raw sums in place of the score)
        else HIPCHK(c, launch_gn_score(wl, lcfg, p->runlen, L.d_score, c->stream));
    }
    if (c->capturing) return ICET_OK;
    HIPCHK(c, hipEventRecord(c->ev_c, c->stream));
    c->timing_valid = true; c->last_iters = (p->flags & ICET_FLAG_TIMING) ? p->runlen : 0;
    return ICET_OK;
}

// Staging buffers of the host-pointer entry points (3 x l floats per scan, leading dimension l = n rounded up to 64).
icet_status ensure_stage(icet_ctx* c, int64_t tot1, int64_t tot2) {
    if (3 * tot1 > c->cap_stage1 || 3 * tot2 > c->cap_stage2) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->st_copy) HIPCHK(c, hipStreamSynchronize(c->st_copy));
        if (3 * tot1 > c->cap_stage1) HIPCHK(c, grow(c->mem.stage1, c->cap_stage1, 3 * tot1, [&] { return c->mem.stage1.device(c->d_stage1, (size_t)3 * tot1); }));
        if (3 * tot2 > c->cap_stage2) HIPCHK(c, grow(c->mem.stage2, c->cap_stage2, 3 * tot2, [&] { return c->mem.stage2.device(c->d_stage2, (size_t)3 * tot2); }));
    }
    return ICET_OK;
}

// The host-pointer entries: scan 2 goes up on the copy stream (`up`) while the keyframe kernels enqueued in front of this run; ev_s2 marks it, and the loop waits for
// that; `then` puts what else the entry has for the copy stream behind the mark.  A failure drains both streams.
template <typename Up, typename Then> icet_status upload_scan2_beside(icet_ctx* c, const char* what, Up up, Then then) {
    hipError_t e = up();
    if (e == hipSuccess) e = hipEventRecord(c->ev_s2, c->st_copy);
    if (e == hipSuccess) e = then();
    if (e == hipSuccess) return ICET_OK;
    (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->st_copy); c->err = std::string(what) + ": " + hipGetErrorString(e);
    return ICET_ERR_HIP;
}

icet_status write_runlen0(icet_ctx* c, int32_t n_pairs, const float* d_x0, float* d_out) {
    // runlen == 0: the reference constructor returns X = X0, pred_stds = 0 (src/icet.cpp:36-37,47).
    HIPCHK(c, hipMemsetAsync(d_out, 0, sizeof(float) * 48 * (size_t)n_pairs, c->stream));
    if (d_x0) HIPCHK(c, hipMemcpy2DAsync(d_out, 48 * sizeof(float), d_x0, 6 * sizeof(float), 6 * sizeof(float), n_pairs, hipMemcpyDeviceToDevice, c->stream));
    return ICET_OK;
}

}  // namespace

extern "C" {

const char* icet_version(void) { return "icet_hip 0.1 (gfx950)"; }

const char* icet_last_error(const icet_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

icet_status icet_create(icet_ctx** out, int device_id, void* hip_stream) {
    if (!out) return ICET_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ICET_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= ndev) return ICET_ERR_NO_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return ICET_ERR_NO_DEVICE;
    icet_ctx* c = new (std::nothrow) icet_ctx();
    if (!c) return ICET_ERR_NOMEM;
    c->device = device_id;
    if (hip_stream) { c->stream = reinterpret_cast<hipStream_t>(hip_stream); c->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return ICET_ERR_HIP; }
        c->own_stream = true;
    }
    if (hipEventCreate(&c->ev_a) != hipSuccess || hipEventCreate(&c->ev_b) != hipSuccess || hipEventCreate(&c->ev_c) != hipSuccess) { delete c; return ICET_ERR_HIP; }
    // per context, with its device current: raise the dynamic-LDS limits of the kernels that need it (no process-global flags)
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id) == hipSuccess && lds > 0) c->max_lds = lds;
    if (init_keyframe_kernels() != hipSuccess || init_accumulate_kernels() != hipSuccess || init_rank_sort_kernels() != hipSuccess) {
        (void)hipGetLastError();
        if (c->own_stream) (void)hipStreamDestroy(c->stream);
        delete c; return ICET_ERR_HIP;       // no usable kernel image for this device: fail loudly, there is no fallback
    }
    {   // which form of the stable multi-splits this device gets (Tuning::lds_rank): ~0.1 ms once per context
        int32_t* d_t = nullptr; BufferGroup g; int ok = 0;                // (the word is freed at the end of this block)
        if (g.device(d_t, 1) == hipSuccess) { if (lds_rank_selftest(d_t, c->stream, &ok) != hipSuccess) { ok = 0; (void)hipGetLastError(); } }
        c->lds_rank_ok = ok;
    }
    if (c->mem.sync_word.pinned(c->h_sync_word, 1, hipHostMallocCoherent) == hipSuccess) *c->h_sync_word = 0;      // (without it icet_sync synchronises the stream)
    else (void)hipGetLastError();
    *out = c;
    return ICET_OK;
}

icet_status icet_destroy(icet_ctx* c) {
    if (!c) return ICET_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->st_copy) (void)hipStreamSynchronize(c->st_copy);
    for (icet_ctx* h : c->helpers) (void)icet_destroy(h);
    for (icet_ctx::GraphSlot* g : {&c->g_solve, &c->g_keyframe, &c->g_loop, &c->g_indexed, &c->g_scored, &c->g_score}) g->reset();
    for (hipEvent_t e : c->ev_acc) (void)hipEventDestroy(e);
    c->sel_read.destroy();
    for (hipEvent_t e : {c->ev_s2, c->ev_kf, c->ev_kfd, c->ev_prev, c->ev_pts2, c->ev_a, c->ev_b, c->ev_c, c->ev_fork, c->ev_desc, c->ev_graph, c->ev_stage, c->ev_join})
        if (e) (void)hipEventDestroy(e);
    if (c->st_copy) (void)hipStreamDestroy(c->st_copy);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                                 // (the groups of c->mem free what the context owned)
    return ICET_OK;
}

icet_status icet_sync(icet_ctx* c) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (c->armed_calls == 1 && c->h_sync_word) {
        // exactly one small solve is in flight and its last kernel raises h_sync_word behind its results: watch the word (hipStreamSynchronize answers several
        // microseconds after the queue has drained), asking the stream only now and then so that a failed launch still ends the wait
        volatile int32_t* w = c->h_sync_word;
        for (long spins = 1; *w == 0; spins++)
            if ((spins & 8191) == 0 && hipStreamQuery(c->stream) != hipErrorNotReady) break;
        (void)hipGetLastError();
        if (*w != 0) { __atomic_thread_fence(__ATOMIC_ACQUIRE); c->armed_calls = 0; return ICET_OK; }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->armed_calls = 0;
    return ICET_OK;
}

static int batch_parts(const icet_ctx* c, const icet_params* p, int32_t n_pairs);
static icet_status ensure_helpers(icet_ctx* c, int parts);

icet_status icet_reserve(icet_ctx* c, const icet_params* p, int32_t n_pairs, int64_t total_n1, int64_t total_n2) {
    if (!c || !params_ok(p) || n_pairs < 0 || total_n1 < 0 || total_n2 < 0) return ICET_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    // (a parked keyframe survives a reservation that fits the current capacity: ensure_workspace un-parks it exactly when its tables move)
    const int parts = batch_parts(c, p, n_pairs);
    if (parts > 1) {            // the batch will be solved in parts (icet_solve_batch_device); 12.5 % headroom for uneven scans
        icet_status hs = ensure_helpers(c, parts);
        if (hs != ICET_OK) return hs;
        const int np = (n_pairs + parts - 1) / parts;
        const int64_t n1 = total_n1 / parts + total_n1 / (8 * parts) + 1;
        const int64_t n2 = total_n2 / parts + total_n2 / (8 * parts) + 1;
        for (icet_ctx* h : c->helpers) { hs = ensure_workspace(h, p, np, n1, n2); if (hs != ICET_OK) { c->err = h->err; return hs; } }
        hs = ensure_workspace(c, p, np, n1, n2);
        if (hs != ICET_OK) return hs;
        return ensure_out(c, n_pairs);
    }
    icet_status s = ensure_workspace(c, p, n_pairs, total_n1, total_n2);
    if (s != ICET_OK) return s;
    return ensure_out(c, n_pairs);
}

// How many parts a device batch is cut into (see icet_ctx::helpers).  Timed calls stay in one part so that every
// kernel is measured alone on the device.
static int batch_parts(const icet_ctx* c, const icet_params* p, int32_t n_pairs) {
    if (p->flags & ICET_FLAG_TIMING) return 1;
    // One part.  Cutting the batch into staggered parts on separate streams paid in round 1 (1 part 84.7 k pairs/s, 2 parts 89.2 k) and has
    // been a wash since the keyframe and loop kernels were tightened: round 3, 256 pairs, 1 part 100.7 k, 2 parts 100.2 k, 3 parts 96.7 k,
    // 4 parts 82.1 k (scripts/exp_parts.sh) -- every phase fills the device on its own.  The mechanism stays behind `batch_parts`.
    int parts = 1;
    if (c->tune.batch_parts > 0) parts = c->tune.batch_parts > 8 ? 8 : c->tune.batch_parts;
    if (parts > n_pairs) parts = n_pairs > 0 ? n_pairs : 1;
    return parts;
}

static icet_status ensure_helpers(icet_ctx* c, int parts) {
    while ((int)c->helpers.size() < parts - 1) {
        icet_ctx* h = nullptr;
        icet_status s = icet_create(&h, c->device, nullptr);
        if (s != ICET_OK) { c->err = "helper context: cannot create"; return s; }
        if (hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) { icet_destroy(h); c->err = "helper context: event"; return ICET_ERR_HIP; }
        c->helpers.push_back(h);
    }
    if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    return ICET_OK;
}

static icet_status solve_device_part(icet_ctx* c, const icet_params* p, int32_t n_pairs, const icet_dev_scan* scan1, const icet_dev_scan* scan2,
                                     const float* d_x0, float* d_out, int64_t tot1);

icet_status icet_solve_batch_device(icet_ctx* c, const icet_params* p, int32_t n_pairs,
                                    const icet_dev_scan* scan1, const icet_dev_scan* scan2,
                                    const float* d_x0, float* d_out) {
    ICET_TRY(use_device(c));                                              // the arming entry: solve_device_part keeps armed_calls
    if (!params_ok(p) || n_pairs < 0 || (n_pairs > 0 && (!scan1 || !scan2 || !d_out))) { c->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (n_pairs == 0) return ICET_OK;
    int64_t tot1 = 0, tot2 = 0;
    if (!dev_scans_ok(scan1, n_pairs, &tot1) || !dev_scans_ok(scan2, n_pairs, &tot2)) { c->err = "bad scan descriptor"; return ICET_ERR_BAD_ARG; }
    const int parts = (p->runlen == 0) ? 1 : batch_parts(c, p, n_pairs);
    auto range_tot = [&](int b, int e) { int64_t t = 0; for (int k = b; k < e; k++) t += scan1[k].n; return t; };
    if (parts == 1) return solve_device_part(c, p, n_pairs, scan1, scan2, d_x0, d_out, tot1);
    c->armed_calls = 2;
    { icet_status s = ensure_helpers(c, parts); if (s != ICET_OK) return s; }
    // fork: helpers start after whatever the caller queued on this context's stream (e.g. the writes of the scans)
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    // Stagger: part i+1 starts once part i has finished the first keyframe stage, so the parts do not move through the
    // same phase in lock step (measured on 256 pairs with the kernels of that day: 1 part 70.6k pairs/s; 3 parts in lock
    // step 73.2k; staggered 76.8k).
    const int stage = c->tune.batch_stage;
    icet_status status = ICET_OK;
    int started = 0;                        // helpers whose stream has work queued
    for (int i = 0; i < parts && status == ICET_OK; i++) {
        const int b = (int)((int64_t)n_pairs * i / parts), e = (int)((int64_t)n_pairs * (i + 1) / parts);
        icet_ctx* h = (i == 0) ? c : c->helpers[i - 1];
        if (h != c) { const bool relut = h->tune.guard_scale != c->tune.guard_scale || h->tune.lut_polar_quantile != c->tune.lut_polar_quantile; h->tune = c->tune; if (relut) h->w.thr_T = 0; }
        hipError_t he = hipSuccess;
        if (stage && !h->ev_stage) he = hipEventCreateWithFlags(&h->ev_stage, hipEventDisableTiming);
        h->stage_at = (i + 1 < parts) ? stage : 0;
        if (he == hipSuccess && i > 0) {
            he = hipStreamWaitEvent(h->stream, c->ev_fork, 0);
            if (he == hipSuccess && stage) { icet_ctx* prev = (i == 1) ? c : c->helpers[i - 2]; he = hipStreamWaitEvent(h->stream, prev->ev_stage, 0); }
        }
        if (he != hipSuccess) { c->err = std::string("batch part fork: ") + hipGetErrorString(he); status = ICET_ERR_HIP; break; }
        if (i > 0) started = i;
        status = solve_device_part(h, p, e - b, scan1 + b, scan2 + b, d_x0 ? d_x0 + 6 * (size_t)b : nullptr, d_out + 48 * (size_t)b, range_tot(b, e));
        if (status != ICET_OK && h != c) c->err = h->err;
    }
    // join -- ALSO on failure: every helper that was started may still be reading the caller's scans / x0 and writing d_out, so
    // the caller's stream must not pass this call (and the caller must not free those buffers) before they have drained
    for (int i = 1; i <= started; i++) {
        icet_ctx* h = c->helpers[i - 1];
        if (hipEventRecord(h->ev_join, h->stream) != hipSuccess || hipStreamWaitEvent(c->stream, h->ev_join, 0) != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);          // last resort: block the host until the helper is idle
            if (status == ICET_OK) { c->err = "batch part join failed"; status = ICET_ERR_HIP; }
        }
    }
    return status;
}

extern "C++" {
// ---- hipGraph replay of small device batches ------------------------------------------------------------------------------------
// The kernels read the scans' addresses and sizes from the descriptor table (re-uploaded from pinned memory by a memcpy node of the graph on
// every replay, and patched with device-side row counts where the caller has them); what the launches themselves depend on is the LaunchCfg
// (grids, LDS sizes, point counts passed by value) and the workspace pointers.  A call whose key equals the previous call's is captured;
// later calls with that key replay: one hipGraphLaunch instead of 15 - 35 launches on the host.
// The identity of an entry's call -- which entry, and the caller's argument pointers -- as the start of its key; an indexed call adds mode, ws_gen and its keyframe source.
static icet_ctx::GraphKey entry_key(icet_ctx::GraphEntry entry, const void* x0, const void* out, const void* extra) {
    icet_ctx::GraphKey key{};
    key.entry = entry; key.x0 = x0; key.out = out; key.extra = extra;
    return key;
}
// ... completed with what the launches of ANY entry depend on: the plan, the workspace pointers, the prologue and the done flag.
static icet_ctx::GraphKey graph_key_of(const icet_ctx* c, const icet_params* p, const LaunchCfg& cfg, icet_ctx::GraphKey key) {
    const Workspace& w = c->w;
    const void* ws[] = {w.desc, w.thr, w.lut, w.r1, w.counts, w.near_over, w.acc, w.fit_items, w.tile_vr};
    static_assert(sizeof(ws) == sizeof(key.ws), "GraphKey::ws");
    std::memcpy(key.ws, ws, sizeof(ws));
    key.prologue_key = c->prologue ? c->prologue_key : 0; key.done_flag = c->done_flag; key.flags = p->flags;
    launch_key_of(cfg, key.launch);
    return key;
}
static bool graph_eligible(const icet_ctx* c, const icet_params* p, int32_t n_pairs) {
#ifdef ICET_DIAG_ENV      /* experiment builds only (make EXTRA=-DICET_DIAG_ENV): the shipped library never reads the environment -- use icet_set_option("graph", 0) */
    static const bool env_off = getenv("ICET_NO_GRAPH") != nullptr;
#else
    constexpr bool env_off = false;
#endif
    return !env_off && c->graph_mode && n_pairs <= 8 && !(p->flags & (ICET_FLAG_TIMING | ICET_FLAG_ROUNDTRIP_SCAN2)) && !c->stage_at;
}
// Runs `enq` (which enqueues on c->stream) eagerly, or captured into `slot` and replayed.  The pinned descriptor staging must already hold this call's
// descriptors; the caller has waited for a replay in flight before it wrote them.
template <typename Enq> static icet_status run_or_replay(icet_ctx* c, icet_ctx::GraphSlot& slot, const icet_ctx::GraphKey& key, Enq enq) {
    auto same = [](const icet_ctx::GraphKey& a, const icet_ctx::GraphKey& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; };
    if (!(slot.have_graph && same(key, slot.key))) {
        if (!(slot.have_seen && same(key, slot.seen))) { slot.seen = key; slot.have_seen = true; return enq(); }      // a key's first call runs eagerly, its second is captured
        slot.reset();
        if (!c->ev_graph) HIPCHK(c, hipEventCreateWithFlags(&c->ev_graph, hipEventDisableTiming));
        HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        c->capturing = true;
        const icet_status es = enq();
        c->capturing = false;
        hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
        const hipError_t ee = hipStreamEndCapture(c->stream, &g);
        // could not capture (a capacity grew, an unsupported call) or instantiate: run this call eagerly and stop trying for this key
        if (es != ICET_OK || ee != hipSuccess || !g || hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) {
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            slot.have_seen = false;
            return enq();
        }
        slot.graph = g; slot.exec = ge; slot.key = key; slot.have_graph = true;
    }
    HIPCHK(c, hipGraphLaunch(slot.exec, c->stream));
    ICET_TRY(staging_mark_replay(c));
    c->timing_valid = false;
    return ICET_OK;
}
// THE CAPTURE STEP of every entry that can replay: `enq` run eagerly, or through `slot` under the key that `ident` (entry_key) begins.  The call's staging is laid
// out and `cfg` is its plan: a replay runs no enqueuer and reads the staging as the layout left it, and the thresholds, which no capture may build, exist since the
// plan was made.  allowed: the entry's own condition (a query, whose search kernels take the call's poses as arguments, is never captured; nor are dump and terms).
template <typename Enq> static icet_status run_captured(icet_ctx* c, icet_ctx::GraphSlot& slot, const icet_params* p, const LaunchCfg& cfg, const icet_ctx::GraphKey& ident, bool allowed, Enq enq) {
    if (!allowed || !graph_eligible(c, p, cfg.n_pairs)) return enq();
    return run_or_replay(c, slot, graph_key_of(c, p, cfg, ident), enq);
}
// One half (1: scan 1, icet_keyframe_device_n; 2: scan 2, icet_register_device_n) of the call's descriptors into h_desc.  A sequential caller hands the SAME buffers
// to a half frame after frame (include/icet_nodes.h): the pinned staging then already holds this call's halves and is left alone -- rewriting it means waiting, on
// the HOST, for whatever replay or copy of this context still reads it, and a burst of frames (icet_node_push_many_device) would have the host wait for the device
// twice per frame instead of running ahead.  Only what the previous call of THIS entry wrote counts (desc_kf_valid / desc_reg_valid): raw staging memory proves nothing.
static icet_status stage_half(icet_ctx* c, int half, int32_t n_pairs, const icet_dev_scan* scan) {
    bool& valid = half == 1 ? c->desc_kf_valid : c->desc_reg_valid;
    bool same_desc = valid;
    for (int k = 0; k < n_pairs && same_desc; k++) same_desc = half == 1 ? same_scan1(c->h_desc[k], scan[k]) : same_scan2(c->h_desc[k], scan[k]);
    if (same_desc) return ICET_OK;
    if (half == 1) c->desc_reg_valid = false;                              // (set_scan1 resets the scan-2 halves)
    ICET_TRY(staging_wait(c));
    for (int k = 0; k < n_pairs; k++) { if (half == 1) set_scan1(c->h_desc[k], scan[k]); else set_scan2(c->h_desc[k], scan[k]); }
    valid = true;
    return ICET_OK;
}
}  // extern "C++"

static icet_status solve_device_part(icet_ctx* c, const icet_params* p, int32_t n_pairs, const icet_dev_scan* scan1, const icet_dev_scan* scan2,
                                     const float* d_x0, float* d_out, int64_t tot1) {
    int64_t tot2 = 0; for (int k = 0; k < n_pairs; k++) tot2 += scan2[k].n;
    c->kf_pairs = 0;                           // whatever keyframe was parked here is gone (runlen == 0 included: h_desc is overwritten below)
    ICET_TRY(ensure_workspace(c, p, n_pairs, tot1, tot2));
    // the previous call may still be copying out of the pinned descriptor staging; its kernels may still be running
    // (the device entry point never waits for them: calls queue up behind each other on the stream)
    ICET_TRY(staging_wait(c));
    c->desc_kf_valid = c->desc_reg_valid = false;
    // A RAGGED throughput batch is laid out XCD-balanced (round 6; icet_layout.h says why and how).  The caller's order comes back in k_init_state (X0) and
    // k_gn_solve (results): LaunchCfg::pair_user.  Same bits: a pair's result does not depend on its slot (section 6 of DESIGN.md).
    c->perm_active = false; c->perm_pairs = n_pairs;
    std::vector<int32_t> order((size_t)n_pairs);
    for (int k = 0; k < n_pairs; k++) order[(size_t)k] = k;
    if (n_pairs > kUploadDescMaxPairs && p->runlen > 0) {
        std::vector<int64_t> size((size_t)n_pairs);
        for (int k = 0; k < n_pairs; k++) size[(size_t)k] = scan1[k].n + scan2[k].n;
        if (icet_layout::is_ragged(size)) {
            order = icet_layout::balanced_slot_order(size);
            for (int s = 0; s < n_pairs; s++) c->h_seg[n_pairs + 1 + s] = order[(size_t)s];
            c->perm_active = true;
        }
    }
    for (int s = 0; s < n_pairs; s++) {
        const int k = order[(size_t)s];
        set_scan1(c->h_desc[s], scan1[k]); set_scan2(c->h_desc[s], scan2[k]);
    }
    if (p->runlen == 0) { c->armed_calls = 2; return write_runlen0(c, n_pairs, d_x0, d_out); }
    const bool eligible = graph_eligible(c, p, n_pairs);
    if (!eligible) c->armed_calls = 2;
    ICET_TRY(ensure_thresholds(c, p->bins_theta, p->bins_phi));
    // (a captured solve's last kernel raises the context's sync word: icet_sync.  The word is the plan's done_flag, and a part of the key: set before either is made)
    const bool own_word = eligible && !c->done_flag && c->h_sync_word;
    if (own_word) { if (c->armed_calls == 0) *static_cast<volatile int32_t*>(c->h_sync_word) = 0; c->done_flag = c->h_sync_word; }
    const LaunchCfg cfg = make_cfg(c, p, n_pairs, lay_out_staging(c->h_desc, c->h_seg, n_pairs));
    const icet_status rs = run_captured(c, c->g_solve, p, cfg, entry_key(icet_ctx::kEntrySolve, d_x0, d_out, nullptr), true, [&]() -> icet_status {
        ICET_TRY(enqueue_keyframe(c, cfg, nullptr));
        return enqueue_loop(c, p, cfg, pair_loop(c, cfg, d_x0, d_out, nullptr, false));      // (the staging went up with the keyframe)
    });
    if (own_word) { c->done_flag = nullptr; c->armed_calls = (rs == ICET_OK && c->g_solve.have_graph) ? c->armed_calls + 1 : 2; }
    return rs;
}

icet_status icet_keyframe_device(icet_ctx* c, const icet_params* p, int32_t n_pairs, const icet_dev_scan* scan1) {
    return icet_keyframe_device_n(c, p, n_pairs, scan1, nullptr);
}

icet_status icet_keyframe_device_n(icet_ctx* c, const icet_params* p, int32_t n_pairs, const icet_dev_scan* scan1, const int32_t* d_rows) {
    ICET_TRY(enter(c));
    if (!params_ok(p) || n_pairs < 1 || !scan1) { c->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    int64_t tot1 = 0;
    if (!dev_scans_ok(scan1, n_pairs, &tot1)) { c->err = "bad scan descriptor"; return ICET_ERR_BAD_ARG; }
    c->kf_pairs = 0; c->perm_active = false;
    icet_status s = ensure_workspace(c, p, n_pairs, tot1, 0);
    if (s != ICET_OK) return s;
    ICET_TRY(stage_half(c, 1, n_pairs, scan1));
    LaunchCfg cfg; ICET_TRY(plan_pairs(c, p, n_pairs, &cfg));
    ICET_TRY(run_captured(c, c->g_keyframe, p, cfg, entry_key(icet_ctx::kEntryKeyframe, nullptr, nullptr, d_rows), true, [&]() { return enqueue_keyframe(c, cfg, nullptr, d_rows); }));
    c->kf_pairs = n_pairs; c->kf_params = *p;
    return ICET_OK;
}

icet_status icet_register_device(icet_ctx* c, const icet_params* p, int32_t n_pairs, const icet_dev_scan* scan2, const float* d_x0, float* d_out) {
    return icet_register_device_n(c, p, n_pairs, scan2, nullptr, d_x0, d_out);
}

icet_status icet_register_device_n(icet_ctx* c, const icet_params* p, int32_t n_pairs, const icet_dev_scan* scan2, const int32_t* d_rows, const float* d_x0, float* d_out) {
    ICET_TRY(enter(c));
    if (!params_ok(p) || n_pairs < 1 || !scan2 || !d_out) { c->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (c->kf_pairs != n_pairs || !same_keyframe_shape(c->kf_params, *p)) { c->err = "no keyframe with these parameters is parked in this context (icet_keyframe_device)"; return ICET_ERR_BAD_ARG; }
    int64_t tot2 = 0;
    if (!dev_scans_ok(scan2, n_pairs, &tot2)) { c->err = "bad scan descriptor"; return ICET_ERR_BAD_ARG; }
    if (p->runlen == 0) return write_runlen0(c, n_pairs, d_x0, d_out);
    icet_status s = ensure_workspace(c, p, n_pairs, 0, tot2);              // only the scan-2 overflow list can grow here: the keyframe tables stay
    if (s != ICET_OK) return s;
    ICET_TRY(stage_half(c, 2, n_pairs, scan2));
    LaunchCfg cfg; ICET_TRY(plan_pairs(c, p, n_pairs, &cfg));                            // (the thresholds: a keyframe store's call on another grid may have rebuilt them since the keyframe was parked)
    return run_captured(c, c->g_loop, p, cfg, entry_key(icet_ctx::kEntryLoop, d_x0, d_out, d_rows), true, [&]() -> icet_status {
        if (c->prologue) HIPCHK(c, c->prologue(c->prologue_user, c->stream));
        LoopCall L = pair_loop(c, cfg, d_x0, d_out, nullptr, true);       // (the scan-2 halves arrived after the keyframe call: the staging goes up again)
        L.d_rows = d_rows;
        return enqueue_loop(c, p, cfg, L);
    });
}

}  // extern "C"
icet_status icet::register_indexed(icet_ctx* c, const icet_params* p, int32_t n_regs, const int32_t* kf_index, const icet_dev_scan* scan2, const float* d_x0, float* d_out,
                                   icet_score* d_score, IndexedMode mode, const icet_keyframe_store* src, const IndexedDev* dev, uint32_t* d_dump, const GnTermsOut* terms) {
    if (!c) return ICET_ERR_BAD_ARG;
    const bool need_out = mode == kIdxRegister || mode == kIdxScored || mode == kIdxTerms, need_score = mode == kIdxScored || mode == kIdxScoreOnly, need_x = mode == kIdxScoreOnly || mode == kIdxDump || mode == kIdxTerms;
    if (!params_ok(p) || n_regs < 0 || (n_regs > 0 && (!kf_index || !scan2 || (need_out && !d_out) || (need_score && !d_score) || (need_x && !d_x0) || ((mode == kIdxDump || mode == kIdxTerms) && !d_dump) || (mode == kIdxTerms && (!terms || !terms->xf || !terms->htwh || !terms->htwdz || p->runlen < 1))))) { c->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (n_regs == 0) return ICET_OK;
    // everything is checked before anything is touched: a refused call leaves the parked keyframe (and every slot of a store) as it was
    const icet_params& q = src ? src->shape : c->kf_params;
    const int32_t n_kf = src ? src->capacity : c->kf_pairs;
    if (n_kf < 1 || !same_keyframe_shape(q, *p)) {
        c->err = src ? "the grid, n, thresh, buff or keyframe-shaping flags differ from the keyframe store's shape" : "no keyframe with these parameters is parked in this context (icet_keyframe_device)";
        return ICET_ERR_BAD_ARG;
    }
    int64_t tot2 = 0;
    for (int r = 0; r < n_regs; r++) {
        if (src && (kf_index[r] < 0 || kf_index[r] >= n_kf || !src->occupied[(size_t)kf_index[r]])) {
            c->err = "slot_index[" + std::to_string(r) + "] = " + std::to_string(kf_index[r]) + " is not an occupied slot of the store (capacity " + std::to_string(n_kf) + ")"; return ICET_ERR_BAD_ARG;
        }
        if (kf_index[r] < 0 || kf_index[r] >= n_kf) { c->err = "kf_index[" + std::to_string(r) + "] = " + std::to_string(kf_index[r]) + " is not a parked keyframe (0 .. " + std::to_string(c->kf_pairs - 1) + ")"; return ICET_ERR_BAD_ARG; }
    }
    if (!dev_scans_ok(scan2, n_regs, &tot2)) { c->err = "bad scan descriptor"; return ICET_ERR_BAD_ARG; }
    if (c->tune.keep != 0) { c->err = "indexed registrations run the plain point pass: option \"keep\" must be 0"; return ICET_ERR_UNSUPPORTED; }
    ICET_TRY(enter(c));
    if (mode == kIdxRegister && p->runlen == 0) return write_runlen0(c, n_regs, d_x0, d_out);
    icet_status s = ensure_regs(c, n_regs, p->bins_phi * p->bins_theta);   // the registration side only: the keyframe tables stay where they are
    if (s == ICET_OK) s = ensure_scan2(c, tot2);
    if (s == ICET_OK) s = ensure_thresholds(c, p->bins_theta, p->bins_phi);
    if (s == ICET_OK) s = staging_wait(c);                                // the previous call may still read the registration staging
    if (s != ICET_OK) return s;
    for (int r = 0; r < n_regs; r++) {
        set_scan1(c->h_desc_reg[r], icet_dev_scan{nullptr, 0, 0});        // (the loop reads no scan-1 field)
        set_scan2(c->h_desc_reg[r], scan2[r]);
        c->h_kf_of[r] = kf_index[r];
    }
    c->h_kf_of[n_regs] = 0;
    // (no segment table in the layout: the keyframe index travels in its place.  A query's staging holds an occupied slot and the scans' full row counts: the launch
    // geometry is sized from those, as in icet_register_device_n)
    const LaunchCfg cfg = make_cfg(c, p, n_regs, lay_out_staging(c->h_desc_reg, nullptr, n_regs));
    const Workspace& w = c->w; LoopCall L;
    L.hd = c->h_desc_reg; L.hs = c->h_kf_of; L.seg_words = (size_t)n_regs + 1; L.upload = true;
    L.view = w; L.view.desc = w.desc_reg; L.view.seg_off = w.kf_of; L.kf_of = w.kf_of;
    if (src) { L.view.hotS = src->hotS; L.view.fitS = src->fitS; L.view.slot_of_voxel = src->slot_of_voxel; L.view.n_slots = src->n_slots; }      // (a store's rows: h_kf_of then holds slot indices)
    L.d_x0 = d_x0; L.d_out = d_out; L.plain = L.own_timing = L.init_on_copy = true;
    if (dev) { L.d_rows = dev->rows; L.d_kf_of = dev->kf_of; }
    // scored calls: runlen == 0 scores X0 (results as the unscored call writes them); score-only, dump and terms take d_x0 without iterating
    L.iters = (mode == kIdxRegister || mode == kIdxScored) ? p->runlen : 0;
    L.tail = mode == kIdxRegister ? kTailNone : mode == kIdxDump ? kTailDump : mode == kIdxTerms ? kTailTerms : kTailScore;
    L.d_score = d_score; L.d_dump = d_dump; L.terms = terms;
    // A replay re-reads the staging -- descriptors AND keyframe index -- when it runs; the key names what the launches themselves take (ws_gen: any buffer moved; the
    // keyframe source: the context's tables, or a store's identity and generation).  Scored and score-only calls have slots of their own, and the mode is a part of
    // the key: a scored call never replays an unscored call's graph, nor the reverse.  A query (dev), dump and terms are never captured.
    icet_ctx::GraphKey ident = entry_key(icet_ctx::kEntryIndexed, d_x0, d_out, d_score);
    ident.mode = mode; ident.ws_gen = c->ws_gen; ident.src_id = src ? src->id : 0; ident.src_gen = src ? src->gen : 0;
    icet_ctx::GraphSlot& slot = mode == kIdxScored ? c->g_scored : mode == kIdxScoreOnly ? c->g_score : c->g_indexed;
    return run_captured(c, slot, p, cfg, ident, !dev && mode != kIdxDump && mode != kIdxTerms, [&]() -> icet_status {
        if (mode == kIdxScored && p->runlen == 0) ICET_TRY(write_runlen0(c, n_regs, d_x0, d_out));
        return enqueue_loop(c, p, cfg, L);
    });
}
extern "C" {

icet_status icet_register_indexed_device(icet_ctx* c, const icet_params* p, int32_t n_regs, const int32_t* kf_index, const icet_dev_scan* scan2, const float* d_x0, float* d_out) {
    return register_indexed(c, p, n_regs, kf_index, scan2, d_x0, d_out, nullptr, kIdxRegister);
}

icet_status icet_register_indexed_scored_device(icet_ctx* c, const icet_params* p, int32_t n_regs, const int32_t* kf_index, const icet_dev_scan* scan2,
                                                const float* d_x0, float* d_out, icet_score* d_score) {
    return register_indexed(c, p, n_regs, kf_index, scan2, d_x0, d_out, d_score, kIdxScored);
}

icet_status icet_score_indexed_device(icet_ctx* c, const icet_params* p, int32_t n_regs, const int32_t* kf_index, const icet_dev_scan* scan2,
                                      const float* d_X, icet_score* d_score) {
    return register_indexed(c, p, n_regs, kf_index, scan2, d_X, nullptr, d_score, kIdxScoreOnly);
}

// Test hook: the point pass of icet_score_indexed_device at the poses d_X, then the raw accumulator records instead of the score.
icet_status icet_debug_point_sums_device(icet_ctx* c, const icet_params* p, int32_t n_regs, const int32_t* kf_index, const icet_dev_scan* scan2,
                                         const float* d_X, void* d_sums) {
    if (c && (reinterpret_cast<uintptr_t>(d_sums) & 15u)) { c->err = "icet_debug_point_sums_device: d_sums must be 16-byte aligned"; return ICET_ERR_BAD_ARG; }      // (the copy-out kernel stores 16 bytes at a time)
    return register_indexed(c, p, n_regs, kf_index, scan2, d_X, nullptr, nullptr, kIdxDump, nullptr, nullptr, static_cast<uint32_t*>(d_sums));
}

// Test hook: the point pass at the poses d_X, the raw records (left in place), then the production solve of iteration runlen - 1 on them.
icet_status icet_debug_gn_terms_device(icet_ctx* c, const icet_params* p, int32_t n_regs, const int32_t* kf_index, const icet_dev_scan* scan2,
                                       const float* d_X, void* d_sums, float* d_xf, float* d_htwh, float* d_htwdz, float* d_out) {
    if (c && (reinterpret_cast<uintptr_t>(d_sums) & 15u)) { c->err = "icet_debug_gn_terms_device: d_sums must be 16-byte aligned"; return ICET_ERR_BAD_ARG; }      // (the copy-out kernel stores 16 bytes at a time)
    const GnTermsOut t{d_xf, d_htwh, d_htwdz};
    return register_indexed(c, p, n_regs, kf_index, scan2, d_X, d_out, nullptr, kIdxTerms, nullptr, nullptr, static_cast<uint32_t*>(d_sums), &t);
}

// Scores of the host-pointer entry points: device + pinned, n entries.
static icet_status ensure_score(icet_ctx* c, int32_t n) {
    if (n <= c->cap_score) return ICET_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    BufferGroup& g = c->mem.score;
    HIPCHK(c, grow(g, c->cap_score, n, [&] { const int e = g.device(c->d_score, (size_t)n); return e ? e : g.pinned(c->h_score, (size_t)n); }));
    return ICET_OK;
}

// icet_solve_indexed (score_out == nullptr), icet_solve_indexed_scored (mode kIdxScored) and icet_score_indexed (kIdxScoreOnly: x0 = the poses, no results but the scores).
static icet_status solve_indexed_host(icet_ctx* c, const icet_params* p, int32_t n_kf, const float* const* scan1, const int64_t* n1,
                                      int32_t n_regs, const int32_t* kf_index, const float* const* scan2, const int64_t* n2,
                                      const float* x0, float* x_out, float* pred_stds_out, float* cov_out, icet_score* score_out, IndexedMode mode) {
    if (!c) return ICET_ERR_BAD_ARG;
    const bool need_out = mode != kIdxScoreOnly;
    if (!params_ok(p) || n_kf < 1 || n_regs < 0 || !scan1 || !n1 || (n_regs > 0 && (!kf_index || !scan2 || !n2 || (need_out && (!x_out || !pred_stds_out)) ||
                                                                                     (mode != kIdxRegister && !score_out) || (mode == kIdxScoreOnly && !x0)))) { c->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (c->pend.active) { c->err = "icet_solve_begin without icet_solve_end on this context"; return ICET_ERR_BAD_ARG; }
    for (int k = 0; k < n_kf; k++)
        if (n1[k] < 0 || (n1[k] > 0 && !scan1[k])) { c->err = "bad scan"; return ICET_ERR_BAD_ARG; }
    for (int r = 0; r < n_regs; r++) {
        if (n2[r] < 0 || (n2[r] > 0 && !scan2[r])) { c->err = "bad scan"; return ICET_ERR_BAD_ARG; }
        if (kf_index[r] < 0 || kf_index[r] >= n_kf) { c->err = "kf_index[" + std::to_string(r) + "] out of range"; return ICET_ERR_BAD_ARG; }
    }
    if (n_regs == 0) return ICET_OK;
    ICET_TRY(enter(c));
    icet_status s = ensure_out(c, n_regs);
    if (s == ICET_OK) s = ensure_stage(c, stage_layout(n1, n_kf, nullptr, nullptr), stage_layout(n2, n_regs, nullptr, nullptr));
    if (s == ICET_OK && mode != kIdxRegister) s = ensure_score(c, n_regs);
    if (s != ICET_OK) return s;
    // scans into the staging buffers (dense column-major), then the two device halves
    std::vector<icet_dev_scan> d1((size_t)n_kf), d2((size_t)n_regs);
    stage_layout(n1, n_kf, c->d_stage1, d1.data()); stage_layout(n2, n_regs, c->d_stage2, d2.data());
    HIPCHK(c, upload_staged(d1.data(), scan1, n_kf, c->stream));
    HIPCHK(c, upload_staged(d2.data(), scan2, n_regs, c->stream));
    const float* dx0 = nullptr;
    ICET_TRY(stage_x0(c, x0, n_regs, &dx0));
    s = icet_keyframe_device(c, p, n_kf, d1.data());
    if (s == ICET_OK) s = register_indexed(c, p, n_regs, kf_index, d2.data(), dx0, need_out ? c->d_out : nullptr, mode != kIdxRegister ? c->d_score : nullptr, mode);
    if (s != ICET_OK) { (void)hipStreamSynchronize(c->stream); return s; }
    if (need_out) HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, sizeof(float) * 48 * n_regs, hipMemcpyDeviceToHost, c->stream));
    if (mode != kIdxRegister) HIPCHK(c, hipMemcpyAsync(c->h_score, c->d_score, sizeof(icet_score) * n_regs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->armed_calls = 0; staging_idle(c);                                  // (a caller that alternates this entry with device calls would otherwise wait for events long past)
    if (need_out) unpack_results(c->h_out, n_regs, x_out, pred_stds_out, cov_out);
    if (mode != kIdxRegister) std::memcpy(score_out, c->h_score, sizeof(icet_score) * n_regs);
    return ICET_OK;
}

icet_status icet_solve_indexed(icet_ctx* c, const icet_params* p, int32_t n_kf, const float* const* scan1, const int64_t* n1,
                               int32_t n_regs, const int32_t* kf_index, const float* const* scan2, const int64_t* n2,
                               const float* x0, float* x_out, float* pred_stds_out, float* cov_out) {
    return solve_indexed_host(c, p, n_kf, scan1, n1, n_regs, kf_index, scan2, n2, x0, x_out, pred_stds_out, cov_out, nullptr, kIdxRegister);
}

icet_status icet_solve_indexed_scored(icet_ctx* c, const icet_params* p, int32_t n_kf, const float* const* scan1, const int64_t* n1,
                                      int32_t n_regs, const int32_t* kf_index, const float* const* scan2, const int64_t* n2,
                                      const float* x0, float* x_out, float* pred_stds_out, float* cov_out, icet_score* score_out) {
    return solve_indexed_host(c, p, n_kf, scan1, n1, n_regs, kf_index, scan2, n2, x0, x_out, pred_stds_out, cov_out, score_out, kIdxScored);
}

icet_status icet_score_indexed(icet_ctx* c, const icet_params* p, int32_t n_kf, const float* const* scan1, const int64_t* n1,
                               int32_t n_regs, const int32_t* kf_index, const float* const* scan2, const int64_t* n2,
                               const float* X, icet_score* score_out) {
    return solve_indexed_host(c, p, n_kf, scan1, n1, n_regs, kf_index, scan2, n2, X, nullptr, nullptr, nullptr, score_out, kIdxScoreOnly);
}

icet_status icet_select_best_device(icet_ctx* c, int32_t n_regs, const int32_t* group, int32_t n_groups,
                                    const icet_score* d_score, const float* d_out, int32_t* d_best, float* d_best_out) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (n_regs < 0 || n_groups < 0 || (n_regs > 0 && (!group || !d_score || (d_best_out && !d_out))) || (n_groups > 0 && !d_best)) { c->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    for (int r = 0; r < n_regs; r++)
        if (group[r] < 0 || group[r] >= n_groups) { c->err = "group[" + std::to_string(r) + "] = " + std::to_string(group[r]) + " is not a group (0 .. " + std::to_string(n_groups - 1) + ")"; return ICET_ERR_BAD_ARG; }
    if (n_groups == 0) return ICET_OK;
    ICET_TRY(enter(c));
    // members of every group in ascending order, then the offsets: one upload from pinned staging
    const int64_t need = (int64_t)n_regs + n_groups + 1;
    HIPCHK(c, c->sel_read.wait());                                    // the previous call's copy has read h_sel
    if (need > c->cap_sel) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        BufferGroup& sm = c->mem.sel;
        HIPCHK(c, grow(sm, c->cap_sel, need, [&] { const int e = sm.device(c->d_sel, (size_t)need); return e ? e : sm.pinned(c->h_sel, (size_t)need); }));
    }
    int32_t* members = c->h_sel; int32_t* offs = c->h_sel + n_regs;
    for (int g = 0; g <= n_groups; g++) offs[g] = 0;
    for (int r = 0; r < n_regs; r++) offs[group[r] + 1] += 1;
    for (int g = 0; g < n_groups; g++) offs[g + 1] += offs[g];
    std::vector<int32_t> fill(offs, offs + n_groups);
    for (int r = 0; r < n_regs; r++) members[fill[(size_t)group[r]]++] = r;
    HIPCHK(c, hipMemcpyAsync(c->d_sel, c->h_sel, sizeof(int32_t) * (size_t)need, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, c->sel_read.mark(c->stream));
    HIPCHK(c, launch_select_best(c->d_sel, c->d_sel + n_regs, n_groups, d_score, d_out, d_best, d_best_out, c->stream));
    return ICET_OK;
}

icet_status icet_solve_batch(icet_ctx* c, const icet_params* p, int32_t n_pairs,
                             const float* const* scan1, const int64_t* n1, const float* const* scan2, const int64_t* n2,
                             const float* x0, float* x_out, float* pred_stds_out, float* cov_out) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (!params_ok(p) || n_pairs < 0 || (n_pairs > 0 && (!scan1 || !n1 || !scan2 || !n2 || !x_out || !pred_stds_out))) { c->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (c->pend.active) { c->err = "icet_solve_begin without icet_solve_end on this context"; return ICET_ERR_BAD_ARG; }
    if (n_pairs == 0) return ICET_OK;
    for (int k = 0; k < n_pairs; k++)
        if (n1[k] < 0 || n2[k] < 0 || (n1[k] > 0 && !scan1[k]) || (n2[k] > 0 && !scan2[k])) { c->err = "bad scan"; return ICET_ERR_BAD_ARG; }
    ICET_TRY(enter(c));
    const int64_t tot1 = stage_layout(n1, n_pairs, nullptr, nullptr), tot2 = stage_layout(n2, n_pairs, nullptr, nullptr);
    icet_status s = ensure_workspace(c, p, n_pairs, tot1, tot2);
    if (s == ICET_OK) s = ensure_out(c, n_pairs);
    if (s == ICET_OK) s = ensure_host_path(c);
    if (s == ICET_OK) s = ensure_stage(c, tot1, tot2);
    if (s == ICET_OK) s = staging_wait(c);
    if (s != ICET_OK) return s;
    // Scan 1 of every pair goes up first on the solve stream (the keyframe build needs nothing else); the scan 2s follow on the copy
    // stream while the keyframe kernels run, and the loop waits for them.  Host scans are dense column-major (ld == n) in this entry point.
    std::vector<icet_dev_scan> d1((size_t)n_pairs), d2((size_t)n_pairs);
    stage_layout(n1, n_pairs, c->d_stage1, d1.data()); stage_layout(n2, n_pairs, c->d_stage2, d2.data());
    c->desc_kf_valid = c->desc_reg_valid = false;
    for (int k = 0; k < n_pairs; k++) { set_scan1(c->h_desc[k], d1[(size_t)k]); set_scan2(c->h_desc[k], d2[(size_t)k]); }
    HIPCHK(c, upload_staged(d1.data(), scan1, n_pairs, c->stream));
    const float* dx0 = nullptr;
    ICET_TRY(stage_x0(c, x0, n_pairs, &dx0));
    if (p->runlen == 0) s = write_runlen0(c, n_pairs, dx0, c->d_out);
    else {
        c->kf_pairs = 0; c->perm_active = false;
        LaunchCfg cfg; s = plan_pairs(c, p, n_pairs, &cfg);
        if (s == ICET_OK) s = enqueue_keyframe(c, cfg, nullptr);
        if (s == ICET_OK) s = upload_scan2_beside(c, "scan-2 upload", [&] { return upload_staged(d2.data(), scan2, n_pairs, c->st_copy); }, [] { return hipSuccess; });
        if (s == ICET_OK) s = enqueue_loop(c, p, cfg, pair_loop(c, cfg, dx0, c->d_out, nullptr, false, c->ev_s2));
    }
    if (s != ICET_OK) { (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->st_copy); return s; }
    HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, sizeof(float) * 48 * n_pairs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    staging_idle(c);
    unpack_results(c->h_out, n_pairs, x_out, pred_stds_out, cov_out);
    return ICET_OK;
}

// The constructor replacement in two halves.  icet_solve_begin enqueues the uploads, the whole registration and the copy of the results
// and returns while the device works (the scans must stay untouched until icet_solve_end: the runtime may still be reading them);
// icet_solve_end waits and fills the outputs named at begin.  What the host does in between -- the reference's constructor deep-copies
// both scans into its members (src/icet.cpp:30,33), include/icet.h does the same there -- overlaps with the device.
icet_status icet_solve_begin(icet_ctx* c, const icet_params* p, const float* scan1, int64_t n1, int64_t ld1,
                             const float* scan2, int64_t n2, int64_t ld2, const float x0[6],
                             float x_out[6], float pred_stds_out[6], float cov_out[36], icet_aux* aux) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (!params_ok(p) || n1 < 0 || n2 < 0 || ld1 < n1 || ld2 < n2 || (n1 > 0 && !scan1) || (n2 > 0 && !scan2) || !x0 || !x_out || !pred_stds_out) {
        c->err = "bad argument"; return ICET_ERR_BAD_ARG;
    }
    if (c->pend.active) { c->err = "icet_solve_begin without icet_solve_end on this context"; return ICET_ERR_BAD_ARG; }
    ICET_TRY(enter(c));
    const int V = p->bins_phi * p->bins_theta;
    const int64_t l1 = padded_ld(n1), l2 = padded_ld(n2);
    icet_status s = ensure_workspace(c, p, 1, l1, l2);
    if (s == ICET_OK) s = ensure_out(c, 1);
    if (s == ICET_OK) s = ensure_host_path(c);
    if (s == ICET_OK) s = ensure_stage(c, l1, l2);
    if (s == ICET_OK) s = ensure_pack(c, V, p->runlen);
    if (s != ICET_OK) return s;
    const bool want_pts2 = aux && aux->points2 && n2 > 0 && p->runlen > 0;
    auto grow_pts2 = [c](size_t want) -> icet_status {                        // `points2` on the device and its pinned copy
        BufferGroup& g = c->mem.pts2;
        HIPCHK(c, grow(g, c->cap_pts2, want, [&] { const int e = g.device(c->d_pts2, want); return e ? e : g.pinned(c->h_pts2, want); }));
        return ICET_OK;
    };
    if (want_pts2 && (p->flags & ICET_FLAG_ROUNDTRIP_SCAN2) && (size_t)3 * n2 > c->cap_pts2) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->st_copy) HIPCHK(c, hipStreamSynchronize(c->st_copy));
        const icet_status gs = grow_pts2((size_t)3 * n2 + (size_t)3 * n2 / 8);
        if (gs != ICET_OK) return gs;
    }
    const bool want_side1 = aux && p->runlen > 0 && n1 > 0 && (aux->points1_spherical || aux->point_index1 || aux->bin_start1);
    const bool want_side2 = aux && p->runlen > 0 && n2 > 0 && (aux->points2_spherical || aux->voxel2);
    if (want_side1 && (size_t)n1 > c->cap_side1) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        BufferGroup& g = c->mem.side1;
        HIPCHK(c, grow(g, c->cap_side1, n1, [&] { const int e = g.device(c->d_sph1, (size_t)3 * n1); return e ? e : g.device(c->d_idx1, (size_t)n1); }));
    }
    if (want_side2 && ((size_t)n2 > c->cap_side2 || (size_t)3 * n2 > c->cap_pts2)) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->st_copy) HIPCHK(c, hipStreamSynchronize(c->st_copy));
        BufferGroup& g = c->mem.side2;
        HIPCHK(c, grow(g, c->cap_side2, n2, [&] { const int e = g.device(c->d_sph2, (size_t)3 * n2); return e ? e : g.device(c->d_vox2, (size_t)n2); }));
        if ((size_t)3 * n2 > c->cap_pts2) { const icet_status gs = grow_pts2((size_t)3 * n2); if (gs != ICET_OK) return gs; }
    }
    ICET_TRY(staging_wait(c));
    // (no stream synchronisation up front: the staging buffers, the result block and the pinned x0 are only ever used by the host-pointer
    // entry points, each of which has drained the stream before it returned; the pinned descriptors are the device entries' too: the wait above)
    std::memcpy(c->h_x0, x0, 6 * sizeof(float));                              // pinned: k_init_state reads X0 straight from it (no H2D command)
    HIPCHK(c, upload_scan(c->d_stage1, l1, scan1, n1, ld1, c->stream));
    c->desc_kf_valid = c->desc_reg_valid = false;
    set_scan1(c->h_desc[0], icet_dev_scan{c->d_stage1, n1, l1}); set_scan2(c->h_desc[0], icet_dev_scan{c->d_stage2, n2, l2});
    const AuxLayout L = aux_layout(V, p->runlen);
    float* h_res = reinterpret_cast<float*>(c->h_pack) + L.out;               // the 48 result floats on the host
    float* d_res = reinterpret_cast<float*>(c->d_pack) + L.out;               // ... and where k_gn_solve writes them
    AuxDev ad = c->aux_dev;
    icet_ctx::Pending& q = c->pend;
    q = icet_ctx::Pending{};
    icet_status st = ICET_OK;
    if (p->runlen == 0) {
        // the reference's constructor leaves X = X0, pred_stds = 0 when runlen == 0 (src/icet.cpp:36-37,47); nothing to enqueue
        std::memset(h_res, 0, 48 * sizeof(float)); std::memcpy(h_res, x0, 6 * sizeof(float));
        if (aux && aux->points2 && n2 > 0)                                    // `points2` of an object that never iterated is its copy of scan 2 (src/icet.cpp:33)
            for (int k = 0; k < 3; k++) std::memcpy(aux->points2 + (size_t)k * n2, scan2 + (size_t)k * ld2, (size_t)n2 * sizeof(float));
    } else {
        if (aux) {
            const size_t rl = p->runlen, v = (size_t)V;
            // per-iteration integer tables: k_gn_solve writes the active voxels only, so they start from zero -- and are neither cleared
            // nor written when nobody asked for them
            if (aux->n2_raw) HIPCHK(c, hipMemsetAsync(ad.n2_raw, 0, sizeof(int32_t) * rl * v, c->stream)); else ad.n2_raw = nullptr;
            if (aux->n2_in) HIPCHK(c, hipMemsetAsync(ad.n2_in, 0, sizeof(int32_t) * rl * v, c->stream)); else ad.n2_in = nullptr;
            q.kf_tables = aux->cluster_bounds || aux->has_fit || aux->mu1 || aux->sigma1 || aux->evecs1 || aux->l_diag || aux->test_points;
            q.tail_ints = aux->n1_raw || aux->n2_raw || aux->n2_in;
            q.pts2 = want_pts2 && !want_side2; q.pts2_dev = q.pts2 && (p->flags & ICET_FLAG_ROUNDTRIP_SCAN2) != 0;
            q.side1 = want_side1; q.side2 = want_side2; q.n1 = n1;
            q.scan2 = scan2; q.ld2 = ld2;
            if (!want_pts2 && !want_side2) ad.xf_last = nullptr;
        }
        c->kf_pairs = 0; c->perm_active = false;
        LaunchCfg cfg; st = plan_pairs(c, p, 1, &cfg);
        if (st == ICET_OK) st = enqueue_keyframe(c, cfg, aux ? &ad : nullptr);
        if (st == ICET_OK && want_side1)                                       // points1Spherical / pointIndices1 from the tables the keyframe build has just left
            HIPCHK(c, launch_side_scan1(c->w, cfg, c->d_sph1, c->d_idx1, c->stream));
        if (st == ICET_OK) st = upload_scan2_beside(c, "scan-2 upload / table download", [&] { return upload_scan(c->d_stage2, l2, scan2, n2, ld2, c->st_copy); }, [&] {
            if (!q.kf_tables) return hipSuccess;
            // the keyframe tables are final now: they travel to the host on the copy stream while the loop iterates
            hipError_t e = hipEventRecord(c->ev_kf, c->stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(c->st_copy, c->ev_kf, 0);
            if (e == hipSuccess) e = hipMemcpyAsync(c->h_pack + L.bounds, c->d_pack + L.bounds, (L.kf_end - L.bounds) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st_copy);
            if (e == hipSuccess) e = hipEventRecord(c->ev_kfd, c->st_copy);
            return e;
        });
        if (st == ICET_OK) {
            LoopCall lc = pair_loop(c, cfg, c->h_x0, d_res, aux ? &ad : nullptr, false, c->ev_s2);
            lc.pts2_out = q.pts2_dev ? c->h_pts2 : nullptr;
            st = enqueue_loop(c, p, cfg, lc);
            if (st == ICET_OK) HIPCHK(c, hipMemcpyAsync(c->h_pack + L.out, c->d_pack + L.out, (aux ? L.small_end : 48) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        }
        if (st == ICET_OK && want_side2) {
            // points2 / points2Spherical / the rows' voxels of the LAST fitScan2: one kernel behind the loop, with the transform record that
            // iteration used (it reads the scan the loop read: the round-tripped copy under ICET_FLAG_ROUNDTRIP_SCAN2)
            Workspace wl = c->w; if (cfg.rt2) wl.desc = c->w.desc_rt;
            HIPCHK(c, launch_side_scan2(wl, cfg, ad.xf_last, c->d_pts2, c->d_sph2, c->d_vox2, c->stream));
        }
        if (st == ICET_OK && q.tail_ints)
            HIPCHK(c, hipMemcpyAsync(c->h_pack + L.n1_raw, c->d_pack + L.n1_raw, (L.ints_end - L.n1_raw) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    if (st != ICET_OK) { (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->st_copy); return st; }
    q.active = true; q.x_out = x_out; q.ps_out = pred_stds_out; q.cov_out = cov_out; q.has_aux = aux != nullptr && p->runlen > 0;
    q.aux = aux ? *aux : icet_aux{}; q.V = V; q.rl = p->runlen; q.n2 = n2;
    return ICET_OK;
}

// The keyframe half of a pending solve: returns when the keyframe tables named at begin (cluster_bounds, has_fit, mu1, sigma1, evecs1,
// l_diag, test_points) are in the caller's arrays -- the loop is still iterating on the device.  Optional; icet_solve_end does it otherwise.
icet_status icet_solve_keyframe_tables(icet_ctx* c) {
    if (!c) return ICET_ERR_BAD_ARG;
    icet_ctx::Pending& q = c->pend;
    if (!q.active) { c->err = "icet_solve_keyframe_tables without icet_solve_begin"; return ICET_ERR_BAD_ARG; }
    if (!q.has_aux || !q.kf_tables || q.kf_done) return ICET_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(c->ev_kfd));
    const AuxLayout L = aux_layout(q.V, q.rl);
    const icet_aux& a = q.aux; const size_t v = (size_t)q.V;
    auto add = [&](void* dst, size_t at, size_t n) { if (dst && n) std::memcpy(dst, c->h_pack + at, n * sizeof(uint32_t)); };
    add(a.cluster_bounds, L.bounds, v * 6); add(a.has_fit, L.has_fit, v); add(a.mu1, L.mu1, v * 3); add(a.sigma1, L.sigma1, v * 9);
    add(a.evecs1, L.evecs1, v * 9); add(a.l_diag, L.l_diag, v * 3); add(a.test_points, L.test_points, v * 18);
    q.kf_done = true;
    return ICET_OK;
}

icet_status icet_solve_end(icet_ctx* c) {
    if (!c) return ICET_ERR_BAD_ARG;
    icet_ctx::Pending& q = c->pend;
    if (!q.active) { c->err = "icet_solve_end without icet_solve_begin"; return ICET_ERR_BAD_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    // what is ready before the loop has finished is moved into the caller's arrays while the device still iterates
    icet_status ks = icet_solve_keyframe_tables(c);
    q.active = false;
    if (q.has_aux && q.pts2 && ks == ICET_OK) {
        if (q.pts2_dev) {
            HIPCHK(c, hipEventSynchronize(c->ev_pts2));
            std::memcpy(q.aux.points2, c->h_pts2, (size_t)3 * q.n2 * sizeof(float));
        } else {
            // the transform of the last iteration is known (its solve is still running): scan 2 is transformed here, under the device's last iteration
            HIPCHK(c, hipEventSynchronize(c->ev_prev));
            const AuxLayout Lp = aux_layout(q.V, q.rl);
            host_points2(reinterpret_cast<const float*>(c->h_pack) + Lp.xf_last, q.scan2, q.ld2, q.n2, q.aux.points2);
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (q.rl > 0) HIPCHK(c, hipStreamSynchronize(c->st_copy));
    if (ks != ICET_OK) return ks;
    const AuxLayout L = aux_layout(q.V, q.rl);
    const float* out = reinterpret_cast<const float*>(c->h_pack) + L.out;
    unpack_results(out, 1, q.x_out, q.ps_out, q.cov_out);
    if (q.has_aux) {
        const icet_aux& a = q.aux; const size_t rl = q.rl, v = (size_t)q.V;
        auto add = [&](void* dst, size_t at, size_t n) { if (dst && n) std::memcpy(dst, c->h_pack + at, n * sizeof(uint32_t)); };
        add(a.x_hist, L.x_hist, rl * 6); add(a.htwh, L.htwh, rl * 36); add(a.htwdz, L.htwdz, rl * 6); add(a.cond_info, L.cond, rl * 8);
        add(a.n1_raw, L.n1_raw, v); add(a.n2_raw, L.n2_raw, rl * v); add(a.n2_in, L.n2_in, rl * v);
        // the per-point tables go from HBM straight into the caller's arrays (several MB; only when asked for)
        if (q.side1) {
            if (a.points1_spherical) HIPCHK(c, hipMemcpy(a.points1_spherical, c->d_sph1, sizeof(float) * 3 * (size_t)q.n1, hipMemcpyDeviceToHost));
            if (a.point_index1) HIPCHK(c, hipMemcpy(a.point_index1, c->d_idx1, sizeof(int32_t) * (size_t)q.n1, hipMemcpyDeviceToHost));
            if (a.bin_start1) HIPCHK(c, hipMemcpy(a.bin_start1, c->w.bin_start, sizeof(int32_t) * (v + 1), hipMemcpyDeviceToHost));
        }
        if (q.side2) {
            if (a.points2) HIPCHK(c, hipMemcpy(a.points2, c->d_pts2, sizeof(float) * 3 * (size_t)q.n2, hipMemcpyDeviceToHost));
            if (a.points2_spherical) HIPCHK(c, hipMemcpy(a.points2_spherical, c->d_sph2, sizeof(float) * 3 * (size_t)q.n2, hipMemcpyDeviceToHost));
            if (a.voxel2) HIPCHK(c, hipMemcpy(a.voxel2, c->d_vox2, sizeof(int32_t) * (size_t)q.n2, hipMemcpyDeviceToHost));
        }
    }
    return ICET_OK;
}

icet_status icet_solve(icet_ctx* c, const icet_params* p, const float* scan1, int64_t n1, int64_t ld1,
                       const float* scan2, int64_t n2, int64_t ld2, const float x0[6],
                       float x_out[6], float pred_stds_out[6], float cov_out[36], icet_aux* aux) {
    const icet_status s = icet_solve_begin(c, p, scan1, n1, ld1, scan2, n2, ld2, x0, x_out, pred_stds_out, cov_out, aux);
    return s == ICET_OK ? icet_solve_end(c) : s;
}

icet_status icet_debug_fetch(icet_ctx* c, int32_t what, void* out, int64_t count) {
    if (!c || !out || count < 0) return ICET_ERR_BAD_ARG;
    const Workspace& w = c->w;
    if (what == 6) { if (count != 1) return ICET_ERR_BAD_ARG; *static_cast<int32_t*>(out) = c->lds_rank_ok; return ICET_OK; }   // no device array: the verdict of lds_rank_selftest
    const void* src = nullptr; int64_t cap = w.cap_n1; size_t elem = 4;
    switch (what) {
        case 0: src = w.r1; break;
        case 1: src = w.bin16; elem = 2; break;
        case 3: src = w.src; break;
        case 4: src = w.flags; cap = w.cap_pairs; break;
        case 5: src = w.rt2; cap = 3 * w.cap_rt2; break;      // ICET_FLAG_ROUNDTRIP_SCAN2: the round-tripped copy of scan 2 (x | y | z, leading dimension = n2 rounded up to 64)
        default: c->err = "unknown array id"; return ICET_ERR_BAD_ARG;
    }
    if (!src || count > cap) { c->err = "nothing to fetch / count too large"; return ICET_ERR_BAD_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, src, (size_t)count * elem, hipMemcpyDeviceToHost));
    if (what == 3) { uint32_t* o = static_cast<uint32_t*>(out); for (int64_t i = 0; i < count; i++) o[i] &= c->kf_row_mask; }      // packed rows: the rows without their voxel words
    return ICET_OK;
}

// Test hook: the 6x6 tail of an iteration (src/icet.cpp:410-433) on n host-side (HTWH, HTWdz), evaluated by the device function k_gn_solve runs.
icet_status icet_debug_gn_tail(icet_ctx* c, const float* htwh, const float* htwdz, int32_t n, float* out) {
    if (!c || !htwh || !htwdz || !out || n < 0) return ICET_ERR_BAD_ARG;
    if (n == 0) return ICET_OK;
    HIPCHK(c, hipSetDevice(c->device));
    float* d = nullptr; BufferGroup g;                                       // (freed at every return)
    HIPCHK(c, g.device(d, (size_t)n * (36 + 6 + 56)));
    float* d_H = d; float* d_g = d + (size_t)n * 36; float* d_o = d_g + (size_t)n * 6;
    hipError_t e = hipMemcpyAsync(d_H, htwh, sizeof(float) * (size_t)n * 36, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_g, htwdz, sizeof(float) * (size_t)n * 6, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_gn_tail_debug(d_H, d_g, d_o, n, (float)(c->tune.gn_cond_bound * c->tune.gn_cond_bound), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_o, sizeof(float) * (size_t)n * 56, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("icet_debug_gn_tail: ") + hipGetErrorString(e); return ICET_ERR_HIP; }
    return ICET_OK;
}

// Test hook: the per-voxel weight's pseudo-inverse under ICET_FLAG_REFERENCE_W (src/icet.cpp:320-321) on n host-side 3 x 3 matrices, through the device function the solve runs.
icet_status icet_debug_pinv3(icet_ctx* c, const float* a, int32_t n, float* out) {
    if (!c || !a || !out || n < 0) return ICET_ERR_BAD_ARG;
    if (n == 0) return ICET_OK;
    HIPCHK(c, hipSetDevice(c->device));
    float* d = nullptr; BufferGroup g;
    HIPCHK(c, g.device(d, (size_t)n * 18));
    hipError_t e = hipMemcpyAsync(d, a, sizeof(float) * (size_t)n * 9, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_pinv3_debug(d, d + (size_t)n * 9, n, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + (size_t)n * 9, sizeof(float) * (size_t)n * 9, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("icet_debug_pinv3: ") + hipGetErrorString(e); return ICET_ERR_HIP; }
    return ICET_OK;
}

// Test hook: the per-voxel weight's pseudo-inverse under ICET_FLAG_DOUBLE_W on n host-side packed symmetric 3 x 3 matrices, through the device function the solve runs.
icet_status icet_debug_pinv3_double(icet_ctx* c, const float* a, int32_t n, float* out) {
    if (!c || !a || !out || n < 0) return ICET_ERR_BAD_ARG;
    if (n == 0) return ICET_OK;
    HIPCHK(c, hipSetDevice(c->device));
    float* d = nullptr; BufferGroup g;
    HIPCHK(c, g.device(d, (size_t)n * 12));
    hipError_t e = hipMemcpyAsync(d, a, sizeof(float) * (size_t)n * 6, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_pinv3_double_debug(d, d + (size_t)n * 6, n, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + (size_t)n * 6, sizeof(float) * (size_t)n * 6, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("icet_debug_pinv3_double: ") + hipGetErrorString(e); return ICET_ERR_HIP; }
    return ICET_OK;
}

// Test hook: the float -> fixed-point conversions of the point pass (icet_device_common.h) on n host-side floats; out: n x 3 uint64 = to_fix_biased | to_fix_wide_biased | to_fix.
icet_status icet_debug_fix(icet_ctx* c, const float* v, int32_t n, uint64_t* out) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (!v || !out || n < 0) { c->err = "icet_debug_fix: bad argument"; return ICET_ERR_BAD_ARG; }
    if (n == 0) return ICET_OK;
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long* d = nullptr; BufferGroup g;
    HIPCHK(c, g.device(d, (size_t)n * 4));
    float* d_v = reinterpret_cast<float*>(d + (size_t)n * 3);
    hipError_t e = hipMemcpyAsync(d_v, v, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_fix_debug(d_v, d, n, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, sizeof(unsigned long long) * (size_t)n * 3, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("icet_debug_fix: ") + hipGetErrorString(e); return ICET_ERR_HIP; }
    return ICET_OK;
}

// Test hook: the device functions of the shared arithmetic rule (icet_device_common.h: c2s_cr, voxel_of, roundtrip_any, roundtrip_cr) on n host-side rows x[n] | y[n] | z[n]
// with leading dimension ld; out: 12 columns of n 32-bit words (k_spherical_debug, icet_keyframe.hip).
icet_status icet_debug_spherical(icet_ctx* c, const float* xyz, int32_t n, int32_t ld, int32_t T, int32_t P, float* out) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (!xyz || !out || n < 0 || ld < n || T < 1 || P < 1) { c->err = "icet_debug_spherical: bad argument"; return ICET_ERR_BAD_ARG; }
    if (n == 0) return ICET_OK;
    HIPCHK(c, hipSetDevice(c->device));
    float* d = nullptr; BufferGroup g;
    HIPCHK(c, g.device(d, (size_t)n * 15));
    float* d_o = d + (size_t)n * 3;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 3 && e == hipSuccess; k++) e = hipMemcpyAsync(d + (size_t)n * k, xyz + (size_t)ld * k, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_spherical_debug(d, n, n, T, P, d_o, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_o, sizeof(float) * (size_t)n * 12, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("icet_debug_spherical: ") + hipGetErrorString(e); return ICET_ERR_HIP; }
    return ICET_OK;
}

icet_status icet_set_option(icet_ctx* c, const char* name, double value) {
    if (!c || !name) return ICET_ERR_BAD_ARG;
    Tuning& t = c->tune;
    const std::string k(name);
    const int iv = (int)value;
    if (k == "lds_slots") t.lds_slots = iv < 0 ? 0 : iv;
    else if (k == "acc_pts") t.acc_pts = iv < 1 ? 1 : iv;
    else if (k == "acc_blocks") t.acc_blocks = iv < 1 ? 1 : iv;
    else if (k == "force_exact") t.force_exact = iv != 0;
    else if (k == "library_sort") {      // the name stays known: 0 is what the library does
        if (iv != 0) { c->err = "library_sort: the library has ONE sort, the hand-written rank sort, and no build flag brings another"; return ICET_ERR_UNSUPPORTED; }
    }
    else if (k == "kf_pts") t.kf_pts = iv < 1 ? 1 : (iv > kKfMaxPtsPerThread ? kKfMaxPtsPerThread : iv);
    else if (k == "batch_parts") t.batch_parts = iv < 0 ? 0 : (iv > 8 ? 8 : iv);
    else if (k == "batch_stage") t.batch_stage = (iv < 0 || iv > 4) ? 0 : iv;
    else if (k == "rs_cap") t.rs_cap = iv < 0 ? 0 : iv;
    else if (k == "rs_max_cell") t.rs_max_cell = iv < 0 ? 0 : iv;
    else if (k == "exec_bits_lds") t.exec_bits_lds = iv != 0;
    else if (k == "lds_rank") t.lds_rank = iv < 0 ? -1 : (iv != 0);
    else if (k == "packed_rows") t.packed_rows = iv < 0 ? -1 : (iv != 0);      // (1: a keyframe call whose shapes do not fit is refused, enqueue_keyframe)
    else if (k == "exec_pairwise") t.exec_pairwise = iv < 0 ? -1 : (iv != 0);
    else if (k == "fuse_solve") { t.fuse_solve = iv < 0 ? -1 : (iv != 0); c->g_solve.have_seen = c->g_keyframe.have_seen = c->g_loop.have_seen = false; }
    else if (k == "keep") t.keep = iv != 0;
    else if (k == "keep_from") t.keep_from = iv < 0 ? 0 : iv;
    else if (k == "keep_budget_t") { if (!(value > 0.0 && value <= 100.0)) { c->err = "keep_budget_t must lie in (0, 100]"; return ICET_ERR_BAD_ARG; } t.keep_budget_t = value; }
    else if (k == "keep_budget_r") { if (!(value > 0.0 && value <= 1.0)) { c->err = "keep_budget_r must lie in (0, 1]"; return ICET_ERR_BAD_ARG; } t.keep_budget_r = value; }
    else if (k == "keep_check_scale") t.keep_check_scale = value > 0 ? value : 1.0;      // timing experiments (Tuning)
    else if (k == "graph") { c->graph_mode = iv < 0 ? -1 : (iv != 0); c->g_solve.have_seen = c->g_keyframe.have_seen = c->g_loop.have_seen = false; }
    else if (k == "gn_cond_bound") { if (!(value >= 0.0 && value <= 1e6)) { c->err = "gn_cond_bound must lie in [0, 1e6]"; return ICET_ERR_BAD_ARG; } t.gn_cond_bound = value; c->g_solve.have_seen = c->g_keyframe.have_seen = c->g_loop.have_seen = false; }
    else if (k == "guard_scale") { if (!(value >= 1.0 && value <= 1024.0)) { c->err = "guard_scale must lie in [1, 1024]"; return ICET_ERR_BAD_ARG; } t.guard_scale = value; c->w.thr_T = 0; }   // tables are rebuilt by the next call
    else if (k == "lut_polar_quantile") { if (!(value >= 0.0 && value <= 1.0)) { c->err = "lut_polar_quantile must lie in [0, 1]"; return ICET_ERR_BAD_ARG; } t.lut_polar_quantile = value; c->w.thr_T = 0; }
    else if (k == "snapshot_chunk_bytes") { if (!(value >= 0.0 && value <= 1e12)) { c->err = "snapshot_chunk_bytes must lie in [0, 1e12] (0: the default, 64 MiB)"; return ICET_ERR_BAD_ARG; } c->snapshot_chunk_bytes = (int64_t)value; }
    else if (k == "pg_solver") { if (!(value == 0.0 || value == 1.0 || value == 2.0)) { c->err = "pg_solver must be 0 (conjugate gradients), 1 (direct) or 2 (auto)"; return ICET_ERR_BAD_ARG; } c->pg_solver = iv; }
    else if (k == "map_lds") c->map_lds = iv != 0;
    else if (k == "map_query_prune") c->map_query_prune = iv != 0;
    else if (k == "map_evidence_prune") c->map_evidence_prune = iv != 0;
    else if (k == "map_evidence_batch") { if (!(value >= 0.0 && value <= 256.0)) { c->err = "map_evidence_batch must lie in 0 .. 256 (0: automatic)"; return ICET_ERR_BAD_ARG; } c->map_evidence_batch = iv; }
    else if (k == "map_snapshot_chunk_entries") { if (!(value >= 0.0 && value <= 1073741824.0)) { c->err = "map_snapshot_chunk_entries must lie in 0 .. 2^30 (0: the default, 2^20)"; return ICET_ERR_BAD_ARG; } c->map_snapshot_chunk_entries = (int64_t)value; }
    else { c->err = "unknown option: " + k; return ICET_ERR_BAD_ARG; }
    return ICET_OK;
}

} // extern "C" (reopened below)
void icet_ctx_set_stream(icet_ctx* c, hipStream_t s) { if (c) c->stream = s; }
void icet_ctx_set_done_flag(icet_ctx* c, int32_t* pinned_word) { if (c) c->done_flag = pinned_word; }
void icet_ctx_set_prologue(icet_ctx* c, hipError_t (*fn)(void*, hipStream_t), void* user, int64_t key) { if (c) { c->prologue = fn; c->prologue_user = user; c->prologue_key = key; } }
extern "C" {
void* icet_stream(icet_ctx* c) { return c ? reinterpret_cast<void*>(c->stream) : nullptr; }
int icet_device(const icet_ctx* c) { return c ? c->device : -1; }

icet_status icet_last_timing(icet_ctx* c, float out_ms[4]) {
    if (!c || !out_ms) return ICET_ERR_BAD_ARG;
    if (!c->timing_valid) { c->err = "no timed call yet"; return ICET_ERR_BAD_ARG; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float a = 0, b = 0, acc = 0;
    HIPCHK(c, hipEventElapsedTime(&a, c->ev_a, c->ev_b));
    HIPCHK(c, hipEventElapsedTime(&b, c->ev_b, c->ev_c));
    for (int it = 0; it < c->last_iters; it++) { float t = 0; HIPCHK(c, hipEventElapsedTime(&t, c->ev_acc[2 * it], c->ev_acc[2 * it + 1])); acc += t; }
    out_ms[0] = a; out_ms[1] = b; out_ms[2] = c->last_iters ? acc : -1.f; out_ms[3] = (float)c->last_iters;
    return ICET_OK;
}

icet_status icet_last_timing_iters(icet_ctx* c, float* acc_ms, int32_t cap, int32_t* n_out) {
    if (!c || !acc_ms || !n_out || cap < 0) return ICET_ERR_BAD_ARG;
    if (!c->timing_valid) { c->err = "no timed call yet"; return ICET_ERR_BAD_ARG; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int n = c->last_iters < cap ? c->last_iters : cap;
    for (int it = 0; it < n; it++) HIPCHK(c, hipEventElapsedTime(&acc_ms[it], c->ev_acc[2 * it], c->ev_acc[2 * it + 1]));
    *n_out = n;
    return ICET_OK;
}

icet_status icet_keep_stats(icet_ctx* c, int32_t n_pairs, int32_t* out) {
    if (!c || !out || n_pairs < 0) return ICET_ERR_BAD_ARG;
    if (!c->w.keep_state || n_pairs > c->w.cap_keep_pairs) { c->err = "no keep-list state for that many pairs (the last call did not use the keep list)"; return ICET_ERR_BAD_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<KeepState> h((size_t)n_pairs);
    HIPCHK(c, hipMemcpy(h.data(), c->w.keep_state, sizeof(KeepState) * (size_t)n_pairs, hipMemcpyDeviceToHost));
    for (int s = 0; s < n_pairs; s++) {
        const int k = (c->perm_active && c->perm_pairs == n_pairs) ? c->h_seg[n_pairs + 1 + s] : s;      // (a ragged batch sits XCD-balanced in the tables: back to the caller's order)
        out[4 * k] = h[s].mode; out[4 * k + 1] = h[s].n_keep; out[4 * k + 2] = h[s].list_passes; out[4 * k + 3] = h[s].builds;
    }
    return ICET_OK;
}

}  // extern "C"
