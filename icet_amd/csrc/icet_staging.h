// icet_amd/csrc/icet_staging.h -- the words the host stages for the device, and the small host rules over them: a pair's descriptor and its two halves, the check
// of a call's device scans, the layout of a call's descriptors (offsets, segment table, totals: lay_out_staging), the layout of host scans in the staging buffers, and the unpacking of the 48 result floats.  Nothing of HIP in here (a host test
// includes it); who may write the pinned descriptors, and when, is icet_ctx.h (staging_wait / staging_mark_read / staging_upload).
#pragma once
#include "../../include/icet_hip.h"
#include <cstdint>
#include <cstring>

namespace icet {

struct PairDesc {
    const float* s1; const float* s2;
    int32_t n1, ld1, n2, ld2;
    int32_t off1;                    // start of this pair's segment in the scan-1 temporaries
    int32_t off2;                    // start of this pair's segment in the scan-2 overflow list (near_over)
};

inline bool dev_scan_ok(const icet_dev_scan& a) { return !(a.n < 0 || a.ld < a.n || (a.n > 0 && !a.ptr) || a.ld >= ((int64_t)1 << 30)); }

// The `count` device scans of a call: false at the first bad one, else their rows in *rows.
inline bool dev_scans_ok(const icet_dev_scan* scan, int32_t count, int64_t* rows) {
    int64_t tot = 0;
    for (int k = 0; k < count; k++) { if (!dev_scan_ok(scan[k])) return false; tot += scan[k].n; }
    *rows = tot;
    return true;
}

// The two halves of a descriptor.  A new scan 1 makes a new pair: its scan-2 half and the offsets (lay_out_staging, below, fills those) are reset.
inline void set_scan1(PairDesc& d, const icet_dev_scan& a) { d.s1 = a.ptr; d.n1 = (int32_t)a.n; d.ld1 = (int32_t)a.ld; d.s2 = nullptr; d.n2 = 0; d.ld2 = 0; d.off1 = 0; d.off2 = 0; }
inline void set_scan2(PairDesc& d, const icet_dev_scan& b) { d.s2 = b.ptr; d.n2 = (int32_t)b.n; d.ld2 = (int32_t)b.ld; }
inline bool same_scan1(const PairDesc& d, const icet_dev_scan& a) { return d.s1 == a.ptr && d.n1 == (int32_t)a.n && d.ld1 == (int32_t)a.ld; }
inline bool same_scan2(const PairDesc& d, const icet_dev_scan& b) { return d.s2 == b.ptr && d.n2 == (int32_t)b.n && d.ld2 == (int32_t)b.ld; }

// THE LAYOUT OF A CALL'S STAGING: pair k's segments start where those of the pairs before it end -- off1 in the scan-1 temporaries, off2 in the scan-2 overflow
// list --, and hs (the segment table; null where a call has none: an indexed call stages its keyframe index there) holds the n + 1 scan-1 offsets.  Every call
// lays its staging out exactly once, behind its last write of a descriptor and before it builds its plan, its graph key or its enqueuers: a replayed graph runs
// no enqueuer and re-reads these very words.  Laying out again writes the same words (the same_desc shortcut of the two halves relies on that).
// Returns what a plan needs of the descriptors (make_cfg, icet_capi.hip); vec4_ok: every scan-2 pointer and leading dimension is 16-byte aligned.
struct StagingTotals { int64_t total_n1 = 0, total_n2 = 0; int32_t max_n1 = 0, max_n2 = 0; int32_t vec4_ok = 1; };
inline StagingTotals lay_out_staging(PairDesc* hd, int32_t* hs, int n) {
    StagingTotals t;
    for (int k = 0; k < n; k++) {
        if ((reinterpret_cast<uintptr_t>(hd[k].s2) & 15u) || (hd[k].ld2 & 3)) t.vec4_ok = 0;
        if (hs) hs[k] = (int32_t)t.total_n1;
        hd[k].off1 = (int32_t)t.total_n1; t.total_n1 += hd[k].n1;
        hd[k].off2 = (int32_t)t.total_n2; t.total_n2 += hd[k].n2;
        t.max_n1 = hd[k].n1 > t.max_n1 ? hd[k].n1 : t.max_n1; t.max_n2 = hd[k].n2 > t.max_n2 ? hd[k].n2 : t.max_n2;
    }
    if (hs) hs[n] = (int32_t)t.total_n1;
    return t;
}

// Host scans in a staging buffer: column-major, leading dimension = rows rounded up to 64, back to back (3 x ld floats each).
inline int64_t padded_ld(int64_t n) { return (n + 63) / 64 * 64; }
// The layout of `count` scans of n[k] rows from `base` on; returns the rows to ask ensure_stage for (3 floats each).  out == nullptr: the total alone
// (the buffer may move when it grows: lay out after).
inline int64_t stage_layout(const int64_t* n, int32_t count, float* base, icet_dev_scan* out) {
    int64_t o = 0;
    for (int k = 0; k < count; k++) {
        const int64_t l = padded_ld(n[k]);
        if (out) out[k] = icet_dev_scan{base + 3 * o, n[k], l};
        o += l;
    }
    return o;
}

// n x 48 result floats (X | pred_stds | cov, icet_solve_body.h) into the caller's arrays; cov may be null.
inline void unpack_results(const float* res, int32_t n, float* x, float* pred_stds, float* cov) {
    for (int k = 0; k < n; k++) {
        std::memcpy(x + 6 * k, res + 48 * k, 6 * sizeof(float));
        std::memcpy(pred_stds + 6 * k, res + 48 * k + 6, 6 * sizeof(float));
        if (cov) std::memcpy(cov + 36 * k, res + 48 * k + 12, 36 * sizeof(float));
    }
}

}  // namespace icet
