// icet_amd/csrc/icet_posegraph_robust.h -- the kernel bodies of the pose-graph optimiser's ROBUST KERNELS (DESIGN.md section 20 "Robust kernels"): iteratively
// reweighted least squares over the machinery of icet_posegraph_body.h.  HIP-free, behind that header's macros: device code under hipcc, one host thread under a
// host compiler, four with a barrier under ICET_PG_EMU (tests/cpp/test_posegraph_robust.cpp).  icet_posegraph.hip has the launches, icet_posegraph_driver.h
// (PgRobustPolicy) the places they run at.
//
// The rule is icet_posegraph.h's (robust_rho, robust_weight): the objective is F = sum rho(chi2_e), an edge's weight w_e = rho'(chi2_e) at the current poses
// scales its Omega J, and everything behind that -- the assembly, the band's factor, both linear solves -- is unchanged.  No atomics, no block waits on another,
// no per-thread array takes a run-time index.
#pragma once
#include "icet_posegraph_body.h"

namespace icet {

// raw sums of chi2 kept beside the scalars (whose slot kScChi holds F): the start's | the last trial's | the returned poses'
constexpr int kPgRobustRaw = 3;
enum PgRawSlot { kPgRawStart = 0, kPgRawTrial = 1, kPgRawFinal = 2 };

// The robust run's own arguments (pg_bind_robust), beside PgArgs.
struct PgRobust {
    int kind, flags;                // icet_pose_graph_robust
    int raw_slot;                   // kPgRobustStats: the slot of raw it writes
    double scale;
    double* wt;                     // E: the weights of the last linearisation, then (kPgRobustFinish) of the returned poses; null in a run with kind 0
    double* raw;                    // kPgRobustRaw: the raw sum of chi2 (the scalars' own slot kScChi holds F); null in a run with kind 0
    double* weight_out;             // E, the caller's (may be null)
};

enum PgRobustGridKernel { kPgRobustScale = 0, kPgRobustFinish };
enum PgRobustGroupKernel { kPgRobustStats = 0 };

ICET_PG_DEV int pg_robust_kind(const PgArgs& a, const PgRobust& r, int e) { return pg::robust_kind_of_edge(r.kind, r.flags, a.N, e); }

// gi < E x 72, between kPgLinearise and kPgAssemble: entry gi of Omega J times its edge's weight at the current chi2; the edge's first thread records the weight
ICET_PG_DEV void pg_robust_scale(const PgArgs& a, const PgRobust& r, int gi) {
    const int e = gi / 72;
    const double w = pg::robust_weight(pg_robust_kind(a, r, e), r.scale, a.chi[e]);
    a.OJ[gi] *= w;
    if (gi % 72 == 0) r.wt[e] = w;
}

// e < E: the weight at the chi2 of the RETURNED poses (the start's after a failed run), 1 for an edge the flags leave alone
ICET_PG_DEV void pg_robust_finish(const PgArgs& a, const PgRobust& r, int e) {
    const double w = pg::robust_weight(pg_robust_kind(a, r, e), r.scale, a.failed ? a.chi0[e] : a.chi[e]);
    if (r.wt) r.wt[e] = w;
    if (r.weight_out) r.weight_out[e] = w;
}

// One workgroup, in the place of kPgStats: F = sum rho(chi2_e) where the accept rule reads the sum of chi2, the raw sum beside it, max |dx| as pg_group_stats
// takes it.  The same tree of kPgLanes lanes: one order for any thread count.
ICET_PG_DEV double pg_robust_tree(PgRed& red) {
    const int t = ICET_PG_TID;
    ICET_PG_SYNC();
    for (int h = kPgLanes / 2; h > 0; h >>= 1) {
        for (int l = t; l < h; l += kPgThreads) red.lane[l] += red.lane[l + h];
        ICET_PG_SYNC();
    }
    const double s = red.lane[0];
    ICET_PG_SYNC();
    return s;
}
ICET_PG_DEV void pg_group_robust_stats(const PgArgs& a, const PgRobust& r, PgRed& red) {
    const int t = ICET_PG_TID;
    const double* chi = a.trial ? a.chit : a.chi;
    for (int l = t; l < kPgLanes; l += kPgThreads) {
        double s = 0.0;
        for (int i = l; i < a.E; i += kPgLanes) s += pg::robust_rho(pg_robust_kind(a, r, i), r.scale, chi[i]);
        red.lane[l] = s;
    }
    const double cost = pg_robust_tree(red);
    for (int l = t; l < kPgLanes; l += kPgThreads) {
        double s = 0.0;
        for (int i = l; i < a.E; i += kPgLanes) s += chi[i];
        red.lane[l] = s;
    }
    const double raw = pg_robust_tree(red);
    if (t == 0) { a.sc[kScChi] = cost; r.raw[r.raw_slot] = raw; }
    for (int l = t; l < kPgLanes; l += kPgThreads) {
        double s = 0.0;
        for (int i = l; i < a.N * 6; i += kPgLanes) { const double v = fabs(a.x[i]); if (v > s) s = v; }
        red.lane[l] = s;
    }
    ICET_PG_SYNC();
    for (int h = kPgLanes / 2; h > 0; h >>= 1) {
        for (int l = t; l < h; l += kPgThreads) if (red.lane[l + h] > red.lane[l]) red.lane[l] = red.lane[l + h];
        ICET_PG_SYNC();
    }
    if (t == 0) a.sc[kScMaxDx] = red.lane[0];
    ICET_PG_SYNC();
}
}  // namespace icet
