// icet_amd/csrc/icet_posegraph_driver.h -- the pose-graph optimiser's driver, written ONCE: the Gauss-Newton loop, the preconditioned
// conjugate gradients, the direct solve over the closures (pg_direct_solve), the accept rule and what a failure returns.  HIP-free.  It runs the bodies of icet_posegraph_body.h through a BACKEND that launches a
// kernel (or loops over its index range on the host) and reads the few scalars back:
//     bool grid(PgGridKernel, int count, const PgArgs&)      the body for every global index below count (count 0: nothing)
//     bool group(PgGroupKernel, const PgArgs&)               the body as one workgroup
//     bool scalars(const PgArgs&, double out[kPgScalars])    wait for what was enqueued, then a.sc on the host
//     bool fetch(void* host, const void* dev, size_t bytes), put(void* dev, const void* host, size_t bytes)      (the test hook only) copies, complete on return
//     bool dgrid(PgDirectGridKernel, int count, const PgArgs&, const PgDirect&), dgroup(PgDirectGroupKernel, const PgArgs&, const PgDirect&)
//                                                            the direct solve's bodies (icet_posegraph_direct.h); only pg_direct_solve and pg_marginals call them
//     bool mgrid(PgMargGridKernel, int count, const PgArgs&, const PgDirect&, const PgMarg&)
//     bool mgroups(PgMargGroupKernel, int groups, const PgArgs&, const PgDirect&, const PgMarg&)
//                                                            the marginals' bodies (icet_posegraph_marginals.h); mgroups runs a group body once per group index
//                                                            below `groups` (one workgroup each; the host loops over them); only pg_marginals calls them
//     bool rgrid(PgRobustGridKernel, int count, const PgArgs&, const PgRobust&), rgroup(PgRobustGroupKernel, const PgArgs&, const PgRobust&)
//                                                            the robust kernels' bodies (icet_posegraph_robust.h); only PgRobustPolicy and pg_optimise_robust call
//                                                            them, so a backend without them still runs every other driver
//     bool xgroups(PgCrossGroupKernel, int groups, const PgArgs&, const PgDirect&, const PgMarg&, const PgCross&, const PgGate&)
//                                                            the columns' and the gate's bodies (icet_posegraph_cross.h), once per group index below `groups`;
//                                                            only pg_columns and pg_gate call them
// each false for a failure of the backend (the driver then returns false at once).  icet_posegraph.hip has the device's backend (PgDeviceBackend),
// tests/cpp/posegraph_host.h the host's (HostBackend), which the three host programs beside it share.
// The sequences of launches that every run repeats are named once (pg_phase_*, below); the four drivers -- pg_gauss_newton, pg_marginals and the two hooks --
// are made of them.
#pragma once
#include "icet_posegraph_body.h"
#include "icet_posegraph_direct.h"
#include "icet_posegraph_marginals.h"
#include "icet_posegraph_cross.h"
#include "icet_posegraph_robust.h"

#include <cmath>
#include <vector>

namespace icet {

constexpr double kPgDefaultPcgTol = 1e-10;

inline icet_pose_graph_options pg_default_options() { icet_pose_graph_options o; o.gn_iters = 10; o.max_pcg = 0; o.dx_tol = 1e-7; o.damping = 0.0; o.pcg_tol = kPgDefaultPcgTol; return o; }

// The graph on the host: the edges' ends, the incidence lists, the count of closures that lie off the band between two free nodes.
struct PgGraph {
    std::vector<int32_t> ei, ej, off, items;
    std::vector<int32_t> ends, end_of;      // the direct solve: the distinct ends of the closures counted by c_offband, ascending | per node its index in ends or -1
    int c_offband = 0;
    void build(int N, int C, const int32_t* ci, const int32_t* cj, const uint8_t* fixed) {
        pg::build_incidence(N, C, ci, cj, fixed, ei, ej, off, items);
        c_offband = 0;
        end_of.assign((size_t)N, -1);
        for (int c = 0; c < C; c++) {
            const int i = ci[c], j = cj[c];
            if ((i - j >= 2 || j - i >= 2) && off[i + 1] != off[i] && off[j + 1] != off[j]) { c_offband++; end_of[i] = 0; end_of[j] = 0; }
        }
        ends.clear();
        for (int k = 0; k < N; k++) if (end_of[k] == 0) { end_of[k] = (int32_t)ends.size(); ends.push_back(k); }
    }
};

// Every work array of a run, each at its exact size: al.d(count) hands out doubles, al.i(count) int32.
struct PgGraphDev { int32_t *ei, *ej, *off, *items; };      // where the backend puts PgGraph's four lists
template <class Alloc>
inline PgGraphDev pg_bind(PgArgs& a, Alloc& al, size_t n_items) {
    const size_t N = (size_t)a.N, E = (size_t)a.E, C = (size_t)a.C;
    a.P = al.d(N * 12); a.Pt = al.d(N * 12);
    a.Om = al.d(E * 36); a.J = al.d(E * 72); a.OJ = al.d(E * 72); a.res = al.d(E * 6);
    a.chi0 = al.d(E); a.chi = a.chi0; a.chit = al.d(E);
    a.D = al.d(N * 36); a.B = al.d(N * 36); a.G = al.d(N * 36); a.W = al.d(N * 36);
    a.A = al.d(C * 36);
    a.g = al.d(N * 6); a.x = al.d(N * 6); a.r = al.d(N * 6); a.z = al.d(N * 6); a.p = al.d(N * 6); a.q = al.d(N * 6); a.u = al.d(N * 6);
    a.sc = al.d(kPgScalars);
    a.spare_chi = al.d(E);
    PgGraphDev gd;
    gd.ei = al.i(E); gd.ej = al.i(E); gd.off = al.i(N + 1); gd.items = al.i(n_items);
    a.ei = gd.ei; a.ej = gd.ej; a.off = gd.off; a.items = gd.items;
    return gd;
}

// ---- the policy of a Gauss-Newton run: what differs between the plain run and a robust one, so that the loop, the accept rule and the failure semantics stay
// written once.  reweight runs between kPgLinearise and kPgAssemble; stats closes pg_phase_start and pg_phase_trial (it leaves the objective in sc[kScChi] and
// max |dx| in sc[kScMaxDx]); finish runs behind kPgFinish with the run's final arguments.  A policy has no state that changes during a run.
struct PgPlainPolicy {
    template <class Backend> bool reweight(Backend&, const PgArgs&) const { return true; }
    template <class Backend> bool stats(Backend& be, const PgArgs& a) const { return be.group(kPgStats, a); }
    template <class Backend> bool finish(Backend&, const PgArgs&) const { return true; }
};
// The robust run (icet_posegraph_robust.h): the weights at the current chi2 scale Omega J, the objective is F = sum rho(chi2).  The raw sum of chi2 goes to
// r.raw: kPgRawStart at the start, kPgRawTrial for every trial (a trial that is refused ends the run, so this slot says nothing at the end), and kPgRawFinal by
// one more launch of the stats kernel over the row of the RETURNED poses behind the weights -- nothing on the host follows which trial was kept.
struct PgRobustPolicy {
    PgRobust r;
    explicit PgRobustPolicy(const PgRobust& r_) : r(r_) {}
    template <class Backend> bool stats_into(Backend& be, const PgArgs& a, int slot) const { PgRobust q = r; q.raw_slot = slot; return be.rgroup(kPgRobustStats, a, q); }
    template <class Backend> bool reweight(Backend& be, const PgArgs& a) const { return be.rgrid(kPgRobustScale, a.E * 72, a, r); }
    template <class Backend> bool stats(Backend& be, const PgArgs& a) const { return stats_into(be, a, a.trial ? kPgRawTrial : kPgRawStart); }
    template <class Backend> bool finish(Backend& be, const PgArgs& a) const {
        PgArgs b = a;
        b.trial = 0;
        if (a.failed) b.chi = a.chi0;          // (the outputs are the inputs: their row is the start's)
        return be.rgrid(kPgRobustFinish, a.E, a, r) && stats_into(be, b, kPgRawFinal);
    }
};

// ---- the phases: the sequences of launches the drivers share, each false for a failure of the backend ----------------------------------------------------
// (the test hooks) count doubles from the device to dst; a null dst is skipped
template <class Backend>
inline bool pg_get(Backend& be, double* dst, const double* src, size_t count) { return !dst || count == 0 || be.fetch(dst, src, count * sizeof(double)); }

// The poses and the information matrices in place, every edge's chi2 at them
template <class Backend>
inline bool pg_phase_init(Backend& be, const PgArgs& a) {
    const int n_init = a.N * 12 > a.E * 36 ? a.N * 12 : a.E * 36;
    return be.grid(kPgInit, n_init, a) && be.grid(kPgChi, a.E, a);
}
// The start of a run: pg_phase_init, then the sum of the chi2 in the scalars, read into h
template <class Backend, class Policy>
inline bool pg_phase_start(Backend& be, const PgArgs& a, double h[kPgScalars], Policy& pol) { return pg_phase_init(be, a) && pol.stats(be, a) && be.scalars(a, h); }
template <class Backend>
inline bool pg_phase_start(Backend& be, const PgArgs& a, double h[kPgScalars]) { PgPlainPolicy pol; return pg_phase_start(be, a, h, pol); }
// The normal equations at the current poses: D, B, A and g
template <class Backend, class Policy>
inline bool pg_phase_linearise(Backend& be, const PgArgs& a, Policy& pol) {
    return be.grid(kPgLinearise, a.E * 12, a) && pol.reweight(be, a) && be.grid(kPgAssemble, a.N * 36, a) && be.grid(kPgOffband, a.C * 36, a);
}
template <class Backend>
inline bool pg_phase_linearise(Backend& be, const PgArgs& a) { PgPlainPolicy pol; return pg_phase_linearise(be, a, pol); }
// ... and the band's factor behind them: what a linear solve starts from
template <class Backend, class Policy>
inline bool pg_phase_factor(Backend& be, const PgArgs& a, Policy& pol) { return pg_phase_linearise(be, a, pol) && be.group(kPgFactor, a); }
template <class Backend>
inline bool pg_phase_factor(Backend& be, const PgArgs& a) { PgPlainPolicy pol; return pg_phase_factor(be, a, pol); }
// The trial poses P (+) x, their chi2 and the step's length in the scalars, read into h.  a.trial is set for these launches alone.
template <class Backend, class Policy>
inline bool pg_phase_trial(Backend& be, PgArgs& a, double h[kPgScalars], Policy& pol) {
    a.trial = 1;
    const bool ok = be.grid(kPgRetract, a.N, a) && be.grid(kPgChi, a.E, a) && pol.stats(be, a) && be.scalars(a, h);
    a.trial = 0;
    return ok;
}
template <class Backend>
inline bool pg_phase_trial(Backend& be, PgArgs& a, double h[kPgScalars]) { PgPlainPolicy pol; return pg_phase_trial(be, a, h, pol); }
// The direct solve's factorisation behind the band's factor (q = d.nq > 0): Z, Wm and its factor, Ks and its factor
template <class Backend>
inline bool pg_phase_direct_factor(Backend& be, const PgArgs& a, const PgDirect& d) {
    const int q = d.nq;
    return be.dgrid(kPgZ, q, a, d) && be.dgrid(kPgWm, q * q, a, d) && be.dgroup(kPgCholW, a, d) && be.dgrid(kPgSl, q * q, a, d) && be.dgrid(kPgKs, q * q, a, d) &&
           be.dgroup(kPgCholK, a, d);
}
// (the test hooks) q = H p for each of the caller's K vectors, through the kernel CG uses; a null q: nothing
template <class Backend>
inline bool pg_phase_hp(Backend& be, const PgArgs& a, int K, const double* p, double* q) {
    const size_t n6 = (size_t)a.N * 6, sd = sizeof(double);
    for (int k = 0; k < K && q; k++)
        if (!be.put(a.p, p + (size_t)k * n6, n6 * sd) || !be.grid(kPgHp, a.N * 6, a) || !be.fetch(q + (size_t)k * n6, a.q, n6 * sd)) return false;
    return true;
}

// The band solves one linear solve may take.  H = M + R: with no closure off the band H is the band, and the first preconditioned step is the exact solve.
inline int pg_cg_cap(int c_offband, const icet_pose_graph_options& o) { return c_offband == 0 ? 1 : (o.max_pcg > 0 ? o.max_pcg : 12 * c_offband + 8); }

// How a linear solve ended (icet_pose_graph_step.cg_end): at pcg_tol, at r.z == 0, at the cap, or in a failure (*bad then has the status).
enum PgCgEnd { kPgCgTolerance = 0, kPgCgZero = 1, kPgCgCap = 2, kPgCgFailed = 3 };

// ONE linear solve H x = -g by preconditioned conjugate gradients, behind kPgFactor: at most `cap` band solves, *pcg counts them on.  The optimiser and the test
// hook (pg_debug_step) both run this.  rec (may be null; 2 x cap doubles): per band solve its r.z | the p.Hp of the step behind it (NaN where no step followed);
// only a recording run reads the scalars once more behind the last step.
template <class Backend>
inline bool pg_cg(Backend& be, PgArgs& a, int cap, double pcg_tol, int* pcg, int* bad, int* end = nullptr, double* rec = nullptr) {
    double h[kPgScalars];
    int why = kPgCgCap, ci = 0;
    *bad = 0;
    for (; ci < cap; ci++) {
        a.first = ci == 0;
        if (!be.group(kPgPrecond, a) || !be.scalars(a, h)) return false;
        if (rec && ci > 0) rec[2 * (ci - 1) + 1] = h[kScPq];
        if (h[kScFactor] != 0.0) { *bad = (int)h[kScFactor]; break; }
        if (h[kScCg] != 0.0) { *bad = (int)h[kScCg]; break; }
        ++*pcg;
        const double rz = h[kScRz], rz0 = h[kScRz0];
        if (rec) { rec[2 * ci] = rz; rec[2 * ci + 1] = std::nan(""); }
        if (!std::isfinite(rz)) { *bad = pg::kNonFinite; break; }
        if (rz < 0.0) { *bad = pg::kNotPositiveDefinite; break; }
        if (rz == 0.0) { why = kPgCgZero; break; }
        if (ci > 0 && std::sqrt(rz / rz0) <= pcg_tol) { why = kPgCgTolerance; break; }
        if (!be.grid(kPgHp, a.N * 6, a) || !be.group(kPgStep, a)) return false;
    }
    if (*bad) why = kPgCgFailed;
    if (rec && ci == cap && cap > 0) {
        if (!be.scalars(a, h)) return false;
        rec[2 * (cap - 1) + 1] = h[kScPq];
    }
    if (end) *end = why;
    return true;
}

// The Gauss-Newton loop, written once over the LINEAR SOLVE: solve(a, &pcg, &bad) runs behind kPgFactor, leaves dx in a.x, counts its band solves on and sets
// *bad to a failure's status; false for a failure of the backend.  `pol` (PgPlainPolicy, PgRobustPolicy) names the objective: chi2_initial and chi2_final
// of *res are the objective's values, the sum of chi2 in a plain run.
template <class Backend, class Solve, class Policy>
inline bool pg_gauss_newton(Backend& be, PgArgs a, const icet_pose_graph_options& o, Solve&& solve, int solver, icet_pose_graph_result* res, Policy& pol) {
    double h[kPgScalars];
    const int N = a.N, E = a.E;
    a.damping = o.damping; a.trial = 0; a.first = 0; a.failed = 0;
    if (!pg_phase_start(be, a, h, pol)) return false;
    const double chi2_initial = h[kScChi];
    double chi2 = chi2_initial, max_dx = 0.0;
    int status = pg::kIterationCap, its = 0, pcg = 0;
    bool failed = false;
    if (!std::isfinite(chi2)) { status = pg::kNonFinite; failed = true; }
    for (int it = 0; it < o.gn_iters && !failed; it++) {
        its++;
        if (!pg_phase_factor(be, a, pol)) return false;
        int bad = 0;
        if (!solve(a, &pcg, &bad)) return false;
        if (bad) { status = bad; failed = true; break; }
        if (!pg_phase_trial(be, a, h, pol)) return false;
        if (h[kScCg] != 0.0) { status = (int)h[kScCg]; failed = true; break; }
        max_dx = h[kScMaxDx];
        const double chit = h[kScChi];
        if (!std::isfinite(chit)) { status = pg::kNonFinite; failed = true; break; }
        if (!(chit < chi2)) { status = max_dx < o.dx_tol ? pg::kConverged : pg::kStalled; break; }
        {   // accepted: the trial poses and their chi2 row become the current ones; the start's row is never a trial row
            double* t = a.P; a.P = a.Pt; a.Pt = t;
            double* c = a.chi; a.chi = a.chit; a.chit = c == a.chi0 ? a.spare_chi : c;
        }
        chi2 = chit;
        if (max_dx < o.dx_tol) { status = pg::kConverged; break; }
    }
    a.failed = failed ? 1 : 0;
    const int n_fin = N > E ? N : E;
    if (!be.grid(kPgFinish, n_fin, a) || !pol.finish(be, a) || !be.scalars(a, h)) return false;
    res->chi2_initial = chi2_initial; res->chi2_final = failed ? chi2_initial : chi2; res->max_dx = max_dx;
    res->status = status; res->gn_iterations = its; res->pcg_iterations = pcg; res->solver = solver;
    return true;
}

// The run.  `a` is bound (pg_bind), the graph uploaded, the caller's arrays in place.  true: *res is the result (its status says how the run ended).
template <class Backend, class Policy>
inline bool pg_optimise(Backend& be, PgArgs a, const icet_pose_graph_options& o, int c_offband, icet_pose_graph_result* res, Policy& pol) {
    const double pcg_tol = o.pcg_tol > 0.0 ? o.pcg_tol : kPgDefaultPcgTol;
    const int cap = pg_cg_cap(c_offband, o);
    return pg_gauss_newton(be, a, o, [&](PgArgs& b, int* pcg, int* bad) { return pg_cg(be, b, cap, pcg_tol, pcg, bad); }, 0, res, pol);
}
template <class Backend>
inline bool pg_optimise(Backend& be, PgArgs a, const icet_pose_graph_options& o, int c_offband, icet_pose_graph_result* res) {
    PgPlainPolicy pol;
    return pg_optimise(be, a, o, c_offband, res, pol);
}

// ---- the direct solve (icet_posegraph_direct.h) --------------------------------------------------------------------------------------------------------------
// Its work arrays, each at its exact size, beside pg_bind's in the same block: m end nodes, nq = 6 m.  Doubles first, then the two int32 lists.
struct PgDirectDev { int32_t *ends, *end_of; };
template <class Alloc>
inline PgDirectDev pg_bind_direct(const PgArgs& a, PgDirect& d, Alloc& al, size_t m) {
    const size_t N = (size_t)a.N, q = 6 * m;
    d.nq = (int)q; d.refine = 0;
    d.Z = al.d(N * 6 * q);
    d.Wm = al.d(q * q); d.Lw = al.d(q * q); d.SL = al.d(q * q); d.Ks = al.d(q * q); d.Lk = al.d(q * q);
    d.rdw = al.d(q); d.rdk = al.d(q); d.cv = al.d(q); d.ct = al.d(q); d.cu = al.d(q); d.cw = al.d(q);
    d.y = al.d(N * 6);
    PgDirectDev dd;
    dd.ends = al.i(m); dd.end_of = al.i(N);
    d.ends = dd.ends; d.end_of = dd.end_of;
    return dd;
}

// What the test hook copies out of one direct solve (null: nothing)
struct PgDirectTap { double *Z = nullptr, *Wm = nullptr, *L = nullptr, *Ks = nullptr, *Lk = nullptr, *x0 = nullptr; };

// ONE linear solve H x = -g by the direct method, behind kPgFactor (which leaves r = -g): Z, Wm, its factor, Ks, its factor, x = apply(-g), then kPgDirectRefine
// steps x += apply(-g - H x).  A fixed number of launches whatever the closures are; with no end node the single band solve.  Nothing is read back here: every
// kernel behind a failed factorisation returns at once, and the caller reads the statuses with the scalars (pg_direct_status).
template <class Backend>
inline bool pg_direct_solve(Backend& be, PgArgs& a, PgDirect& d, int* pcg, const PgDirectTap* tap = nullptr) {
    const int q = d.nq, n6 = a.N * 6;
    const size_t qq = (size_t)q * (size_t)q;
    d.refine = 0;
    if (q == 0) {
        if (!be.dgroup(kPgBand, a, d) || !be.dgrid(kPgZw, n6, a, d)) return false;
        ++*pcg;
        return pg_get(be, tap ? tap->x0 : nullptr, a.x, (size_t)n6);
    }
    if (!pg_phase_direct_factor(be, a, d)) return false;
    if (tap && (!pg_get(be, tap->Z, d.Z, (size_t)n6 * (size_t)q) || !pg_get(be, tap->Wm, d.Wm, qq) || !pg_get(be, tap->L, d.Lw, qq) || !pg_get(be, tap->Ks, d.Ks, qq) || !pg_get(be, tap->Lk, d.Lk, qq))) return false;
    if (!be.dgroup(kPgBand, a, d) || !be.dgroup(kPgCapSolve, a, d) || !be.dgrid(kPgZw, n6, a, d)) return false;
    ++*pcg;
    if (!pg_get(be, tap ? tap->x0 : nullptr, a.x, (size_t)n6)) return false;
    for (int it = 0; it < kPgDirectRefine; it++) {
        PgArgs b = a;
        b.p = a.x;                                  // q = H x through the kernel CG uses
        if (!be.grid(kPgHp, n6, b) || !be.dgrid(kPgResid, n6, a, d)) return false;
        d.refine = 1;
        if (!be.dgroup(kPgBand, a, d) || !be.dgroup(kPgCapSolve, a, d) || !be.dgrid(kPgZw, n6, a, d)) return false;
        d.refine = 0;
        ++*pcg;
    }
    return true;
}

// The statuses behind a direct solve from the scalars: the band's factor, Wm's, Ks's; returns the first that failed, or 0.
inline int pg_direct_status(const double h[kPgScalars], int st[3]) {
    const int d = (int)h[kScDirect];
    st[0] = (int)h[kScFactor]; st[1] = d % 4; st[2] = d / 4;
    return st[0] ? st[0] : (st[1] ? st[1] : st[2]);
}

// The run with the direct solve in place of conjugate gradients: pg_optimise's loop, accept rule and outputs.  `a` is bound by pg_bind, `d` by pg_bind_direct.
// o.max_pcg and o.pcg_tol are not used; pcg_iterations counts the single-right-hand-side band solves.
template <class Backend, class Policy>
inline bool pg_optimise_direct(Backend& be, PgArgs a, PgDirect d, const icet_pose_graph_options& o, icet_pose_graph_result* res, Policy& pol) {
    return pg_gauss_newton(be, a, o, [&](PgArgs& b, int* pcg, int* bad) {
        double h[kPgScalars]; int st[3], solves = 0;
        if (!pg_direct_solve(be, b, d, &solves) || !be.scalars(b, h)) return false;
        *bad = pg_direct_status(h, st);
        if (!*bad) *pcg += solves;          // (behind a failed factorisation the solves were launched but did nothing)
        return true;
    }, 1, res, pol);
}
template <class Backend>
inline bool pg_optimise_direct(Backend& be, PgArgs a, PgDirect d, const icet_pose_graph_options& o, icet_pose_graph_result* res) {
    PgPlainPolicy pol;
    return pg_optimise_direct(be, a, d, o, res, pol);
}

// ---- the robust run (icet_posegraph_robust.h) ----------------------------------------------------------------------------------------------------------------
// Its arrays beside the others in the same block: the weights and the raw sums of chi2, doubles only.  Bound only for a run with a kind.
template <class Alloc>
inline void pg_bind_robust(const PgArgs& a, PgRobust& r, Alloc& al) { r.wt = al.d((size_t)a.E); r.raw = al.d((size_t)kPgRobustRaw); }

// The arguments of a robust run from the caller's struct (null: kind 0); false for one the optimiser does not take (pg::robust_ok)
inline bool pg_robust_args(const icet_pose_graph_robust* rb, PgRobust* r) {
    *r = PgRobust{};
    if (!rb) return true;
    r->kind = rb->kind; r->flags = rb->flags; r->scale = rb->scale;
    return pg::robust_ok(rb->kind, rb->flags, rb->scale);
}

// The run under a robust kernel, through conjugate gradients or (direct; `d` bound by pg_bind_direct) the direct solve.  `r` has the kind, the caller's
// weight_out and, with a kind, pg_bind_robust's arrays.  With kind 0 the launches are pg_optimise's or pg_optimise_direct's, and kPgRobustFinish behind them
// where weights were asked for.  out->base has the RAW sums of chi2, cost_* the objective F.
template <class Backend>
inline bool pg_optimise_robust(Backend& be, const PgArgs& a, const PgDirect& d, bool direct, const icet_pose_graph_options& o, int c_offband, const PgRobust& r,
                               icet_pose_graph_robust_result* out) {
    icet_pose_graph_result res{};
    out->downweighted = 0; out->reserved = 0;
    if (r.kind == pg::kRobustNone) {
        if (!(direct ? pg_optimise_direct(be, a, d, o, &res) : pg_optimise(be, a, o, c_offband, &res))) return false;
        if (r.weight_out && !be.rgrid(kPgRobustFinish, a.E, a, r)) return false;
        out->base = res; out->cost_initial = res.chi2_initial; out->cost_final = res.chi2_final;
        return true;
    }
    PgRobustPolicy pol(r);
    if (!(direct ? pg_optimise_direct(be, a, d, o, &res, pol) : pg_optimise(be, a, o, c_offband, &res, pol))) return false;
    const bool failed = res.status == pg::kNotPositiveDefinite || res.status == pg::kNonFinite;
    double raw[kPgRobustRaw];
    std::vector<double> w((size_t)a.E);
    if (!be.fetch(raw, r.raw, sizeof(raw)) || (a.E > 0 && !be.fetch(w.data(), r.wt, sizeof(double) * (size_t)a.E))) return false;
    for (double v : w) if (v < 0.5) out->downweighted++;
    out->cost_initial = res.chi2_initial; out->cost_final = res.chi2_final;
    res.chi2_initial = raw[kPgRawStart]; res.chi2_final = failed ? raw[kPgRawStart] : raw[kPgRawFinal];
    out->base = res;
    return true;
}

// ---- the marginal covariances (icet_posegraph_marginals.h) ---------------------------------------------------------------------------------------------------
// Their work arrays beside pg_bind's and pg_bind_direct's in the same block, doubles only.  own_cov: the result is staged in the block (the host-pointer form
// and the hook); otherwise the caller points mg.cov at its own N x 36 doubles.
template <class Alloc>
inline void pg_bind_marg(const PgArgs& a, const PgDirect& d, PgMarg& mg, Alloc& al, bool own_cov) {
    const size_t N = (size_t)a.N, q = (size_t)d.nq;
    mg.Y = al.d(N * 36); mg.band_cov = al.d(N * 36);
    mg.Lt = al.d(q * q); mg.Lkt = al.d(q * q);
    mg.cov = own_cov ? al.d(N * 36) : nullptr;
}

// What the test hook copies out of a marginals run (null: nothing)
struct PgMargTap { double *D = nullptr, *B = nullptr, *A = nullptr, *band_cov = nullptr; };

// The marginal covariances of the poses the caller passed: one linearisation with no damping, the band's factor, with end nodes the direct solve's Z, L and Lk
// (its bodies, unchanged), then the selected inverse of the band and the closures' correction per node.  A fixed number of launches whatever the graph is,
// nothing read back but the scalars at the end.  kPgChi runs only so that the gradient kPgAssemble writes beside D is defined; the result does not depend on
// the measurements.  res->status: 0, or the first failed factorisation's status (kNotPositiveDefinite, kNonFinite) -- every free node's block is then NaN.
// assembled (the host test only, to run the device's own blocks): D, B, A, a zero g and zero scalars are in place, the run starts at the band's factor.
template <class Backend>
inline bool pg_marginals(Backend& be, PgArgs a, PgDirect d, PgMarg mg, icet_pose_graph_marginals_result* res, const PgMargTap* tap = nullptr, bool assembled = false) {
    double h[kPgScalars];
    const int N = a.N, C = a.C, q = d.nq;
    a.damping = 0.0; a.trial = 0; a.first = 0; a.failed = 0;
    // (no sum of the chi2 and no scalars read at the start: nothing here depends on them)
    if (!assembled && (!pg_phase_init(be, a) || !pg_phase_linearise(be, a))) return false;
    if (!be.group(kPgFactor, a)) return false;
    if (q > 0 && (!pg_phase_direct_factor(be, a, d) || !be.mgrid(kPgMargLt, q * q, a, d, mg))) return false;
    if (!be.mgrid(kPgSelinvPrep, N, a, d, mg) || !be.mgroups(kPgSelinv, 1, a, d, mg) || !be.mgroups(kPgMargNode, N, a, d, mg) || !be.scalars(a, h)) return false;
    int st[3];
    res->status = pg_direct_status(h, st);
    res->m = q / 6; res->factor_status = st[0]; res->wm_status = st[1]; res->ks_status = st[2]; res->reserved = 0;
    if (tap) {
        // (band_cov is written only behind a band that factored)
        if (!pg_get(be, tap->D, a.D, (size_t)N * 36) || !pg_get(be, tap->B, a.B, (size_t)N * 36) || !pg_get(be, tap->A, a.A, (size_t)C * 36) ||
            (st[0] == 0 && !pg_get(be, tap->band_cov, mg.band_cov, (size_t)N * 36))) return false;
    }
    return true;
}

// ---- the covariance columns and the gate (icet_posegraph_cross.h) -----------------------------------------------------------------------------------------
// Their work arrays beside the marginals' in the same block: the doubles, then the int32 list of the targets.  own_cols: the result is staged in the block (the
// host-pointer form); otherwise the caller points x.cols at its own T x N x 36 doubles.
struct PgCrossDev { int32_t* targets; };
template <class Alloc>
inline PgCrossDev pg_bind_cross(const PgArgs& a, const PgDirect& d, PgCross& x, Alloc& al, int T, bool own_cols) {
    const size_t N = (size_t)a.N, q = (size_t)d.nq, t = (size_t)T;
    x.T = T;
    x.Zt = al.d(N * 6 * 6 * t);
    x.Pt = al.d(t * 6 * q); x.Qt = al.d(t * 6 * q);
    x.cols = own_cols ? al.d(t * N * 36) : nullptr;
    PgCrossDev xd;
    xd.targets = al.i(t);
    x.targets = xd.targets;
    return xd;
}
// The gate's arrays: d2, S and the statuses where they are staged (own_out), the candidates' ends and target indices; the measurements are the caller's.
struct PgGateDev { int32_t *gi, *gj, *tcol; };
template <class Alloc>
inline PgGateDev pg_bind_gate(PgGate& g, Alloc& al, int n_cand, bool own_out, bool want_S) {
    const size_t n = (size_t)n_cand;
    g.n = n_cand;
    if (own_out) { g.d2 = al.d(n); g.S = want_S ? al.d(n * 36) : nullptr; }
    PgGateDev gd;
    gd.gi = al.i(n); gd.gj = al.i(n); gd.tcol = al.i(n);
    g.gi = gd.gi; g.gj = gd.gj; g.tcol = gd.tcol;
    if (own_out) g.status = al.i(n);
    return gd;
}

// The covariance columns of the poses the caller passed: pg_marginals as it is, then the band solves for the targets' 6 T unit columns (pg_z, the targets in
// the place of the end nodes), P_t and Q_t of the targets, and one workgroup per node for its T blocks.  A fixed number of launches whatever the graph is.
template <class Backend>
inline bool pg_columns(Backend& be, const PgArgs& a, const PgDirect& d, const PgMarg& mg, const PgCross& x, icet_pose_graph_marginals_result* res,
                       const PgMargTap* tap = nullptr, bool assembled = false) {
    if (!pg_marginals(be, a, d, mg, res, tap, assembled)) return false;
    PgDirect dz = d;          // Zt = M^-1 E_T: pg_z's columns are the targets'
    dz.nq = 6 * x.T; dz.ends = x.targets; dz.Z = x.Zt;
    const PgGate none{};
    return be.dgrid(kPgZ, 6 * x.T, a, dz) && be.xgroups(kPgCrossTarget, x.T, a, d, mg, x, none) && be.xgroups(kPgCrossNode, a.N, a, d, mg, x, none);
}

// (host) The gate's targets: the distinct live nodes gj of the candidates, ascending, and per candidate the index of its live node among them.  false: an end
// is out of range or a candidate's two ends are equal.
inline bool pg_gate_targets(int N, int n_cand, const int32_t* gi, const int32_t* gj, std::vector<int32_t>& targets, std::vector<int32_t>& tcol) {
    std::vector<int32_t> col((size_t)N, -1);
    for (int c = 0; c < n_cand; c++) {
        if (gi[c] < 0 || gi[c] >= N || gj[c] < 0 || gj[c] >= N || gi[c] == gj[c]) return false;
        col[(size_t)gj[c]] = 0;
    }
    targets.clear();
    for (int k = 0; k < N; k++) if (col[(size_t)k] == 0) { col[(size_t)k] = (int32_t)targets.size(); targets.push_back(k); }
    tcol.resize((size_t)n_cand);
    for (int c = 0; c < n_cand; c++) tcol[(size_t)c] = col[(size_t)gj[c]];
    return true;
}

// The covariance gate: pg_columns for the distinct live nodes of the candidates, then one workgroup per candidate.  rejected: the candidates whose d2 is not
// below the threshold (a NaN counts).
template <class Backend>
inline bool pg_gate(Backend& be, const PgArgs& a, const PgDirect& d, const PgMarg& mg, const PgCross& x, const PgGate& g, double threshold,
                    icet_pose_graph_gate_result* res) {
    if (!pg_columns(be, a, d, mg, x, &res->marg) || !be.xgroups(kPgGateCand, g.n, a, d, mg, x, g)) return false;
    std::vector<double> d2((size_t)g.n);
    if (!be.fetch(d2.data(), g.d2, sizeof(double) * (size_t)g.n)) return false;
    res->n_targets = x.T; res->rejected = 0;
    for (double v : d2) if (!(v < threshold)) res->rejected++;
    return true;
}

// The direct solve's test hook (icet_debug_pose_graph_direct; the host test runs it too): the optimiser's FIRST iteration with the direct solve, kernel for
// kernel, with its intermediate arrays copied out, then q = H p per caller vector.  Stops where the optimiser would: out->trial says whether the trial poses were taken.
template <class Backend>
inline bool pg_debug_direct_step(Backend& be, PgArgs a, PgDirect d, const icet_pose_graph_options& o, int K, const double* p, icet_pose_graph_direct_step* out) {
    double h[kPgScalars];
    const int N = a.N, E = a.E, C = a.C;
    const size_t n6 = (size_t)N * 6;
    a.damping = o.damping; a.trial = 0; a.first = 0; a.failed = 0;
    out->m = d.nq / 6; out->factor_status = 0; out->wm_status = 0; out->ks_status = 0; out->band_solves = 0; out->trial = 0;
    out->chi2_start = 0.0; out->chi2_trial = 0.0; out->max_dx = 0.0;
    if (out->ends && d.nq > 0 && !be.fetch(out->ends, d.ends, sizeof(int32_t) * (size_t)(d.nq / 6))) return false;
    if (!pg_phase_start(be, a, h)) return false;
    out->chi2_start = h[kScChi];
    if (!std::isfinite(h[kScChi])) { out->factor_status = pg::kNonFinite; return true; }
    if (!pg_phase_factor(be, a)) return false;
    if (!pg_get(be, out->D, a.D, (size_t)N * 36) || !pg_get(be, out->B, a.B, (size_t)N * 36) || !pg_get(be, out->A, a.A, (size_t)C * 36) || !pg_get(be, out->g, a.g, n6)) return false;
    PgDirectTap tap;
    tap.Z = out->Z; tap.Wm = out->Wm; tap.L = out->L; tap.Ks = out->Ks; tap.Lk = out->Lk; tap.x0 = out->x0;
    int pcg = 0, st[3];
    if (!pg_direct_solve(be, a, d, &pcg, &tap) || !be.scalars(a, h)) return false;
    const int bad = pg_direct_status(h, st);
    out->factor_status = st[0]; out->wm_status = st[1]; out->ks_status = st[2]; out->band_solves = pcg;
    if (!pg_get(be, out->x, a.x, n6)) return false;
    if (!bad) {
        if (!pg_phase_trial(be, a, h)) return false;
        out->trial = 1; out->chi2_trial = h[kScChi]; out->max_dx = h[kScMaxDx];
        if (!pg_get(be, out->Pt, a.Pt, (size_t)N * 12) || !pg_get(be, out->chi_trial, a.chit, (size_t)E)) return false;
    }
    return pg_phase_hp(be, a, K, p, out->q);
}

// The test hook's run (icet_debug_pose_graph_step; the host test runs it too): the optimiser's FIRST iteration, kernel for kernel -- the start's chi2, one
// linearisation, one linear solve through pg_cg, the trial poses and their chi2 -- with every intermediate array copied out, then q = H p per caller vector.
// The backend copies with fetch(host, device, bytes) and put(device, host, bytes), each false for a failure.  Where the optimiser would stop (a chi2 that is
// not finite, a failed solve) the hook stops: out->trial says whether the trial poses were taken.  out's null arrays are skipped.
template <class Backend>
inline bool pg_debug_step(Backend& be, PgArgs a, const icet_pose_graph_options& o, int c_offband, int K, const double* p, icet_pose_graph_step* out) {
    double h[kPgScalars];
    const int N = a.N, E = a.E, C = a.C;
    const size_t n6 = (size_t)N * 6;
    const double pcg_tol = o.pcg_tol > 0.0 ? o.pcg_tol : kPgDefaultPcgTol;
    a.damping = o.damping; a.trial = 0; a.first = 0; a.failed = 0;
    out->factor_status = 0; out->cg_status = 0; out->band_solves = 0; out->cg_end = kPgCgFailed; out->trial = 0;
    out->c_offband = c_offband; out->cap = pg_cg_cap(c_offband, o);
    out->chi2_start = 0.0; out->chi2_trial = 0.0; out->max_dx = 0.0;
    if (!pg_phase_start(be, a, h)) return false;
    out->chi2_start = h[kScChi];
    if (!pg_get(be, out->res, a.res, (size_t)E * 6) || !pg_get(be, out->chi_start, a.chi, (size_t)E)) return false;
    if (!std::isfinite(h[kScChi])) { out->cg_status = pg::kNonFinite; return true; }
    if (!pg_phase_factor(be, a)) return false;
    if (!pg_get(be, out->J, a.J, (size_t)E * 72) || !pg_get(be, out->D, a.D, (size_t)N * 36) || !pg_get(be, out->B, a.B, (size_t)N * 36) || !pg_get(be, out->A, a.A, (size_t)C * 36) ||
        !pg_get(be, out->g, a.g, n6)) return false;
    std::vector<double> rec(2 * (size_t)out->cap, std::nan(""));
    int pcg = 0, bad = 0, end = kPgCgCap;
    if (!pg_cg(be, a, out->cap, pcg_tol, &pcg, &bad, &end, rec.data())) return false;
    if (!be.scalars(a, h)) return false;
    out->factor_status = (int)h[kScFactor]; out->cg_status = bad; out->band_solves = pcg; out->cg_end = end;
    for (int i = 0; i < pcg && i < out->cg_capacity && out->cg_scalars; i++) { out->cg_scalars[2 * i] = rec[2 * i]; out->cg_scalars[2 * i + 1] = rec[2 * i + 1]; }
    if (!pg_get(be, out->x, a.x, n6)) return false;
    if (!bad) {
        if (!pg_phase_trial(be, a, h)) return false;
        out->trial = 1; out->chi2_trial = h[kScChi]; out->max_dx = h[kScMaxDx];
        if (h[kScCg] != 0.0) { out->cg_status = (int)h[kScCg]; out->cg_end = kPgCgFailed; }      // (the last step under the cap found p.Hp not positive)
        if (!pg_get(be, out->Pt, a.Pt, (size_t)N * 12) || !pg_get(be, out->chi_trial, a.chit, (size_t)E)) return false;
    }
    return pg_phase_hp(be, a, K, p, out->q);
}

}  // namespace icet
