// icet_amd/csrc/icet_posegraph_driver.h -- the pose-graph optimiser's driver, written ONCE: the Gauss-Newton loop, the preconditioned
// conjugate gradients, the accept rule and what a failure returns.  HIP-free.  It runs the bodies of icet_posegraph_body.h through a BACKEND that launches a
// kernel (or loops over its index range on the host) and reads the few scalars back:
//     bool grid(PgGridKernel, int count, const PgArgs&)      the body for every global index below count (count 0: nothing)
//     bool group(PgGroupKernel, const PgArgs&)               the body as one workgroup
//     bool scalars(const PgArgs&, double out[kPgScalars])    wait for what was enqueued, then a.sc on the host
//     bool fetch(void* host, const void* dev, size_t bytes), put(void* dev, const void* host, size_t bytes)      (the test hook only) copies, complete on return
// each false for a failure of the backend (the driver then returns false at once).  icet_posegraph.hip has the device's backend,
// tests/cpp/test_posegraph_optimize.cpp the host's.
#pragma once
#include "icet_posegraph_body.h"

#include <cmath>
#include <vector>

namespace icet {

constexpr double kPgDefaultPcgTol = 1e-10;

inline icet_pose_graph_options pg_default_options() { icet_pose_graph_options o; o.gn_iters = 10; o.max_pcg = 0; o.dx_tol = 1e-7; o.damping = 0.0; o.pcg_tol = kPgDefaultPcgTol; return o; }

// The graph on the host: the edges' ends, the incidence lists, the count of closures that lie off the band between two free nodes.
struct PgGraph {
    std::vector<int32_t> ei, ej, off, items;
    int c_offband = 0;
    void build(int N, int C, const int32_t* ci, const int32_t* cj, const uint8_t* fixed) {
        pg::build_incidence(N, C, ci, cj, fixed, ei, ej, off, items);
        c_offband = 0;
        for (int c = 0; c < C; c++) {
            const int i = ci[c], j = cj[c];
            if ((i - j >= 2 || j - i >= 2) && off[i + 1] != off[i] && off[j + 1] != off[j]) c_offband++;
        }
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

// The run.  `a` is bound (pg_bind), the graph uploaded, the caller's arrays in place.  true: *res is the result (its status says how the run ended).
template <class Backend>
inline bool pg_optimise(Backend& be, PgArgs a, const icet_pose_graph_options& o, int c_offband, icet_pose_graph_result* res) {
    double h[kPgScalars];
    const int N = a.N, E = a.E, C = a.C;
    const double pcg_tol = o.pcg_tol > 0.0 ? o.pcg_tol : kPgDefaultPcgTol;
    const int n_init = N * 12 > E * 36 ? N * 12 : E * 36;
    a.damping = o.damping; a.trial = 0; a.first = 0; a.failed = 0;
    if (!be.grid(kPgInit, n_init, a) || !be.grid(kPgChi, E, a) || !be.group(kPgStats, a) || !be.scalars(a, h)) return false;
    const double chi2_initial = h[kScChi];
    double chi2 = chi2_initial, max_dx = 0.0;
    int status = pg::kIterationCap, its = 0, pcg = 0;
    bool failed = false;
    if (!std::isfinite(chi2)) { status = pg::kNonFinite; failed = true; }
    for (int it = 0; it < o.gn_iters && !failed; it++) {
        its++;
        if (!be.grid(kPgLinearise, E * 12, a) || !be.grid(kPgAssemble, N * 36, a) || !be.grid(kPgOffband, C * 36, a) || !be.group(kPgFactor, a)) return false;
        int bad = 0;
        if (!pg_cg(be, a, pg_cg_cap(c_offband, o), pcg_tol, &pcg, &bad)) return false;
        if (bad) { status = bad; failed = true; break; }
        a.trial = 1;
        if (!be.grid(kPgRetract, N, a) || !be.grid(kPgChi, E, a) || !be.group(kPgStats, a) || !be.scalars(a, h)) return false;
        a.trial = 0;
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
    if (!be.grid(kPgFinish, n_fin, a) || !be.scalars(a, h)) return false;
    res->chi2_initial = chi2_initial; res->chi2_final = failed ? chi2_initial : chi2; res->max_dx = max_dx;
    res->status = status; res->gn_iterations = its; res->pcg_iterations = pcg; res->reserved = 0;
    return true;
}

// The test hook's run (icet_debug_pose_graph_step; the host test runs it too): the optimiser's FIRST iteration, kernel for kernel -- the start's chi2, one
// linearisation, one linear solve through pg_cg, the trial poses and their chi2 -- with every intermediate array copied out, then q = H p per caller vector.
// The backend copies with fetch(host, device, bytes) and put(device, host, bytes), each false for a failure.  Where the optimiser would stop (a chi2 that is
// not finite, a failed solve) the hook stops: out->trial says whether the trial poses were taken.  out's null arrays are skipped.
template <class Backend>
inline bool pg_debug_step(Backend& be, PgArgs a, const icet_pose_graph_options& o, int c_offband, int K, const double* p, icet_pose_graph_step* out) {
    double h[kPgScalars];
    const int N = a.N, E = a.E, C = a.C;
    const size_t sd = sizeof(double), n6 = (size_t)N * 6;
    const double pcg_tol = o.pcg_tol > 0.0 ? o.pcg_tol : kPgDefaultPcgTol;
    const int n_init = N * 12 > E * 36 ? N * 12 : E * 36;
    auto get = [&](double* dst, const double* src, size_t count) { return !dst || count == 0 || be.fetch(dst, src, count * sd); };
    a.damping = o.damping; a.trial = 0; a.first = 0; a.failed = 0;
    out->factor_status = 0; out->cg_status = 0; out->band_solves = 0; out->cg_end = kPgCgFailed; out->trial = 0;
    out->c_offband = c_offband; out->cap = pg_cg_cap(c_offband, o);
    out->chi2_start = 0.0; out->chi2_trial = 0.0; out->max_dx = 0.0;
    if (!be.grid(kPgInit, n_init, a) || !be.grid(kPgChi, E, a) || !be.group(kPgStats, a) || !be.scalars(a, h)) return false;
    out->chi2_start = h[kScChi];
    if (!get(out->res, a.res, (size_t)E * 6) || !get(out->chi_start, a.chi, (size_t)E)) return false;
    if (!std::isfinite(h[kScChi])) { out->cg_status = pg::kNonFinite; return true; }
    if (!be.grid(kPgLinearise, E * 12, a) || !be.grid(kPgAssemble, N * 36, a) || !be.grid(kPgOffband, C * 36, a) || !be.group(kPgFactor, a)) return false;
    if (!get(out->J, a.J, (size_t)E * 72) || !get(out->D, a.D, (size_t)N * 36) || !get(out->B, a.B, (size_t)N * 36) || !get(out->A, a.A, (size_t)C * 36) ||
        !get(out->g, a.g, n6)) return false;
    std::vector<double> rec(2 * (size_t)out->cap, std::nan(""));
    int pcg = 0, bad = 0, end = kPgCgCap;
    if (!pg_cg(be, a, out->cap, pcg_tol, &pcg, &bad, &end, rec.data())) return false;
    if (!be.scalars(a, h)) return false;
    out->factor_status = (int)h[kScFactor]; out->cg_status = bad; out->band_solves = pcg; out->cg_end = end;
    for (int i = 0; i < pcg && i < out->cg_capacity && out->cg_scalars; i++) { out->cg_scalars[2 * i] = rec[2 * i]; out->cg_scalars[2 * i + 1] = rec[2 * i + 1]; }
    if (!get(out->x, a.x, n6)) return false;
    if (!bad) {
        a.trial = 1;
        if (!be.grid(kPgRetract, N, a) || !be.grid(kPgChi, E, a) || !be.group(kPgStats, a) || !be.scalars(a, h)) return false;
        a.trial = 0;
        out->trial = 1; out->chi2_trial = h[kScChi]; out->max_dx = h[kScMaxDx];
        if (h[kScCg] != 0.0) { out->cg_status = (int)h[kScCg]; out->cg_end = kPgCgFailed; }      // (the last step under the cap found p.Hp not positive)
        if (!get(out->Pt, a.Pt, (size_t)N * 12) || !get(out->chi_trial, a.chit, (size_t)E)) return false;
    }
    for (int k = 0; k < K && out->q; k++)
        if (!be.put(a.p, p + (size_t)k * n6, n6 * sd) || !be.grid(kPgHp, N * 6, a) || !be.fetch(out->q + (size_t)k * n6, a.q, n6 * sd)) return false;
    return true;
}

}  // namespace icet
