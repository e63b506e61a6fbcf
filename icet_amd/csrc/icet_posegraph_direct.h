// icet_amd/csrc/icet_posegraph_direct.h -- the kernel bodies of the pose-graph optimiser's DIRECT solve (DESIGN.md section 20 "The direct solve").  HIP-free, behind
// the macros of icet_posegraph_body.h: device code under hipcc, one host thread under a host compiler, four with a barrier under ICET_PG_EMU
// (tests/cpp/test_posegraph_direct.cpp).  icet_posegraph.hip has the launches, icet_posegraph_driver.h (pg_direct_solve) the order they run in.
//
// H = M + R, M the block-tridiagonal band (factor G, W of bt_factor), R = U S U^T the closures off the band: U selects the 6 components of the m END nodes
// (d.ends, ascending; d.end_of[node] = its index or -1), q = 6 m, S = U^T R U (q x q, never stored: its products walk the end nodes' incidence lists).
//     Z = M^-1 U (6N x q, [row][col])      Wm = U^T Z = L L^T      Ks = I + L^T S L = Lk Lk^T
//     apply(b): y = M^-1 b, v = U^T y, t = L^T S v, Lk Lk^T u = t, L^T w = u, result y - Z w
// (M + U S U^T)^-1 = M^-1 - M^-1 U (I + S Wm)^-1 S U^T M^-1 and (I + S L L^T)^-1 = L^-T (I + L^T S L)^-1 L^T.  Ks is congruent to M^-1/2 H M^-1/2 on the closures'
// subspace: with M positive definite, H is positive definite exactly when Ks is.
// L and Lk are stored whole (q x q row-major, zeros above the diagonal, the TRUE diagonal: the products L^T S L read it) with the reciprocals of their diagonals
// beside them (d.rdw, d.rdk: what the substitutions multiply by).  No atomics, no block waits on another, every loop is bounded by N, q or an incidence count, no
// per-thread array takes a run-time index.
#pragma once
#include "icet_posegraph_body.h"

namespace icet {

using pg::kPgDirectMaxEnds;                // 128 (icet_posegraph.h): q <= 768, one workgroup factors Wm and Ks
constexpr int kPgDirectRefine = 1;         // steps of iterative refinement behind the first apply
// sc[kScDirect]: the status of the factorisation of Wm + 4 x that of Ks (each 0, kNotPositiveDefinite or kNonFinite)
constexpr int kScDirect = 7;

// The direct solve's own arrays (pg_bind_direct), beside PgArgs: m end nodes, nq = 6 m.
struct PgDirect {
    int nq;
    int refine;                     // kPgZw: 0 = x is y - Z w, 1 = it is added to x
    const int32_t *ends, *end_of;   // m: the end nodes, ascending | N: a node's index in ends, or -1
    double *Z;                      // 6N x nq: M^-1 U
    double *Wm, *Lw, *SL, *Ks, *Lk; // nq x nq
    double *rdw, *rdk;              // nq: the reciprocal diagonals of Lw, Lk
    double *cv, *ct, *cu, *cw;      // nq: the capacitance solve's vectors, cw its result
    double *y;                      // N x 6: a band solve's result
};

enum PgDirectGridKernel { kPgZ = 0, kPgWm, kPgSl, kPgKs, kPgZw, kPgResid };
enum PgDirectGroupKernel { kPgCholW = 0, kPgCholK, kPgBand, kPgCapSolve };

// true when an earlier kernel of this iteration has failed: everything behind it leaves its outputs alone (the same for every thread)
ICET_PG_DEV bool pg_direct_failed(const PgArgs& a) { return a.sc[kScFactor] != 0.0 || a.sc[kScDirect] != 0.0; }

// col < q: column col of Z = M^-1 U, one thread per column.  The right-hand side is component col % 6 of node ends[col / 6] and zero elsewhere, so the forward
// sweep has nothing to do before that node (its result there is zero); from there on bt_solve's recurrences, the same arithmetic per column.  Every thread
// walks k = 0 .. N - 1 together, so G_k and W_k are read at one address per wave.  The forward result is held in Z and overwritten by the backward sweep.
ICET_PG_DEV void pg_z(const PgArgs& a, const PgDirect& d, int col) {
    if (a.sc[kScFactor] != 0.0) return;
    const int N = a.N, s = d.ends[col / 6], comp = col % 6;
    const size_t q = (size_t)d.nq;
    const double* G = a.G; const double* W = a.W;
    double* Z = d.Z + col;
    double carry[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < N; k++) {
        const double* Gk = G + (size_t)k * 36; const double* Wk = W + (size_t)k * 36;
        double v[6];
        if (k < s) {
ICET_PG_UNROLL
            for (int c = 0; c < 6; c++) Z[((size_t)k * 6 + c) * q] = 0.0;
            continue;
        }
ICET_PG_UNROLL
        for (int c = 0; c < 6; c++) {
            double t = (k == s && c == comp) ? 1.0 : 0.0;
ICET_PG_UNROLL
            for (int e = 0; e < 6; e++) t -= Wk[c * 6 + e] * carry[e];
            v[c] = t;
        }
ICET_PG_UNROLL
        for (int c = 0; c < 6; c++) {
            double t = v[c];
ICET_PG_UNROLL
            for (int e = 0; e < c; e++) t -= Gk[c * 6 + e] * v[e];
            v[c] = t * Gk[c * 6 + c];
        }
ICET_PG_UNROLL
        for (int c = 0; c < 6; c++) { carry[c] = v[c]; Z[((size_t)k * 6 + c) * q] = v[c]; }
    }
ICET_PG_UNROLL
    for (int c = 0; c < 6; c++) carry[c] = 0.0;
    for (int k = N - 1; k >= 0; k--) {
        const double* Gk = G + (size_t)k * 36;
        double v[6];
        if (k + 1 < N) {
            const double* Wn = W + (size_t)(k + 1) * 36;         // W of the NEXT node; nothing behind the last
ICET_PG_UNROLL
            for (int c = 0; c < 6; c++) {
                double t = Z[((size_t)k * 6 + c) * q];
ICET_PG_UNROLL
                for (int e = 0; e < 6; e++) t -= Wn[e * 6 + c] * carry[e];
                v[c] = t;
            }
        } else {
ICET_PG_UNROLL
            for (int c = 0; c < 6; c++) v[c] = Z[((size_t)k * 6 + c) * q];
        }
        // (fully unrolled by hand where the bound counts down: no run-time index into v)
        v[5] = v[5] * Gk[35];
        v[4] = (v[4] - Gk[5 * 6 + 4] * v[5]) * Gk[28];
        v[3] = ((v[3] - Gk[4 * 6 + 3] * v[4]) - Gk[5 * 6 + 3] * v[5]) * Gk[21];
        v[2] = (((v[2] - Gk[3 * 6 + 2] * v[3]) - Gk[4 * 6 + 2] * v[4]) - Gk[5 * 6 + 2] * v[5]) * Gk[14];
        v[1] = ((((v[1] - Gk[2 * 6 + 1] * v[2]) - Gk[3 * 6 + 1] * v[3]) - Gk[4 * 6 + 1] * v[4]) - Gk[5 * 6 + 1] * v[5]) * Gk[7];
        v[0] = (((((v[0] - Gk[1 * 6 + 0] * v[1]) - Gk[2 * 6 + 0] * v[2]) - Gk[3 * 6 + 0] * v[3]) - Gk[4 * 6 + 0] * v[4]) - Gk[5 * 6 + 0] * v[5]) * Gk[0];
ICET_PG_UNROLL
        for (int c = 0; c < 6; c++) { carry[c] = v[c]; Z[((size_t)k * 6 + c) * q] = v[c]; }
    }
}

// gi < q x q: Wm = U^T Z, entry (r, c) read at (max, min): both triangles carry the same bits
ICET_PG_DEV void pg_wm(const PgArgs& a, const PgDirect& d, int gi) {
    if (a.sc[kScFactor] != 0.0) return;
    const int q = d.nq, r = gi / q, c = gi % q;
    const int rr = r > c ? r : c, cc = r > c ? c : r;
    d.Wm[gi] = d.Z[((size_t)d.ends[rr / 6] * 6 + rr % 6) * (size_t)q + cc];
}

// One workgroup: src = L L^T (n x n, symmetric; only its lower triangle is read), left-looking by columns out of global memory.  Entry (i, j) is ONE thread's
// dot product over m < j in ascending order, so the bits do not depend on the thread count.  L keeps its true diagonal, rd its reciprocals.  A pivot at or below
// kPivotRel x its diagonal entry of src ends the factorisation: kNotPositiveDefinite (kNonFinite for a pivot that is not finite); returns the status (the same in
// every thread).
ICET_PG_DEV int pg_chol(int n, const double* src, double* L, double* rd) {
    const int t = ICET_PG_TID;
    for (int i = t; i < n; i += kPgThreads)
        for (int j = i + 1; j < n; j++) L[(size_t)i * n + j] = 0.0;
    for (int j = 0; j < n; j++) {
        for (int i = j + t; i < n; i += kPgThreads) {
            const double* Li = L + (size_t)i * n; const double* Lj = L + (size_t)j * n;
            double s = src[(size_t)i * n + j];
            for (int m = 0; m < j; m++) s -= Li[m] * Lj[m];
            L[(size_t)i * n + j] = s;
        }
        ICET_PG_SYNC();
        const double d = L[(size_t)j * n + j];
        ICET_PG_SYNC();
        if (d != d || fabs(d) > 1.7e308) return pg::kNonFinite;
        if (!(d > pg::kPivotRel * fabs(src[(size_t)j * n + j]))) return pg::kNotPositiveDefinite;
        const double root = sqrt(d), inv = 1.0 / root;
        for (int i = j + t; i < n; i += kPgThreads) {
            if (i == j) { L[(size_t)j * n + j] = root; rd[j] = inv; }
            else L[(size_t)i * n + j] *= inv;
        }
        ICET_PG_SYNC();
    }
    return 0;
}

// Wm = L L^T (which = 0) or Ks = Lk Lk^T (which = 1); the status goes to sc[kScDirect]
ICET_PG_DEV void pg_group_chol(const PgArgs& a, const PgDirect& d, int which) {
    if (pg_direct_failed(a)) return;
    const int st = which == 0 ? pg_chol(d.nq, d.Wm, d.Lw, d.rdw) : pg_chol(d.nq, d.Ks, d.Lk, d.rdk);
    ICET_PG_SYNC();
    if (ICET_PG_TID == 0 && st != 0) a.sc[kScDirect] = (double)(which == 0 ? st : 4 * st);
    ICET_PG_SYNC();
}

// Row r of S times the end-indexed vector p (entry e at p[e x stride]): the off-band closures of node ends[r / 6] in the order of its incidence list, as pg_hp
// walks them.  A is zero for a closure with a fixed end, and such an end has no index: it is skipped.
ICET_PG_DEV double pg_s_row(const PgArgs& a, const PgDirect& d, int r, const double* p, size_t stride) {
    const int k = d.ends[r / 6], rc = r % 6;
    double s = 0.0;
    for (int it = a.off[k]; it < a.off[k + 1]; it++) {
        const int item = a.items[it], e = item >> 1, side = item & 1;
        if (e < a.N - 1) continue;
        const int other = side ? a.ei[e] : a.ej[e];
        if (other - k < 2 && k - other < 2) continue;
        const int b = d.end_of[other];
        if (b < 0) continue;
        const double* Ac = a.A + (size_t)(e - (a.N - 1)) * 36;
        const double* pb = p + (size_t)b * 6 * stride;
        if (side == 0) for (int c = 0; c < 6; c++) s += Ac[rc * 6 + c] * pb[(size_t)c * stride];
        else           for (int c = 0; c < 6; c++) s += Ac[c * 6 + rc] * pb[(size_t)c * stride];
    }
    return s;
}

// gi < q x q: SL = S L
ICET_PG_DEV void pg_sl(const PgArgs& a, const PgDirect& d, int gi) {
    if (pg_direct_failed(a)) return;
    const int q = d.nq, r = gi / q, c = gi % q;
    d.SL[gi] = pg_s_row(a, d, r, d.Lw + c, (size_t)q);
}

// gi < q x q: Ks = I + L^T (S L), entry (r, c) computed at (max, min): a dot product over m in ascending order (L is zero above its diagonal: m starts at max)
ICET_PG_DEV void pg_ks(const PgArgs& a, const PgDirect& d, int gi) {
    if (pg_direct_failed(a)) return;
    const int q = d.nq, r = gi / q, c = gi % q;
    const int rr = r > c ? r : c, cc = r > c ? c : r;
    double s = 0.0;
    for (int m = rr; m < q; m++) s += d.Lw[(size_t)m * q + rr] * d.SL[(size_t)m * q + cc];
    d.Ks[gi] = rr == cc ? 1.0 + s : s;
}

// the band solve alone: y = M^-1 r through the factor
ICET_PG_DEV void pg_group_band(const PgArgs& a, const PgDirect& d, PgShared& sh) {
    if (pg_direct_failed(a)) return;
    bt_solve(a.N, a.G, a.W, a.r, d.y, a.u, &sh);
}

// b <- T^-T b for a lower-triangular T (q x q, reciprocal diagonal rd), column-oriented: entry j is final once the columns behind it have been taken off
ICET_PG_DEV void pg_back_subst(int q, const double* T, const double* rd, double* b, double* x) {
    const int t = ICET_PG_TID;
    for (int j = q - 1; j >= 0; j--) {
        const double xj = b[j] * rd[j];
        const double* Tj = T + (size_t)j * q;
        for (int i = t; i < j; i += kPgThreads) b[i] -= Tj[i] * xj;
        if (t == 0) x[j] = xj;
        ICET_PG_SYNC();
    }
}

// One workgroup, from y: v = U^T y, t = L^T S v, Lk Lk^T u = t, L^T w = u.  cv, ct, cu: q doubles of scratch each; cw: the result.
ICET_PG_DEV void pg_group_cap_solve(const PgArgs& a, const PgDirect& d) {
    if (pg_direct_failed(a)) return;
    const int t = ICET_PG_TID, q = d.nq;
    for (int r = t; r < q; r += kPgThreads) d.cv[r] = d.y[(size_t)d.ends[r / 6] * 6 + r % 6];
    ICET_PG_SYNC();
    for (int r = t; r < q; r += kPgThreads) d.cu[r] = pg_s_row(a, d, r, d.cv, 1);
    ICET_PG_SYNC();
    for (int c = t; c < q; c += kPgThreads) {
        double s = 0.0;
        for (int m = c; m < q; m++) s += d.Lw[(size_t)m * q + c] * d.cu[m];
        d.ct[c] = s;
    }
    ICET_PG_SYNC();
    // Lk u' = t, column-oriented: every entry's updates arrive in ascending column order
    for (int j = 0; j < q; j++) {
        const double uj = d.ct[j] * d.rdk[j];
        for (int i = j + 1 + t; i < q; i += kPgThreads) d.ct[i] -= d.Lk[(size_t)i * q + j] * uj;
        if (t == 0) d.cu[j] = uj;
        ICET_PG_SYNC();
    }
    pg_back_subst(q, d.Lk, d.rdk, d.cu, d.cv);
    pg_back_subst(q, d.Lw, d.rdw, d.cv, d.cw);
}

// gi < 6N: x = y - Z w (d.refine = 0) or x += y - Z w, one thread per row over the columns in ascending order
ICET_PG_DEV void pg_zw(const PgArgs& a, const PgDirect& d, int gi) {
    if (pg_direct_failed(a)) return;
    const double* Zr = d.Z + (size_t)gi * (size_t)d.nq;
    double s = d.y[gi];
    for (int c = 0; c < d.nq; c++) s -= Zr[c] * d.cw[c];
    a.x[gi] = d.refine ? a.x[gi] + s : s;
}

// gi < 6N: the residual of the solve, r = -g - q behind q = H x
ICET_PG_DEV void pg_resid(const PgArgs& a, const PgDirect& d, int gi) {
    if (pg_direct_failed(a)) return;
    a.r[gi] = -a.g[gi] - a.q[gi];
}

}  // namespace icet
