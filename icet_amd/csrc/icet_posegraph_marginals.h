// icet_amd/csrc/icet_posegraph_marginals.h -- the kernel bodies of the pose graph's MARGINAL COVARIANCES (DESIGN.md section 20 "Marginal covariances"): block
// (k, k) of H^-1 for every node, in the optimiser's tangent (translation, rotation vector of the right update).  HIP-free, behind the macros of
// icet_posegraph_body.h: device code under hipcc, one host thread under a host compiler, four with a barrier under ICET_PG_EMU
// (tests/cpp/test_posegraph_marginals.cpp).  icet_posegraph.hip has the launches, icet_posegraph_driver.h (pg_marginals) the order they run in.
//
// H = M + U S U^T as in icet_posegraph_direct.h, with its Z = M^-1 U, Wm = L L^T and Ks = I + L^T S L = Lk Lk^T.  From L^T S L = Ks - I:
//     H^-1 = M^-1 - P P^T + Q Q^T,      P = Z L^-T,      Q = P Lk^-T
// so a node's block needs its six rows of Z, two forward substitutions per row and the node's block of M^-1.  Those come from the band's factor G, W (bt_factor;
// G keeps the reciprocals on its diagonal) by the backward recurrence
//     Sigma_{N-1} = T_{N-1},      Sigma_k = T_k + Y_k^T Sigma_{k+1} Y_k,      T_k = G_k^-T G_k^-1,      Y_k = W_{k+1} G_k^-1
// a sum of positive semi-definite terms.  A fixed node carries the identity in M and no coupling: the recurrence passes it by, and its block of the result is zero.
// No atomics, no block waits on another, every loop is bounded by N, q or 6, no per-thread array takes a run-time index (the 6 x 6 loops unroll), every output
// entry is one thread's sum in a fixed order, and every symmetric entry (r, c) is computed as (max, min): both triangles carry the same bits.
#pragma once
#include "icet_posegraph_direct.h"

namespace icet {

constexpr int kPgMargCols = 6 * kPgDirectMaxEnds;        // 768: a node's six rows of Z fit in LDS (36 KB)

// The marginals' own arrays (pg_bind_marg), beside PgArgs and PgDirect.
struct PgMarg {
    double *Y;                      // N x 36: Y_k = W_{k+1} G_k^-1 (zero for the last node)
    double *band_cov;               // N x 36: T_k behind kPgSelinvPrep, the diagonal blocks of M^-1 behind kPgSelinv
    double *Lt, *Lkt;               // nq x nq: L^T and Lk^T, so that a column of L is a contiguous row
    double *cov;                    // N x 36: the result
};

enum PgMargGridKernel { kPgSelinvPrep = 0, kPgMargLt };
enum PgMargGroupKernel { kPgSelinv = 0, kPgMargNode };

struct PgMargShared { double z[6 * kPgMargCols]; double pp[36]; };

ICET_PG_DEV double pg_quiet_nan() { return __builtin_nan(""); }

// k < N: T_k = G_k^-T G_k^-1 into band_cov and Y_k = W_{k+1} G_k^-1, by 6 x 6 triangular substitutions.  The nodes are independent.
ICET_PG_DEV void pg_selinv_prep(const PgArgs& a, const PgMarg& mg, int k) {
    if (a.sc[kScFactor] != 0.0) return;
    const double* Gk = a.G + (size_t)k * 36;
    double Gi[36];                  // G_k^-1: lower triangular, column c by forward substitution from the unit vector c
ICET_PG_UNROLL
    for (int c = 0; c < 6; c++) {
ICET_PG_UNROLL
        for (int i = 0; i < 6; i++) {
            double s = 0.0;
            if (i == c) s = Gk[c * 6 + c];
            if (i > c) {
ICET_PG_UNROLL
                for (int m = c; m < i; m++) s -= Gk[i * 6 + m] * Gi[m * 6 + c];
                s *= Gk[i * 6 + i];
            }
            Gi[i * 6 + c] = s;
        }
    }
    double* Tk = mg.band_cov + (size_t)k * 36;
    double* Yk = mg.Y + (size_t)k * 36;
    const bool last = k + 1 >= a.N;
    const double* Wn = a.W + (size_t)(last ? k : k + 1) * 36;
ICET_PG_UNROLL
    for (int r = 0; r < 6; r++) {
ICET_PG_UNROLL
        for (int c = 0; c < 6; c++) {
            const int rr = r > c ? r : c, cc = r > c ? c : r;
            double s = 0.0, y = 0.0;
ICET_PG_UNROLL
            for (int m = rr; m < 6; m++) s += Gi[m * 6 + rr] * Gi[m * 6 + cc];
ICET_PG_UNROLL
            for (int m = c; m < 6; m++) y += Wn[r * 6 + m] * Gi[m * 6 + c];
            Tk[r * 6 + c] = s;
            Yk[r * 6 + c] = last ? 0.0 : y;
        }
    }
}

// One workgroup: the backward recurrence over the nodes, the 36 entries of a block side by side, out of chunks of kPgChunk nodes staged through LDS as
// bt_solve stages its sweeps (sh.G: T, sh.W: Y, sh.D: the results, sh.v: Sigma_{k+1} Y_k, sh.prev: the block carried into the next chunk).
ICET_PG_DEV void pg_group_selinv(const PgArgs& a, const PgMarg& mg, PgShared& sh) {
    if (a.sc[kScFactor] != 0.0) return;
    const int t = ICET_PG_TID, N = a.N;
    const int last0 = ((N - 1) / kPgChunk) * kPgChunk;
    for (int k0 = last0; k0 >= 0; k0 -= kPgChunk) {
        const int nt = pg_min(kPgChunk, N - k0);
        ICET_PG_SYNC();
        for (int i = t; i < nt * 36; i += kPgThreads) { sh.G[i] = mg.band_cov[(size_t)k0 * 36 + i]; sh.W[i] = mg.Y[(size_t)k0 * 36 + i]; }
        ICET_PG_SYNC();
        for (int k = nt - 1; k >= 0; k--) {
            const bool tail = k0 + k == N - 1;          // (the same for every thread)
            const double* Sn = k == nt - 1 ? sh.prev : sh.D + (k + 1) * 36;
            const double* Yk = sh.W + k * 36;
            if (!tail)
                for (int e = t; e < 36; e += kPgThreads) {
                    const int r = e / 6, c = e % 6;
                    double s = 0.0;
                    for (int m = 0; m < 6; m++) s += Sn[r * 6 + m] * Yk[m * 6 + c];
                    sh.v[e] = s;
                }
            ICET_PG_SYNC();
            for (int e = t; e < 36; e += kPgThreads) {
                const int r = e / 6, c = e % 6;
                const int rr = r > c ? r : c, cc = r > c ? c : r;
                double s = sh.G[k * 36 + rr * 6 + cc];
                if (!tail) {
                    double u = 0.0;
                    for (int m = 0; m < 6; m++) u += Yk[m * 6 + rr] * sh.v[m * 6 + cc];
                    s += u;
                }
                sh.D[k * 36 + e] = s;
            }
            ICET_PG_SYNC();
        }
        for (int i = t; i < 36; i += kPgThreads) sh.prev[i] = sh.D[i];
        for (int i = t; i < nt * 36; i += kPgThreads) mg.band_cov[(size_t)k0 * 36 + i] = sh.D[i];
    }
    ICET_PG_SYNC();
}

// gi < q x q: the transposes of L and Lk
ICET_PG_DEV void pg_marg_lt(const PgArgs& a, const PgDirect& d, const PgMarg& mg, int gi) {
    if (pg_direct_failed(a)) return;
    const int q = d.nq, r = gi / q, c = gi % q;
    mg.Lt[gi] = d.Lw[(size_t)c * q + r];
    mg.Lkt[gi] = d.Lk[(size_t)c * q + r];
}

// The six rows z (LDS, [row][q]) times T^-T for a lower-triangular T given as Tt = T^T with the reciprocal diagonal rd: T x = z per row, column-oriented as
// pg_group_cap_solve's -- every entry's updates arrive in ascending column order, one barrier per column, then the division.
ICET_PG_DEV void pg_marg_forward(int q, const double* Tt, const double* rd, double* z) {
    const int t = ICET_PG_TID;
    for (int j = 0; j < q; j++) {
        const double rj = rd[j];
        const double* Tj = Tt + (size_t)j * q;
        const double x0 = z[j] * rj, x1 = z[q + j] * rj, x2 = z[2 * q + j] * rj, x3 = z[3 * q + j] * rj, x4 = z[4 * q + j] * rj, x5 = z[5 * q + j] * rj;
        for (int i = j + 1 + t; i < q; i += kPgThreads) {
            const double l = Tj[i];
            z[i] -= l * x0; z[q + i] -= l * x1; z[2 * q + i] -= l * x2; z[3 * q + i] -= l * x3; z[4 * q + i] -= l * x4; z[5 * q + i] -= l * x5;
        }
        ICET_PG_SYNC();
    }
    for (int i = t; i < 6 * q; i += kPgThreads) z[i] *= rd[i % q];
    ICET_PG_SYNC();
}

// entry e = (r, c) of z z^T at (max, min), over the columns in ascending order
ICET_PG_DEV double pg_marg_gram(int q, const double* z, int e) {
    const int r = e / 6, c = e % 6;
    const double* zr = z + (size_t)(r > c ? r : c) * q; const double* zc = z + (size_t)(r > c ? c : r) * q;
    double s = 0.0;
    for (int j = 0; j < q; j++) s += zr[j] * zc[j];
    return s;
}

// One workgroup per node k: Sigma_k = band_cov_k - P_k P_k^T + Q_k Q_k^T.  The node's six rows of Z sit in LDS and become P_k, then Q_k, in place.  With q = 0
// the result is band_cov_k.  A fixed node's block is zero; behind a failed factorisation every free node's block is quiet NaN.
ICET_PG_DEV void pg_group_marg(const PgArgs& a, const PgDirect& d, const PgMarg& mg, int k, PgMargShared& sh) {
    const int t = ICET_PG_TID, q = d.nq;
    double* out = mg.cov + (size_t)k * 36;
    if (pg_fixed(a, k) || pg_direct_failed(a)) {          // (the same for every thread)
        const double v = pg_fixed(a, k) ? 0.0 : pg_quiet_nan();
        for (int e = t; e < 36; e += kPgThreads) out[e] = v;
        return;
    }
    const double* band = mg.band_cov + (size_t)k * 36;
    if (q == 0) {
        for (int e = t; e < 36; e += kPgThreads) out[e] = band[e];
        return;
    }
    const double* Zk = d.Z + (size_t)k * 6 * (size_t)q;
    for (int i = t; i < 6 * q; i += kPgThreads) sh.z[i] = Zk[i];
    ICET_PG_SYNC();
    pg_marg_forward(q, mg.Lt, d.rdw, sh.z);
    for (int e = t; e < 36; e += kPgThreads) sh.pp[e] = pg_marg_gram(q, sh.z, e);
    ICET_PG_SYNC();
    pg_marg_forward(q, mg.Lkt, d.rdk, sh.z);
    for (int e = t; e < 36; e += kPgThreads) out[e] = (band[e] - sh.pp[e]) + pg_marg_gram(q, sh.z, e);
    ICET_PG_SYNC();
}

}  // namespace icet
