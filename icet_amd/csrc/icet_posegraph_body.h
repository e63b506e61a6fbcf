// icet_amd/csrc/icet_posegraph_body.h -- the kernel bodies of the pose-graph optimiser: the block-tridiagonal solve as one workgroup runs
// it, then the optimiser's grid and workgroup bodies (icet_posegraph.hip has the launches and the host entry points, icet_posegraph_driver.h the loop that runs them).
// Under hipcc this is device code for 256 threads.  Under a host compiler the same text runs as a "workgroup" of ONE thread (every strided
// loop then covers its whole range, the barriers are empty): tests/cpp/test_posegraph.cpp and tests/cpp/test_posegraph_optimize.cpp run it that way, under the
// address sanitizer too; the latter also as ICET_PG_EMU: four host threads with a real barrier.
#pragma once
#include "../../include/icet_hip.h"
#include "icet_posegraph.h"

#if defined(ICET_PG_EMU)
// (a test defines the four macros and ICET_PG_EMU_THREADS itself: host threads with a real barrier)
#elif defined(__HIPCC__)
#define ICET_PG_DEV __device__ static inline
#define ICET_PG_TID ((int)threadIdx.x)
#define ICET_PG_SYNC() __syncthreads()
#define ICET_PG_UNROLL _Pragma("unroll")
#else
#define ICET_PG_UNROLL
#define ICET_PG_DEV static inline
#define ICET_PG_TID 0
#define ICET_PG_SYNC() ((void)0)
#endif

namespace icet {
namespace pg = icet_pg_rule;

#if defined(ICET_PG_EMU)
constexpr int kPgThreads = ICET_PG_EMU_THREADS;
#elif defined(__HIPCC__)
constexpr int kPgThreads = 256;
#else
constexpr int kPgThreads = 1;
#endif
constexpr int kPgChunk = 32;          // nodes per staged chunk of the band sweeps
ICET_PG_HD static inline int pg_min(int a, int b) { return a < b ? a : b; }

struct PgShared {
    double G[kPgChunk * 36], W[kPgChunk * 36], D[kPgChunk * 36], B[kPgChunk * 36];
    double v[kPgChunk * 6];
    double prev[36];
    int status;
};

// ---- the block-tridiagonal factor and solve ---------------------------------------------------------------------------------------------------------------
// M = [D_k on the diagonal, B_k at (k, k - 1), B_k^T at (k - 1, k)], symmetric positive definite.  Block Cholesky M = L L^T: diagonal blocks G_k (lower
// triangular), sub-diagonal blocks W_k = B_k G_{k-1}^{-T}, G_k G_k^T = D_k - W_k W_k^T.  G is stored with the RECIPROCALS of its diagonal on the diagonal and
// zeros above.  A pivot that is not above kPivotRel x its diagonal entry of D ends the factorisation: sh->status = kNotPositiveDefinite (kNonFinite for a NaN).
ICET_PG_DEV void bt_factor(int N, const double* Dm, const double* Bm, double* G, double* W, PgShared* sh) {
    const int t = ICET_PG_TID;
    if (t < 36) sh->prev[t] = (t % 7 == 0) ? 1.0 : 0.0;
    for (int k0 = 0; k0 < N; k0 += kPgChunk) {
        const int nt = pg_min(kPgChunk, N - k0);
        ICET_PG_SYNC();
        for (int i = t; i < nt * 36; i += kPgThreads) { sh->D[i] = Dm[(size_t)k0 * 36 + i]; sh->B[i] = Bm[(size_t)k0 * 36 + i]; sh->G[i] = 0.0; sh->W[i] = 0.0; }
        ICET_PG_SYNC();
        if (t == 0 && sh->status == 0) {
            for (int k = 0; k < nt && sh->status == 0; k++) {
                const double* Gp = k == 0 ? sh->prev : sh->G + (k - 1) * 36;
                const double* Dk = sh->D + k * 36; const double* Bk = sh->B + k * 36;
                double* Gk = sh->G + k * 36; double* Wk = sh->W + k * 36;
                for (int r = 0; r < 6; r++)                       // row r of W: G_prev y = (row r of B)^T
                    for (int c = 0; c < 6; c++) {
                        double s = Bk[r * 6 + c];
                        for (int m = 0; m < c; m++) s -= Gp[c * 6 + m] * Wk[r * 6 + m];
                        Wk[r * 6 + c] = s * Gp[c * 6 + c];
                    }
                for (int j = 0; j < 6 && sh->status == 0; j++)
                    for (int i = j; i < 6; i++) {
                        double s = Dk[i * 6 + j];
                        for (int c = 0; c < 6; c++) s -= Wk[i * 6 + c] * Wk[j * 6 + c];
                        for (int m = 0; m < j; m++) s -= Gk[i * 6 + m] * Gk[j * 6 + m];
                        if (i == j) {
                            if (s != s || fabs(s) > 1.7e308) { sh->status = pg::kNonFinite; break; }
                            if (!(s > pg::kPivotRel * fabs(Dk[j * 6 + j]))) { sh->status = pg::kNotPositiveDefinite; break; }
                            Gk[j * 6 + j] = 1.0 / sqrt(s);
                        } else {
                            Gk[i * 6 + j] = s * Gk[j * 6 + j];
                        }
                    }
            }
            const int last = nt > 0 ? nt - 1 : 0;
            for (int i = 0; i < 36; i++) sh->prev[i] = sh->G[last * 36 + i];
        }
        ICET_PG_SYNC();
        for (int i = t; i < nt * 36; i += kPgThreads) { G[(size_t)k0 * 36 + i] = sh->G[i]; W[(size_t)k0 * 36 + i] = sh->W[i]; }
    }
    ICET_PG_SYNC();
}

// z = M^{-1} r through the factor: forward u_k = G_k^{-1} (r_k - W_k u_{k-1}), backward z_k = G_k^{-T} (u_k - W_{k+1}^T z_{k+1}).  u: 6 N doubles of scratch.
ICET_PG_DEV void bt_solve(int N, const double* G, const double* W, const double* r, double* z, double* u, PgShared* sh) {
    const int t = ICET_PG_TID;
    double carry[6] = {0, 0, 0, 0, 0, 0};         // (thread 0) the previous node's u, then z
    for (int k0 = 0; k0 < N; k0 += kPgChunk) {
        const int nt = pg_min(kPgChunk, N - k0);
        ICET_PG_SYNC();
        for (int i = t; i < nt * 36; i += kPgThreads) { sh->G[i] = G[(size_t)k0 * 36 + i]; sh->W[i] = W[(size_t)k0 * 36 + i]; }
        for (int i = t; i < nt * 6; i += kPgThreads) sh->v[i] = r[(size_t)k0 * 6 + i];
        ICET_PG_SYNC();
        if (t == 0) {
            for (int k = 0; k < nt; k++) {
                const double* Gk = sh->G + k * 36; const double* Wk = sh->W + k * 36;
                double v[6];
ICET_PG_UNROLL
                for (int a = 0; a < 6; a++) {
                    double s = sh->v[k * 6 + a];
ICET_PG_UNROLL
                    for (int c = 0; c < 6; c++) s -= Wk[a * 6 + c] * carry[c];
                    v[a] = s;
                }
ICET_PG_UNROLL
                for (int a = 0; a < 6; a++) {
                    double s = v[a];
ICET_PG_UNROLL
                    for (int m = 0; m < a; m++) s -= Gk[a * 6 + m] * v[m];
                    v[a] = s * Gk[a * 6 + a];
                }
ICET_PG_UNROLL
                for (int a = 0; a < 6; a++) { carry[a] = v[a]; sh->v[k * 6 + a] = v[a]; }
            }
        }
        ICET_PG_SYNC();
        for (int i = t; i < nt * 6; i += kPgThreads) u[(size_t)k0 * 6 + i] = sh->v[i];
    }
ICET_PG_UNROLL
    for (int a = 0; a < 6; a++) carry[a] = 0.0;
    const int last0 = ((N - 1) / kPgChunk) * kPgChunk;
    for (int k0 = last0; k0 >= 0; k0 -= kPgChunk) {
        const int nt = pg_min(kPgChunk, N - k0);
        ICET_PG_SYNC();
        for (int i = t; i < nt * 36; i += kPgThreads) {
            sh->G[i] = G[(size_t)k0 * 36 + i];
            const size_t wi = (size_t)(k0 + 1) * 36 + i;                       // W of the NEXT node; nothing behind the last
            sh->W[i] = wi < (size_t)N * 36 ? W[wi] : 0.0;
        }
        for (int i = t; i < nt * 6; i += kPgThreads) sh->v[i] = u[(size_t)k0 * 6 + i];
        ICET_PG_SYNC();
        if (t == 0) {
            for (int k = nt - 1; k >= 0; k--) {
                const double* Gk = sh->G + k * 36; const double* Wn = sh->W + k * 36;
                double v[6];
ICET_PG_UNROLL
                for (int a = 0; a < 6; a++) {
                    double s = sh->v[k * 6 + a];
ICET_PG_UNROLL
                    for (int c = 0; c < 6; c++) s -= Wn[c * 6 + a] * carry[c];
                    v[a] = s;
                }
ICET_PG_UNROLL
                for (int a = 5; a >= 0; a--) {
                    double s = v[a];
ICET_PG_UNROLL
                    for (int m = a + 1; m < 6; m++) s -= Gk[m * 6 + a] * v[m];
                    v[a] = s * Gk[a * 6 + a];
                }
ICET_PG_UNROLL
                for (int a = 0; a < 6; a++) { carry[a] = v[a]; sh->v[k * 6 + a] = v[a]; }
            }
        }
        ICET_PG_SYNC();
        for (int i = t; i < nt * 6; i += kPgThreads) z[(size_t)k0 * 6 + i] = sh->v[i];
    }
    ICET_PG_SYNC();
}

// the band solve alone: factor, one right-hand side
ICET_PG_DEV void pg_block_tridiag(int N, const double* Dm, const double* Bm, const double* rhs, double* x, double* G, double* W, double* u, int32_t* status, PgShared& sh) {
    if (ICET_PG_TID == 0) sh.status = 0;
    ICET_PG_SYNC();
    bt_factor(N, Dm, Bm, G, W, &sh);
    if (sh.status == 0) bt_solve(N, G, W, rhs, x, u, &sh);
    else for (int i = ICET_PG_TID; i < N * 6; i += kPgThreads) x[i] = rhs[i];
    if (ICET_PG_TID == 0) *status = sh.status;
}

// ---- the optimiser's kernels (icet_posegraph_driver.h runs them) ----------------------------------------------------------------------
// Every array below is sized exactly (pg_bind): N nodes, E = N - 1 + C edges, off[N] incidence items.  A GRID body takes its global index and does one entry's
// work out of global memory; a GROUP body is one workgroup's (the band sweeps, the reductions).  A node is fixed exactly when its incidence list is empty.
struct PgArgs {
    int N, C, E;
    int trial;                      // kPgChi / kPgStats: 1 = the trial poses Pt and their chit, 0 = P and chi
    int first;                      // kPgPrecond: 1 = the first CG iteration (p = z, r0.z0 recorded)
    int failed;                     // kPgFinish: 1 = the outputs are the inputs
    double damping;
    const float *poses_in, *odo_X, *odo_info, *clo_X, *clo_info;
    float* poses_out; double* poses64_out; double* edge_chi2_out;      // (the last two may be null)
    const int32_t *ei, *ej, *off, *items;
    double *P, *Pt;                 // N x 12: the poses, the trial poses
    double *Om;                     // E x 36: the symmetrised information
    double *J, *OJ;                 // E x 72: the 6 x 12 Jacobians, Omega J
    double *res;                    // E x 6: the residuals at the poses chi was last taken at
    double *chi0, *chi, *chit;      // E: chi2 per edge at the start, at P, at Pt (chi is chi0 until a step is accepted)
    double *spare_chi;              // E: the row that takes chi0's place in the swap of chi and chit
    double *D, *B, *G, *W;          // N x 36: the band M and its factor
    double *A;                      // C x 36: the off-band block at (i, j) of every closure (zeros where there is none)
    double *g, *x, *r, *z, *p, *q, *u;      // N x 6
    double *sc;                     // kPgScalars doubles
};
// sc: r.z | r0.z0 | p.Hp | sum chi2 | max |dx| | status of the factor | status of CG (p.Hp not positive) | spare
constexpr int kPgScalars = 8;
enum PgScalar { kScRz = 0, kScRz0 = 1, kScPq = 2, kScChi = 3, kScMaxDx = 4, kScFactor = 5, kScCg = 6 };
enum PgGridKernel { kPgInit = 0, kPgChi, kPgLinearise, kPgAssemble, kPgOffband, kPgHp, kPgRetract, kPgFinish };
enum PgGroupKernel { kPgFactor = 0, kPgPrecond, kPgStep, kPgStats };

constexpr int kPgLanes = 256;       // the reductions: lane l sums the entries l, l + 256, ... in ascending order, then a binary tree over the lanes -- one order for any thread count
struct PgRed { double lane[kPgLanes]; };

ICET_PG_DEV bool pg_fixed(const PgArgs& a, int k) { return a.off[k + 1] == a.off[k]; }
ICET_PG_DEV const float* pg_meas(const PgArgs& a, int e) { return e < a.N - 1 ? a.odo_X + (size_t)e * 6 : a.clo_X + (size_t)(e - (a.N - 1)) * 6; }

// gi < max(N x 12, E x 36): the state from the caller's float32 arrays (N x 12 covers dx and the scalars)
ICET_PG_DEV void pg_init(const PgArgs& a, int gi) {
    if (gi < a.N * 12) {
        const int k = gi / 12, m = gi % 12;
        a.P[gi] = (double)a.poses_in[(size_t)k * 16 + (m < 9 ? 4 * (m / 3) + m % 3 : 4 * (m - 9) + 3)];
    }
    if (gi < a.E * 36) {
        const int e = gi / 36, r = (gi % 36) / 6, c = gi % 6;
        const float* src = e < a.N - 1 ? a.odo_info + (size_t)e * 36 : a.clo_info + (size_t)(e - (a.N - 1)) * 36;
        a.Om[gi] = 0.5 * ((double)src[r * 6 + c] + (double)src[c * 6 + r]);
    }
    if (gi < a.N * 6) a.x[gi] = 0.0;
    if (gi < kPgScalars) a.sc[gi] = 0.0;
}

// e < E: the residual and chi2 of one edge
ICET_PG_DEV void pg_chi(const PgArgs& a, int e) {
    const double* T = a.trial ? a.Pt : a.P;
    double r6[6];
    pg::residual(T + (size_t)a.ei[e] * 12, T + (size_t)a.ej[e] * 12, pg_meas(a, e), r6);
    const double* Om = a.Om + (size_t)e * 36;
    double s = 0.0;
ICET_PG_UNROLL
    for (int m = 0; m < 6; m++) {
        double w = 0.0;
ICET_PG_UNROLL
        for (int n = 0; n < 6; n++) w += Om[m * 6 + n] * r6[n];
        s += r6[m] * w;
        a.res[(size_t)e * 6 + m] = r6[m];
    }
    (a.trial ? a.chit : a.chi)[e] = s;
}

// gi < E x 12: one column of an edge's Jacobian and of Omega J
ICET_PG_DEV void pg_linearise(const PgArgs& a, int gi) {
    const int e = gi / 12, col = gi % 12;
    double jc[6];
    pg::jacobian_column(a.P + (size_t)a.ei[e] * 12, a.P + (size_t)a.ej[e] * 12, col, jc);
    const double* Om = a.Om + (size_t)e * 36;
ICET_PG_UNROLL
    for (int m = 0; m < 6; m++) {
        double w = 0.0;
ICET_PG_UNROLL
        for (int n = 0; n < 6; n++) w += Om[m * 6 + n] * jc[n];
        a.J[(size_t)e * 72 + m * 12 + col] = jc[m];
        a.OJ[(size_t)e * 72 + m * 12 + col] = w;
    }
}

// gi < N x 36: entry (r, c) of node k's diagonal block D_k and of its coupling B_k to node k - 1, and (c == 0) entry r of g_k, over the node's incidence list
// in its order.  D's entry (r, c) is computed as (max, min): both triangles carry the same bits.
ICET_PG_DEV void pg_assemble(const PgArgs& a, int gi) {
    const int k = gi / 36, r = (gi % 36) / 6, c = gi % 6;
    const int rr = r > c ? r : c, cc = r > c ? c : r;
    double d = 0.0, b = 0.0, gr = 0.0;
    const int i0 = a.off[k], i1 = a.off[k + 1];
    if (i0 == i1) d = r == c ? 1.0 : 0.0;
    for (int it = i0; it < i1; it++) {
        const int item = a.items[it], e = item >> 1, side = item & 1;
        const int other = side ? a.ei[e] : a.ej[e];
        const double* Je = a.J + (size_t)e * 72 + 6 * side;
        const double* Oe = a.OJ + (size_t)e * 72 + 6 * side;
        double s = 0.0;
        for (int m = 0; m < 6; m++) s += Je[m * 12 + rr] * Oe[m * 12 + cc];
        d += s;
        if (other == k - 1 && !pg_fixed(a, other)) {
            const double* Oo = a.OJ + (size_t)e * 72 + 6 * (1 - side);
            double t = 0.0;
            for (int m = 0; m < 6; m++) t += Je[m * 12 + r] * Oo[m * 12 + c];
            b += t;
        }
        if (c == 0) {
            double t = 0.0;
            for (int m = 0; m < 6; m++) t += Oe[m * 12 + r] * a.res[(size_t)e * 6 + m];
            gr += t;
        }
    }
    if (i0 != i1 && r == c) d += a.damping;
    a.D[gi] = d;
    a.B[gi] = b;
    if (c == 0) a.g[(size_t)k * 6 + r] = gr;
}

// gi < C x 36: entry (r, c) of the block at (i, j) of closure gi / 36 when it lies off the band and both ends are free, else zero
ICET_PG_DEV void pg_offband(const PgArgs& a, int gi) {
    const int cl = gi / 36, r = (gi % 36) / 6, c = gi % 6, e = a.N - 1 + cl;
    const int i = a.ei[e], j = a.ej[e];
    double s = 0.0;
    if ((i - j >= 2 || j - i >= 2) && !pg_fixed(a, i) && !pg_fixed(a, j)) {
        const double* Je = a.J + (size_t)e * 72;
        const double* Oe = a.OJ + (size_t)e * 72 + 6;
        for (int m = 0; m < 6; m++) s += Je[m * 12 + r] * Oe[m * 12 + c];
    }
    a.A[gi] = s;
}

// gi < N x 6: one row of q = H p, matrix-free: D, the two couplings, then the node's off-band closures in incidence order
ICET_PG_DEV void pg_hp(const PgArgs& a, int gi) {
    const int k = gi / 6, r = gi % 6;
    const double* p = a.p;
    double s = 0.0;
    for (int c = 0; c < 6; c++) s += a.D[(size_t)k * 36 + r * 6 + c] * p[(size_t)k * 6 + c];
    if (k > 0) for (int c = 0; c < 6; c++) s += a.B[(size_t)k * 36 + r * 6 + c] * p[(size_t)(k - 1) * 6 + c];
    if (k < a.N - 1) for (int c = 0; c < 6; c++) s += a.B[(size_t)(k + 1) * 36 + c * 6 + r] * p[(size_t)(k + 1) * 6 + c];
    for (int it = a.off[k]; it < a.off[k + 1]; it++) {
        const int item = a.items[it], e = item >> 1, side = item & 1;
        if (e < a.N - 1) continue;
        const int other = side ? a.ei[e] : a.ej[e];
        if (other - k < 2 && k - other < 2) continue;
        const double* Ac = a.A + (size_t)(e - (a.N - 1)) * 36;
        if (side == 0) for (int c = 0; c < 6; c++) s += Ac[r * 6 + c] * p[(size_t)other * 6 + c];
        else           for (int c = 0; c < 6; c++) s += Ac[c * 6 + r] * p[(size_t)other * 6 + c];
    }
    a.q[gi] = s;
}

// k < N: the trial pose T_k Exp(dx_k)
ICET_PG_DEV void pg_retract(const PgArgs& a, int k) {
    if (pg_fixed(a, k)) { for (int m = 0; m < 12; m++) a.Pt[(size_t)k * 12 + m] = a.P[(size_t)k * 12 + m]; return; }
    pg::exp_update(a.P + (size_t)k * 12, a.x + (size_t)k * 6, a.Pt + (size_t)k * 12);
}

// gi < max(N, E): the outputs.  A fixed node, and every node of a failed run, returns its input bits.
ICET_PG_DEV void pg_finish(const PgArgs& a, int gi) {
    if (gi < a.N) {
        const float* in = a.poses_in + (size_t)gi * 16;
        float* out = a.poses_out + (size_t)gi * 16;
        if (a.failed || pg_fixed(a, gi)) { for (int m = 0; m < 16; m++) out[m] = in[m]; }
        else pg::pose_to_float(a.P + (size_t)gi * 12, out);
        if (a.poses64_out) {
            if (a.failed) pg::pose_from_float(in, a.poses64_out + (size_t)gi * 12);
            else for (int m = 0; m < 12; m++) a.poses64_out[(size_t)gi * 12 + m] = a.P[(size_t)gi * 12 + m];
        }
    }
    if (gi < a.E && a.edge_chi2_out) {
        a.edge_chi2_out[gi] = a.chi0[gi];
        a.edge_chi2_out[(size_t)a.E + gi] = a.failed ? a.chi0[gi] : a.chi[gi];
    }
}

// ---- one workgroup -----------------------------------------------------------------------------------------------------------------------------------------
ICET_PG_DEV double pg_dot(int n, const double* a, const double* b, PgRed* red) {
    const int t = ICET_PG_TID;
    for (int l = t; l < kPgLanes; l += kPgThreads) {
        double s = 0.0;
        for (int i = l; i < n; i += kPgLanes) s += a[i] * b[i];
        red->lane[l] = s;
    }
    ICET_PG_SYNC();
    for (int h = kPgLanes / 2; h > 0; h >>= 1) {
        for (int l = t; l < h; l += kPgThreads) red->lane[l] += red->lane[l + h];
        ICET_PG_SYNC();
    }
    const double s = red->lane[0];
    ICET_PG_SYNC();
    return s;
}

// the factor of the band, once per Gauss-Newton iteration; x = 0, r = -g
ICET_PG_DEV void pg_group_factor(const PgArgs& a, PgShared& sh) {
    const int t = ICET_PG_TID;
    if (t == 0) sh.status = 0;
    ICET_PG_SYNC();
    bt_factor(a.N, a.D, a.B, a.G, a.W, &sh);
    for (int i = t; i < a.N * 6; i += kPgThreads) { a.x[i] = 0.0; a.r[i] = -a.g[i]; }
    if (t == 0) { a.sc[kScFactor] = (double)sh.status; a.sc[kScCg] = 0.0; }
    ICET_PG_SYNC();
}

// z = M^-1 r, r.z, and the next direction p = z + (r.z / the previous r.z) p
ICET_PG_DEV void pg_group_precond(const PgArgs& a, PgShared& sh, PgRed& red) {
    const int t = ICET_PG_TID;
    if (a.sc[kScFactor] != 0.0 || a.sc[kScCg] != 0.0) return;      // (the same for every thread: nothing below has written them)
    bt_solve(a.N, a.G, a.W, a.r, a.z, a.u, &sh);
    const double rz = pg_dot(a.N * 6, a.r, a.z, &red);
    const double beta = a.first ? 0.0 : rz / a.sc[kScRz];
    for (int i = t; i < a.N * 6; i += kPgThreads) a.p[i] = a.first ? a.z[i] : a.z[i] + beta * a.p[i];
    ICET_PG_SYNC();
    if (t == 0) { a.sc[kScRz] = rz; if (a.first) a.sc[kScRz0] = rz; }
    ICET_PG_SYNC();
}

// the step along p: alpha = r.z / p.Hp, x += alpha p, r -= alpha q
ICET_PG_DEV void pg_group_step(const PgArgs& a, PgRed& red) {
    const int t = ICET_PG_TID;
    const double pq = pg_dot(a.N * 6, a.p, a.q, &red);
    if (pq > 0.0) {
        const double alpha = a.sc[kScRz] / pq;
        for (int i = t; i < a.N * 6; i += kPgThreads) { a.x[i] += alpha * a.p[i]; a.r[i] -= alpha * a.q[i]; }
    }
    if (t == 0) { a.sc[kScPq] = pq; if (!(pq > 0.0)) a.sc[kScCg] = (double)(pq != pq ? pg::kNonFinite : pg::kNotPositiveDefinite); }
    ICET_PG_SYNC();
}

// sum of chi2 over the edges, max |dx|
ICET_PG_DEV void pg_group_stats(const PgArgs& a, PgRed& red) {
    const int t = ICET_PG_TID;
    const double* chi = a.trial ? a.chit : a.chi;
    for (int l = t; l < kPgLanes; l += kPgThreads) {
        double s = 0.0;
        for (int i = l; i < a.E; i += kPgLanes) s += chi[i];
        red.lane[l] = s;
    }
    ICET_PG_SYNC();
    for (int h = kPgLanes / 2; h > 0; h >>= 1) {
        for (int l = t; l < h; l += kPgThreads) red.lane[l] += red.lane[l + h];
        ICET_PG_SYNC();
    }
    if (t == 0) a.sc[kScChi] = red.lane[0];
    ICET_PG_SYNC();
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
