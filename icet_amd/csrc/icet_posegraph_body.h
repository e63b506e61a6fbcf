// icet_amd/csrc/icet_posegraph_body.h -- the block-tridiagonal solve of the pose-graph work, as one workgroup runs it
// (icet_posegraph.hip has the launch and the host entry point).  Under hipcc this is device code for 256 threads.  Under a host compiler the same text runs as a "workgroup" of ONE thread (every strided
// loop then covers its whole range, the barriers are empty): tests/cpp/test_posegraph.cpp runs the algebra that way, under the address sanitizer too.
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
}  // namespace icet
