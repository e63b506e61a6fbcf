"""GPU tests of the block-tridiagonal solve that pose-graph optimisation needs (icet_debug_block_tridiag): the relative residual against
numpy.linalg.solve's own at the sizes where a chunk or a wave boundary goes wrong, and the report of a singular block."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_model as pgm      # noqa: E402

pytestmark = pytest.mark.gpu


# ---- 1. the block-tridiagonal solve alone ------------------------------------------------------------------------------------------------------------------
BAND_SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 257)


def _band_system(n, seed):
    """A chain of SPD 6 x 6 stiffness blocks K_k between x_(k-1) and x_k (x_(-1) = 0): block tridiagonal, SPD; the blocks' condition numbers run from 1e2 to
    1e8, every third one is 1e8."""
    rs = np.random.RandomState(seed)
    D, B = np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    for k in range(n):
        A = rs.standard_normal((6, 6))
        cond = 1e8 if k % 3 == 0 else 10.0 ** rs.uniform(2, 8)
        K = (A * cond ** (np.arange(6) / 5.0 - 1.0)) @ A.T
        K = 0.5 * (K + K.T)
        D[k] += K
        if k > 0:
            D[k - 1] += K; B[k] = -K
    return D, B, rs.standard_normal((n, 6))


def _dense(D, B):
    n = len(D)
    M = np.zeros((6 * n, 6 * n))
    for k in range(n):
        M[6 * k:6 * k + 6, 6 * k:6 * k + 6] = D[k]
        if k > 0:
            M[6 * k:6 * k + 6, 6 * k - 6:6 * k] = B[k]; M[6 * k - 6:6 * k, 6 * k:6 * k + 6] = B[k].T
    return M


@pytest.fixture(scope="module")
def band(gpu_ctx):
    """Every size once: numpy.linalg.solve's relative residual and the device's."""
    out = {}
    for n in BAND_SIZES:
        D, B, r = _band_system(n, 1000 + n)
        M, b = _dense(D, B), r.ravel()
        ref = np.linalg.norm(M @ np.linalg.solve(M, b) - b) / np.linalg.norm(b)
        x, st = gpu_ctx.debug_block_tridiag(D, B, r)
        out[n] = (ref, np.linalg.norm(M @ x.ravel() - b) / np.linalg.norm(b), st)
    print("block-tridiagonal solve, |Mx - b| / |b|  (numpy.linalg.solve | device): " + ", ".join("N=%d %.2e | %.2e" % (n, out[n][0], out[n][1]) for n in BAND_SIZES))
    return out


@pytest.mark.parametrize("n", BAND_SIZES)
def test_block_tridiagonal_solve_against_numpy(band, n):
    """Relative residual at most 16 x the worst residual numpy.linalg.solve leaves on these systems (the margin covers the different elimination order).
    Measured on an MI355X: see DESIGN.md section 20."""
    worst_ref = max(v[0] for v in band.values())
    ref, got, st = band[n]
    assert st == 0 and np.isfinite(got)
    assert got <= 16 * worst_ref, (n, got, worst_ref)


def test_block_tridiagonal_solve_reports_a_singular_block(gpu_ctx):
    D, B, r = _band_system(5, 7)
    D[3] = 0.0                                          # no positive pivot in block 3
    x, st = gpu_ctx.debug_block_tridiag(D, B, r)
    assert st == pgm.NOT_POSITIVE_DEFINITE and np.array_equal(x, r)
