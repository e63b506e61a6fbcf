"""CPU tests of the pose-graph work (-m "not gpu"): the NumPy model of the contract (tests/pose_graph_model.py) against scipy.optimize.least_squares and
against the ground truth, the consistency of a chain built with pose_step_from_X, the host side of the device code (tests/cpp/test_posegraph.cpp, also under
the address and undefined-behaviour sanitizers), the Python helpers, and the refusal of the band-solve hook that needs no device."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_model as pgm      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a tenth of the smallest sigma of the test graphs (pgm.SIGMA_CLOSURE): no disagreement the tests accept may exceed it
CAP_T, CAP_R = 0.1 * pgm.SIGMA_CLOSURE[0], 0.1 * pgm.SIGMA_CLOSURE[1]


def test_model_agrees_with_scipy_least_squares():
    """12-node loop, 2 closures: the model's Gauss-Newton and scipy's trust-region solver minimise the same residuals L^T e (info = L L^T) over
    T_k = T0_k Exp(xi_k).  least_squares is run to xtol = ftol = gtol = 1e-14; the model stops at |dx| < 1e-7 in a quadratically convergent iteration, so
    the poses must agree to 1e-7 (m, rad) and chi2 to 1e-9 relative."""
    from scipy.optimize import least_squares
    g = pgm.make_loop(12, [(0, 11), (2, 9)], seed=3)
    m = pgm.optimise(g["poses"], g["odo_X"], g["odo_info"], g["closures"])
    assert m["status"] == pgm.CONVERGED and m["chi2_final"] < m["chi2_initial"] and m["gn_iterations"] <= 6
    n = 12
    edges = pgm.edge_list(n, g["closures"])
    X, info = pgm._measurements(n, g["odo_X"], g["odo_info"], g["closures"])
    Ls = [np.linalg.cholesky(w) for w in info]
    T0 = g["poses"].astype(np.float64)

    def poses_of(xi):
        T = T0.copy()
        for k in range(1, n):
            T[k] = T0[k] @ pgm.exp_se3(xi[6 * (k - 1):6 * k])
        return T

    def res(xi):
        T = poses_of(xi)
        return np.concatenate([Ls[q].T @ pgm.residual(T[i], T[j], X[q]) for q, (i, j) in enumerate(edges)])

    sol = least_squares(res, np.zeros(6 * (n - 1)), method="trf", xtol=1e-14, ftol=1e-14, gtol=1e-14, x_scale=1.0, max_nfev=200)
    chi2_ls = 2.0 * sol.cost
    dt, dr = pgm.pose_error(poses_of(sol.x), m["poses64"])
    print("model chi2 %.12g, least_squares chi2 %.12g, poses differ by %.2e m %.2e rad" % (m["chi2_final"], chi2_ls, dt, dr))
    assert abs(m["chi2_final"] - chi2_ls) <= 1e-9 * chi2_ls
    assert dt <= 1e-7 and dr <= 1e-7


@pytest.mark.parametrize("n,pairs", [(12, [(0, 11), (2, 9)]), (33, [(0, 32), (1, 30), (5, 31)]), (65, [(0, 64), (3, 60), (10, 63)])])
def test_model_recovers_a_noise_free_graph(n, pairs):
    """Exact measurements (rounded to float32), the start a chain of noisy odometry: the model must land on the truth within a tenth of the smallest sigma --
    the cap that every device-against-model tolerance has to respect as well."""
    g, drifted = pgm.make_loop(n, pairs, seed=11, noise=0.0), pgm.make_loop(n, pairs, seed=11, noise=1.0)
    before = pgm.pose_error(drifted["poses"], g["truth"])
    m = pgm.optimise(drifted["poses"], g["odo_X"], g["odo_info"], g["closures"])
    dt, dr = pgm.pose_error(m["poses"], g["truth"])
    print("n = %d: drifted %.3e m %.3e rad, optimised %.3e m %.3e rad of the truth, chi2 %.3e -> %.3e" % (n, before[0], before[1], dt, dr, m["chi2_initial"], m["chi2_final"]))
    assert m["status"] == pgm.CONVERGED and before[0] > 10 * CAP_T
    assert dt <= CAP_T and dr <= CAP_R


def test_chain_from_pose_step_has_zero_odometry_chi2():
    """T_k = T_(k-1) pose_step_from_X(X_k): every odometry residual is the float32 rounding of the poses and steps.  Per edge the two poses and the step carry
    at most 4 roundings of 2^-24 relative on a coordinate of at most 8 m and on rotation entries of at most 1, against sigmas of 1 cm / 0.5 mrad."""
    from icet_amd import api
    g = pgm.make_loop(65, [], seed=5)
    T = [g["truth"][0].astype(np.float32)]
    for x in g["odo_X"]:
        T.append((T[-1].astype(np.float64) @ api.pose_step_from_X(x).astype(np.float64)).astype(np.float32))
    T = np.array(T)
    assert np.abs(T - g["poses"]).max() <= 64 * 2.0 ** -24 * 8.0          # (the model's chain rounds once per pose from a double product; this one rounds every link: 64 roundings of a coordinate below 8 m)
    chi = pgm.edge_chi2(T.astype(np.float64), pgm.edge_list(65, []), *pgm._measurements(65, g["odo_X"], g["odo_info"], []))
    ulp = 2.0 ** -24
    bound = 3 * (4 * ulp * 8.0 / pgm.SIGMA_ODO[0]) ** 2 + 3 * (4 * ulp / pgm.SIGMA_ODO[1]) ** 2
    print("largest odometry chi2 of a consistent chain: %.3e (bound %.3e)" % (chi.max(), bound))
    assert chi.max() <= bound
    m = pgm.optimise(T, g["odo_X"], g["odo_info"])
    # the optimum of a chain alone is the exact product of the steps: it undoes the 64 link roundings, nothing more
    print("status %d, chi2 %.3e -> %.3e, poses moved by %.3e" % (m["status"], m["chi2_initial"], m["chi2_final"], np.abs(m["poses"] - T).max()))
    assert m["status"] == pgm.CONVERGED and m["chi2_final"] <= m["chi2_initial"] and np.abs(m["poses"] - T).max() <= 64 * ulp * 8.0
    m = pgm.optimise(g["poses"], g["odo_X"], g["odo_info"])          # the chain rounded once per pose: one rounding
    assert m["status"] == pgm.CONVERGED and np.abs(m["poses"] - g["poses"]).max() <= 2 * ulp * 8.0


def test_host_side_of_the_device_code(tmp_path):
    """tests/cpp/test_posegraph.cpp: Xof against the store's start-pose rule, Exp, the wrap at +-pi, the incidence lists of repeated, adjacent, reversed and
    fixed-node closures, and the band solve's workgroup body run as one thread (at the chunk boundaries, a singular block) -- plain and
    under -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "test_posegraph.cpp")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("test_posegraph_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", ROOT, src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_info_from_cov_and_closure_edges():
    from icet_amd import api
    rs = np.random.RandomState(2)
    A = rs.standard_normal((6, 6)); cov = (A @ A.T * 1e-4).astype(np.float32)
    info = api.info_from_cov(cov)
    assert info.dtype == np.float32 and info.shape == (6, 6) and np.array_equal(info, info.T)
    assert np.abs(info.astype(np.float64) @ cov.astype(np.float64) - np.eye(6)).max() < 1e-3
    cov[2, :] = 0; cov[:, 2] = 0                           # a pruned axis: the pseudo-inverse has it as a null direction
    info = api.info_from_cov(cov)
    assert np.abs(info[2]).max() <= 1e-12 * np.abs(info).max() and np.array_equal(info, info.T) and np.linalg.matrix_rank(info.astype(np.float64)) == 5
    recs = [dict(slot=4, accepted=True, X=np.arange(6, dtype=np.float32), cov=np.eye(6, dtype=np.float32)),
            dict(slot=None, accepted=False, X=None, cov=None),
            dict(slot=2, accepted=False, X=np.zeros(6, np.float32), cov=np.eye(6, dtype=np.float32)),
            dict(slot=7, accepted=True, X=np.ones(6, np.float32), cov=np.eye(6, dtype=np.float32))]
    edges = api.closure_edges(recs, [20, 21, 22, 17], {4: 3, 2: 1, 7: 17})
    assert len(edges) == 1 and edges[0][0] == 3 and edges[0][1] == 20 and np.array_equal(edges[0][2], np.arange(6)) and np.array_equal(edges[0][3], np.eye(6))


def test_abi_of_the_band_solve_hook():
    import icet_amd
    from icet_amd import api
    lib = icet_amd.load_library()
    assert "icet_debug_block_tridiag" in api.EXPORTED_SYMBOLS and lib.icet_debug_block_tridiag is not None
    assert lib.icet_debug_block_tridiag(None, 1, None, None, None, None, None) == api.ICET_ERR_BAD_ARG
