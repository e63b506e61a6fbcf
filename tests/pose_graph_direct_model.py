"""The pose-graph optimiser's DIRECT solve restated in float64 NumPy (DESIGN.md section 20 "The direct solve"), from the band blocks D, B and the off-band
blocks A as the device holds them, with every intermediate array returned; and pgm.optimise with that solve in place of numpy.linalg.solve.  Nothing here is
shared with the device code.  Also the graphs, the file formats of tests/cpp/test_posegraph_direct.cpp and the checks that tests/test_pose_graph_direct_step.py
runs on the host build's and on the device's hook output."""
import os
import struct
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_model as pgm      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
          ("emu", ["-O2", "-DICET_PG_EMU", "-pthread"]), ("emu_san", ["-O1", "-g", "-DICET_PG_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def build_and_run(tmp, fin, mode=()):
    """tests/cpp/test_posegraph_direct.cpp built four ways and run on the file fin: the four outputs must be the same bytes, the sanitised runs must end clean.
    Returns the path of the plain build's output."""
    src = os.path.join(ROOT, "tests", "cpp", "test_posegraph_direct.cpp")
    outs = {}
    for name, flags in BUILDS:
        exe = str(tmp / ("test_posegraph_direct_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", ROOT, src, "-o", exe])
        fout = str(tmp / (name + ".bin"))
        r = subprocess.run([exe, *mode, fin, fout], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "ERROR" not in r.stderr, (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        outs[name] = open(fout, "rb").read()
        if name == "plain":
            print(r.stdout)
    assert outs["plain"] == outs["san"] == outs["emu"] == outs["emu_san"]
    return str(tmp / "plain.bin")


REFINE = 1          # kPgDirectRefine
MAX_ENDS = 128      # kPgDirectMaxEnds


def ends_of(n, closures, is_fixed):
    """The distinct nodes that are an end of a closure with |i - j| >= 2 and both ends free, ascending.  closures: (i, j, ...) tuples."""
    ends = set()
    for c in closures:
        i, j = int(c[0]), int(c[1])
        if abs(i - j) >= 2 and not is_fixed[i] and not is_fixed[j]:
            ends.update((i, j))
    return sorted(ends)


def dense_band(D, B):
    """The dense 6n x 6n band M over ALL nodes from D n x 6 x 6 and B n x 6 x 6 (B[k] at (k, k - 1)); a fixed node carries the identity and no coupling."""
    D, B = np.asarray(D, np.float64).reshape(-1, 6, 6), np.asarray(B, np.float64).reshape(-1, 6, 6)
    n = D.shape[0]
    M = np.zeros((6 * n, 6 * n))
    for k in range(n):
        M[6 * k:6 * k + 6, 6 * k:6 * k + 6] = D[k]
        if k > 0:
            M[6 * k:6 * k + 6, 6 * k - 6:6 * k] = B[k]; M[6 * k - 6:6 * k, 6 * k:6 * k + 6] = B[k].T
    return M


def s_matrix(A, edges, ends, is_fixed, n, dtype=np.float64):
    """S = U^T R U (q x q): block (a, b) sums A_c over the closures (ends[a], ends[b]) and A_c^T over the closures (ends[b], ends[a])."""
    A = np.asarray(A, dtype).reshape(-1, 6, 6)
    end_of = {k: a for a, k in enumerate(ends)}
    S = np.zeros((6 * len(ends), 6 * len(ends)), dtype)
    for c, (i, j) in enumerate(edges[n - 1:]):
        if abs(i - j) >= 2 and not is_fixed[i] and not is_fixed[j]:
            a, b = end_of[i], end_of[j]
            S[6 * a:6 * a + 6, 6 * b:6 * b + 6] += A[c]; S[6 * b:6 * b + 6, 6 * a:6 * a + 6] += A[c].T
    return S


def _mirror(X):
    """Both triangles from the lower one: entry (r, c) read at (max, min)."""
    return np.tril(X) + np.tril(X, -1).T


def direct_solve(D, B, A, g, edges, is_fixed, band_solver=None, refine=REFINE):
    """Steps 1-7.  D, B n x 6 x 6, A C x 6 x 6, g n x 6 (zero rows at fixed nodes), edges as pgm.edge_list.  band_solver(M) -> (r -> M^-1 r), default
    pgm.band_solver.  dict(status 0 | 2 | 3, ends, M, S, H, Z, Wm, L, Ks, Lk, x0, x (n x 6), band_solves)."""
    D = np.asarray(D, np.float64).reshape(-1, 6, 6)
    n = D.shape[0]
    is_fixed = np.asarray(is_fixed, bool)
    ends = ends_of(n, edges[n - 1:], is_fixed)
    q = 6 * len(ends)
    M = dense_band(D, B)
    gv = np.asarray(g, np.float64).reshape(-1)
    out = dict(status=0, ends=ends, M=M, band_solves=0)
    solve = (band_solver or pgm.band_solver)(M)
    if q == 0:
        x = solve(-gv)
        return dict(out, S=np.zeros((0, 0)), H=M, x0=x.reshape(n, 6), x=x.reshape(n, 6), band_solves=1)
    U = np.zeros((6 * n, q))
    for a, k in enumerate(ends):
        U[6 * k:6 * k + 6, 6 * a:6 * a + 6] = np.eye(6)
    S = s_matrix(A, edges, ends, is_fixed, n)
    H = M + U @ S @ U.T
    Z = solve(U)
    Wm = _mirror(U.T @ Z)
    out.update(S=S, H=H, Z=Z, Wm=Wm)
    if not np.isfinite(Wm).all():
        return dict(out, status=pgm.NON_FINITE)
    try:
        L = np.linalg.cholesky(Wm)
    except np.linalg.LinAlgError:
        return dict(out, status=pgm.NOT_POSITIVE_DEFINITE)
    Ks = _mirror(np.eye(q) + L.T @ (S @ L))
    out.update(L=L, Ks=Ks)
    if not np.isfinite(Ks).all():
        return dict(out, status=pgm.NON_FINITE)
    try:
        Lk = np.linalg.cholesky(Ks)
    except np.linalg.LinAlgError:
        return dict(out, status=pgm.NOT_POSITIVE_DEFINITE)

    def apply(b):
        y = solve(b)
        t = L.T @ (S @ (U.T @ y))
        u = np.linalg.solve(Lk.T, np.linalg.solve(Lk, t))
        return y - Z @ np.linalg.solve(L.T, u)
    x0 = apply(-gv)
    x = x0.copy()
    for _ in range(refine):
        x = x + apply(-gv - H @ x)
    return dict(out, Lk=Lk, x0=x0.reshape(n, 6), x=x.reshape(n, 6), band_solves=1 + refine)


def blocks_of(H, Js, info, edges, is_fixed):
    """The device's D, B, A from the model's linearisation: D, B out of the dense free-node H (identity and zero at fixed nodes), A_c = J_i^T Omega J_j per
    closure off the band between two free nodes."""
    is_fixed = np.asarray(is_fixed, bool)
    n = is_fixed.size
    free = np.nonzero(~is_fixed)[0]
    col = -np.ones(n, int); col[free] = np.arange(free.size)
    D, B, A = np.tile(np.eye(6), (n, 1, 1)), np.zeros((n, 6, 6)), np.zeros((len(edges) - (n - 1), 6, 6))
    for k in free:
        D[k] = H[6 * col[k]:6 * col[k] + 6, 6 * col[k]:6 * col[k] + 6]
        if k > 0 and col[k - 1] >= 0:
            B[k] = H[6 * col[k]:6 * col[k] + 6, 6 * col[k - 1]:6 * col[k - 1] + 6]
    for c, (i, j) in enumerate(edges[n - 1:]):
        if abs(i - j) >= 2 and not is_fixed[i] and not is_fixed[j]:
            J = Js[n - 1 + c]
            A[c] = J[:, :6].T @ info[n - 1 + c] @ J[:, 6:]
    return D, B, A


def optimise_direct(poses, odo_X, odo_info, closures=(), fixed=None, gn_iters=10, dx_tol=1e-7, damping=0.0):
    """pgm.optimise with direct_solve as its linear solve: a failed factorisation of the band (numpy's Cholesky of M), of Wm or of Ks is status 2, a value
    that is not finite status 3; the outputs are then the inputs.  Adds pcg_iterations (the single band solves)."""
    P32 = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    n = P32.shape[0]
    closures = list(closures)
    edges = pgm.edge_list(n, closures)
    X, info = pgm._measurements(n, odo_X, odo_info, closures)
    is_fixed = pgm.fixed_mask(n, fixed)
    free = np.nonzero(~is_fixed)[0]
    T = P32.astype(np.float64)
    chi0 = pgm.edge_chi2(T, edges, X, info)
    chi_e, chi2 = chi0.copy(), float(chi0.sum())
    status, its, max_dx, failed, solves = pgm.ITERATION_CAP, 0, 0.0, False, 0
    if not np.isfinite(chi2):
        status, failed = pgm.NON_FINITE, True
    for _ in range(gn_iters if not failed else 0):
        its += 1
        Js, _, H, g = pgm.linearise(T, edges, X, info, is_fixed, damping)
        if not (np.isfinite(H).all() and np.isfinite(g).all()):
            status, failed = pgm.NON_FINITE, True; break
        D, B, A = blocks_of(H, Js, info, edges, is_fixed)
        try:
            np.linalg.cholesky(dense_band(D, B))
        except np.linalg.LinAlgError:
            status, failed = pgm.NOT_POSITIVE_DEFINITE, True; break
        gn = np.zeros((n, 6)); gn[free] = g.reshape(-1, 6)
        s = direct_solve(D, B, A, gn, edges, is_fixed)
        if s["status"]:
            status, failed = s["status"], True; break
        solves += s["band_solves"]
        dx = s["x"]
        max_dx = float(np.abs(dx).max())
        Tt = T.copy()
        for k in free:
            Tt[k] = T[k] @ pgm.exp_se3(dx[k])
        chit = pgm.edge_chi2(Tt, edges, X, info)
        if not np.isfinite(chit.sum()):
            status, failed = pgm.NON_FINITE, True; break
        if not (chit.sum() < chi2):
            status = pgm.CONVERGED if max_dx < dx_tol else pgm.STALLED
            break
        T, chi_e, chi2 = Tt, chit, float(chit.sum())
        if max_dx < dx_tol:
            status = pgm.CONVERGED
            break
    out = T.astype(np.float32)
    out[:, 3, :] = (0, 0, 0, 1)
    if failed:
        out, chi_e, chi2, T = P32.copy(), chi0, float(chi0.sum()), P32.astype(np.float64)
    out[is_fixed] = P32[is_fixed]
    return dict(poses=out, poses64=T, chi2_initial=float(chi0.sum()), chi2_final=chi2, status=status, gn_iterations=its, max_dx=max_dx, edge_chi2=np.stack([chi0, chi_e]),
                pcg_iterations=solves)


# ---- the graphs the direct solve's tests share -------------------------------------------------------------------------------------------------------------------
ENDS288_PAIRS = tuple([(k, k + 60) for k in range(1, 25)] + [(k + 30, k + 90) for k in range(1, 25)])
OVER_LIMIT_PAIRS = tuple((k, k + 70) for k in range(1, 70))


def ends288_graph():
    """120 poses, 48 closures with 96 distinct ends: q = 576 crosses 256 threads twice and a 256-thread grid block."""
    return dict(pgm.make_loop(120, list(ENDS288_PAIRS), seed=11), fixed=None)


def over_limit_graph():
    """140 poses, 69 closures with 138 distinct ends: above kPgDirectMaxEnds."""
    return dict(pgm.make_loop(140, list(OVER_LIMIT_PAIRS), seed=11), fixed=None)


def m0_graph():
    """A graph whose only closures have a fixed far end or lie on the band: no end node."""
    g = pgm.make_loop(12, [(0, 7), (3, 4), (5, 4), (9, 6)], seed=11)
    fixed = np.zeros(12, np.uint8); fixed[6] = 1
    return dict(g, fixed=fixed)


def whole_run_items():
    """The items of tests/test_pose_graph_optimize_host.py's list that a direct run answers (max_pcg and pcg_tol do not exist for it), strong at default options."""
    items = []
    for (n, pairs, fx) in pc.CASES:
        for noisy in (True, False):
            if n == 257 and not noisy:
                continue
            items.append((("loop", n, pairs, fx, noisy), pc.graph(n, pairs, fx, noisy), {}))
    items.append((("chain", 65), dict(pgm.make_loop(65, [], seed=11), fixed=None), {}))
    items.append((("rank5",), pc.rank5_graph(), {}))
    items.append((("zero_row",), pc.zero_row_graph(), {}))
    items.append((("nan",), pc.nan_graph(), {}))
    items.append((("cap",), pc.graph(33, pc.CASES[4][1], None, True), dict(gn_iters=1)))
    items.append((("damped",), pc.graph(33, pc.CASES[4][1], None, True), dict(damping=1e-3)))
    items.append((("single",), dict(pgm.make_loop(1, [], seed=11), fixed=None), {}))
    items.append((("seam",), pc.seam_graph(), {}))
    items.append((("stalled",), pc.stalled_graph(), {}))
    items.append((("negative",), pc.negative_graph(), {}))
    items.append((("negative_cg",), pc.negative_graph(0.1), {}))
    items.append((("strong",), pc.strong_graph(), {}))
    return items


def graph_ends(g):
    n = g["poses"].shape[0]
    return ends_of(n, g["closures"], pgm.fixed_mask(n, g["fixed"]))


def check_whole_run(key, g, o, r):
    """One whole direct run r against pgm.optimise (pc.model): pc.compare with pc's tolerances, status and gn_iterations the model's, the band solves counted."""
    m = pc.model(key, g, **pc.model_options(o))
    n_ends = len(graph_ends(g))
    print(key[:2], "status", r["status"], "|", m["status"], "iterations", r["gn_iterations"], "|", m["gn_iterations"], "band solves", r["pcg_iterations"], "ends", n_ends)
    assert r["status"] == m["status"] and r["gn_iterations"] == m["gn_iterations"]
    if key[0] in ("zero_row", "nan", "negative", "negative_cg"):
        assert r["status"] == (pgm.NON_FINITE if key[0] == "nan" else pgm.NOT_POSITIVE_DEFINITE)
        assert r["gn_iterations"] == (0 if key[0] == "nan" else 1)
        assert np.array_equal(np.asarray(r["poses"]).view(np.uint32), np.asarray(g["poses"], np.float32).view(np.uint32))
        assert np.array_equal(np.asarray(r["poses64"]).view(np.uint64), np.asarray(g["poses"], np.float32).astype(np.float64).view(np.uint64))
        assert np.array_equal(r["edge_chi2"][0], r["edge_chi2"][1], equal_nan=True) and (r["chi2_final"] == r["chi2_initial"] or key[0] == "nan")
        return
    pc.compare(str(key[:2]), r, m, g)
    completed = r["gn_iterations"]
    assert r["pcg_iterations"] == ((1 + REFINE) * completed if n_ends else completed)
    if key[0] == "cap":
        assert r["status"] == pgm.ITERATION_CAP and r["gn_iterations"] == 1
    if key[0] == "stalled":
        assert r["status"] == pgm.STALLED and r["gn_iterations"] == 2
    if key[0] == "strong":
        assert r["status"] == pgm.CONVERGED and r["gn_iterations"] == 3


# ---- the hook's file (tests/cpp/test_posegraph_direct.cpp, `step` mode) ----------------------------------------------------------------------------------------
DIRECT_ARRAYS = ("D", "B", "A", "g", "Z", "Wm", "L", "Ks", "Lk", "x0", "x", "Pt", "chi_trial", "q")


def read_direct_steps(path, items):
    """The output file of the `step` mode, one dict per graph with the keys of Context.debug_pose_graph_direct.  items: [(graph, options, p)]."""
    raw = open(path, "rb").read()
    pos, out = 0, []
    for g, _, p in items:
        n, C = g["poses"].shape[0], len(g["closures"])
        E, K = n - 1 + C, np.asarray(p).reshape(-1, n, 6).shape[0]
        hd = struct.unpack_from("<8i", raw, pos); pos += 32
        r = dict(zip(("m", "factor_status", "wm_status", "ks_status", "band_solves", "trial"), hd))
        r.update(zip(("chi2_start", "chi2_trial", "max_dx"), struct.unpack_from("<ddd", raw, pos))); pos += 24
        m = r["m"]; q = 6 * m
        r["ends"] = np.frombuffer(raw, np.int32, m, pos).copy(); pos += 4 * m
        shapes = dict(D=(n, 6, 6), B=(n, 6, 6), A=(C, 6, 6), g=(n, 6), Z=(6 * n, q), Wm=(q, q), L=(q, q), Ks=(q, q), Lk=(q, q), x0=(n, 6), x=(n, 6), Pt=(n, 12),
                      chi_trial=(E,), q=(K, n, 6))
        for k in DIRECT_ARRAYS:
            cnt = int(np.prod(shapes[k]))
            r[k] = np.frombuffer(raw, np.float64, cnt, pos).reshape(shapes[k]); pos += 8 * cnt
        out.append(r)
    assert pos == len(raw)
    return out
