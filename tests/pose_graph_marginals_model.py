"""The pose graph's MARGINAL COVARIANCES restated in float64 NumPy (DESIGN.md section 20 "Marginal covariances"): the block factor of the band, the backward
recurrence for the diagonal blocks of its inverse, P = Z L^-T and Q = P Lk^-T; two dense references (numpy.linalg.inv, and the inverse through a Cholesky
factor); the scaled measure; the graphs, the file format of tests/cpp/test_posegraph_marginals.cpp and the checks that tests/test_pose_graph_marginals_host.py
runs on the host build's output and tests/test_pose_graph_marginals.py on the device's.  Nothing here is shared with the device code.

THE MEASURE.  scaled(S, R) = max over the free nodes k and the entries a, b of |S_k - R_k|_ab / sqrt(R_k,aa R_k,bb): an error of a covariance in units of the
standard deviations it is about.
THE BOUNDS.  own(X) is the scaled distance between the two NumPy references on the matrix X that a check inverts.  (a), (b), (e) allow 10 x own (the margin
tests/test_pose_graph_direct_step.py gives x); (c), against the model's H, allows 10 x own + 4 x the scaled difference between the model's covariance from its
float64 Jacobians and from pgm.jacobians_ld (the noise of the central differences, which the device's Jacobians carry too).  No bound may exceed CAP."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_direct_model as pdm      # noqa: E402
import pose_graph_model as pgm      # noqa: E402

ROOT = pdm.ROOT
CAP = 1e-6          # a standard deviation known to one part in a million
MARGIN = 10


# ---- the graphs ------------------------------------------------------------------------------------------------------------------------------------------------
ENDS128_PAIRS = tuple((k, k + 70) for k in range(1, 65))


def ends128_graph():
    """140 poses, 64 closures with 128 distinct ends: q = 768, the limit itself."""
    return dict(pgm.make_loop(140, list(ENDS128_PAIRS), seed=11), fixed=None)


def chain65_graph():
    return dict(pgm.make_loop(65, [], seed=11), fixed=None)


@functools.lru_cache(maxsize=None)
def graphs():
    """name -> graph."""
    out = {}
    out["n1"] = dict(pgm.make_loop(1, [], seed=11), fixed=None)
    out["n2"] = pc.graph(2, pc.CASES[1][1], None, True)
    out["n3"] = pc.graph(3, pc.CASES[2][1], None, True)
    out["n6"] = pc.graph(*pc.CASES[3], True)
    out["n33"] = pc.graph(*pc.CASES[4], True)
    out["n65"] = pc.graph(*pc.CASES[5], True)
    out["chain65"] = chain65_graph()
    out["m0"] = pdm.m0_graph()
    out["rank5"] = pc.rank5_graph()
    out["strong"] = pc.strong_graph()
    out["ends288"] = pdm.ends288_graph()
    out["ends128"] = ends128_graph()
    out["n257"] = pc.graph(*pc.CASES[6], True)
    return out


def chain_of(g):
    """The same poses and odometry without the closures."""
    return dict(g, closures=[])


FAILING = {"negative": (lambda: pc.negative_graph(1.0), pgm.NOT_POSITIVE_DEFINITE, "factor_status"),
           "negative_ks": (lambda: pc.negative_graph(0.1), pgm.NOT_POSITIVE_DEFINITE, "ks_status"),
           "nan": (pc.nan_graph, pgm.NON_FINITE, "factor_status")}


# ---- the NumPy restatement -------------------------------------------------------------------------------------------------------------------------------------
def block_factor(D, B):
    """The band's block Cholesky factor: G n x 6 x 6 lower triangular (its true diagonal), W n x 6 x 6 with W[k] = B[k] G[k-1]^-T."""
    D, B = np.asarray(D, np.float64).reshape(-1, 6, 6), np.asarray(B, np.float64).reshape(-1, 6, 6)
    n = D.shape[0]
    G, W = np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    for k in range(n):
        if k > 0:
            W[k] = np.linalg.solve(G[k - 1], B[k].T).T
        G[k] = np.linalg.cholesky(D[k] - W[k] @ W[k].T)
    return G, W


def band_selinv(G, W, skip_term_at=None, transpose_y=False):
    """The diagonal blocks of M^-1 by the backward recurrence.  skip_term_at / transpose_y: the corruptions of test_the_checks_bite."""
    n = G.shape[0]
    S = np.zeros((n, 6, 6))
    for k in range(n - 1, -1, -1):
        Gi = np.linalg.inv(G[k])
        S[k] = Gi.T @ Gi
        if k + 1 < n and k != skip_term_at:
            Y = W[k + 1] @ Gi
            if transpose_y:
                Y = Y.T
            S[k] = S[k] + Y.T @ S[k + 1] @ Y
    return S


def restate(D, B, A, edges, is_fixed, drop_qq=False, skip_end=None, **kw):
    """dict(band_cov n x 6 x 6, cov n x 6 x 6 (zero at fixed nodes)) from the device's D, B, A: H^-1 = M^-1 - P P^T + Q Q^T."""
    D = np.asarray(D, np.float64).reshape(-1, 6, 6)
    n = D.shape[0]
    is_fixed = np.asarray(is_fixed, bool)
    G, W = block_factor(D, B)
    band = band_selinv(G, W, **kw)
    cov = band.copy()
    ends = pdm.ends_of(n, edges[n - 1:], is_fixed)
    if ends:
        q = 6 * len(ends)
        M = pdm.dense_band(D, B)
        U = np.zeros((6 * n, q))
        for a, k in enumerate(ends):
            U[6 * k:6 * k + 6, 6 * a:6 * a + 6] = np.eye(6)
        S = pdm.s_matrix(A, edges, ends, is_fixed, n)
        Z = pgm.band_solver(M, cholesky=True)(U)
        Wm = pdm._mirror(U.T @ Z)
        L = np.linalg.cholesky(Wm)
        Lk = np.linalg.cholesky(pdm._mirror(np.eye(q) + L.T @ (S @ L)))
        P = np.linalg.solve(L, Z.T).T
        Q = np.linalg.solve(Lk, P.T).T
        if skip_end is not None:          # (the corruption: the two products pass over one end node's six columns)
            P[:, 6 * skip_end:6 * skip_end + 6] = 0; Q[:, 6 * skip_end:6 * skip_end + 6] = 0
        for k in range(n):
            Pk, Qk = P[6 * k:6 * k + 6], Q[6 * k:6 * k + 6]
            cov[k] = band[k] - Pk @ Pk.T + (0 if drop_qq else Qk @ Qk.T)
    cov[is_fixed] = 0
    return dict(band_cov=band, cov=cov)


# ---- the references and the measure ----------------------------------------------------------------------------------------------------------------------------
def diag_blocks(X):
    m = X.shape[0] // 6
    return np.stack([X[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(m)]) if m else np.zeros((0, 6, 6))


def inv_blocks(X):
    """The diagonal blocks of numpy.linalg.inv(X)."""
    return diag_blocks(np.linalg.inv(X))


def chol_inv_blocks(X):
    """The diagonal blocks of X^-1 through its Cholesky factor: X = C C^T, X^-1 = C^-T C^-1."""
    Ci = np.linalg.solve(np.linalg.cholesky(X), np.eye(X.shape[0]))
    return diag_blocks(Ci.T @ Ci)


def scaled(S, R):
    """max |S - R|_ab / sqrt(R_aa R_bb) over the blocks (each k x 6 x 6)."""
    S, R = np.asarray(S, np.float64).reshape(-1, 6, 6), np.asarray(R, np.float64).reshape(-1, 6, 6)
    if R.shape[0] == 0:
        return 0.0
    d = np.sqrt(np.einsum("kaa->ka", R))
    return float((np.abs(S - R) / (d[:, :, None] * d[:, None, :])).max())


def own(X):
    """The scaled distance between the two NumPy references on X, and the first of them."""
    R = inv_blocks(X)
    return scaled(chol_inv_blocks(X), R), R


def model_H(g, ld=False):
    """The model's dense H over the free nodes at the graph's float32 poses, damping 0: pgm.linearise's sum, the Jacobians in float64 or (ld) pgm.jacobians_ld."""
    n = g["poses"].shape[0]
    closures = list(g["closures"])
    edges = pgm.edge_list(n, closures)
    X, info = pgm._measurements(n, g["odo_X"], g["odo_info"], closures)
    is_fixed = pgm.fixed_mask(n, g["fixed"])
    T = np.asarray(g["poses"], np.float32).reshape(n, 4, 4).astype(np.float64)
    if not ld:
        return pgm.linearise(T, edges, X, info, is_fixed)[2]
    free = np.nonzero(~is_fixed)[0]
    col = -np.ones(n, int); col[free] = np.arange(free.size)
    H = np.zeros((6 * free.size, 6 * free.size))
    for q, (i, j) in enumerate(edges):
        J = np.asarray(pgm.jacobians_ld(T[i], T[j]), np.float64)
        for (a, Ja) in ((i, J[:, :6]), (j, J[:, 6:])):
            for (b, Jb) in ((i, J[:, :6]), (j, J[:, 6:])):
                if col[a] >= 0 and col[b] >= 0:
                    H[6 * col[a]:6 * col[a] + 6, 6 * col[b]:6 * col[b] + 6] += Ja.T @ info[q] @ Jb
    return H


_MODEL = {}


def model_ref(name, g):
    """(the model's covariance blocks over the free nodes, own of the model's H, the Jacobian term), once per process and name."""
    if name not in _MODEL:
        H = model_H(g)
        o, R = own(H) if H.size else (0.0, np.zeros((0, 6, 6)))
        jac = scaled(inv_blocks(model_H(g, ld=True)), R) if H.size else 0.0
        _MODEL[name] = (R, o, jac)
    return _MODEL[name]


# ---- the checks, on a result r = dict(status, m, ends, D, B, A, band_cov, cov) ----------------------------------------------------------------------------------
def context(name, g, r):
    n = g["poses"].shape[0]
    is_fixed = pgm.fixed_mask(n, g["fixed"])
    return dict(name=name, g=g, n=n, edges=pgm.edge_list(n, g["closures"]), is_fixed=is_fixed, free=np.nonzero(~is_fixed)[0])


def check_status(r, m):
    assert r["status"] == 0 and r["factor_status"] == 0 and r["wm_status"] == 0 and r["ks_status"] == 0
    ends = pdm.ends_of(m["n"], m["g"]["closures"], m["is_fixed"])
    assert r["m"] == len(ends) and list(r["ends"]) == ends


def check_a(r, m):
    """band_cov against the diagonal blocks of the inverse of dense_band(D, B) (the run's own), every node: a fixed node carries the identity."""
    o, R = own(pdm.dense_band(r["D"], r["B"]))
    d = scaled(r["band_cov"], R)
    print("  (a) %s: band_cov is %.3e from inv(M) in the scaled measure; the two NumPy references are %.3e apart (bound %.3e)" % (m["name"], d, o, MARGIN * o))
    assert MARGIN * o <= CAP and d <= MARGIN * o
    return dict(a=d, a_own=o)


def check_b(r, m):
    """cov against the diagonal blocks of the inverse of dense_from_band(D, B, A), the free nodes.  Returns the bound too."""
    if m["free"].size == 0:
        return dict(b=0.0, b_own=0.0, b_bound=0.0)
    o, R = own(pgm.dense_from_band(r["D"], r["B"], r["A"], m["edges"], m["is_fixed"]))
    d = scaled(r["cov"][m["free"]], R)
    print("  (b) %s: cov is %.3e from inv(H) of its own D, B, A; the two NumPy references are %.3e apart (bound %.3e)" % (m["name"], d, o, MARGIN * o))
    assert MARGIN * o <= CAP and d <= MARGIN * o
    return dict(b=d, b_own=o, b_bound=MARGIN * o)


def check_c(cov, m):
    """cov against the model's H (pgm.linearise at the same poses)."""
    if m["free"].size == 0:
        return dict(c=0.0)
    R, o, jac = model_ref(m["name"], m["g"])
    d = scaled(np.asarray(cov)[m["free"]], R)
    bound = MARGIN * o + 4 * jac
    print("  (c) %s: cov is %.3e from the model's; references %.3e apart, Jacobian term %.3e (bound %.3e)" % (m["name"], d, o, jac, bound))
    assert bound <= CAP and d <= bound
    return dict(c=d, c_own=o, c_jac=jac)


def check_d(cov, m):
    """Every block bitwise symmetric; the smallest eigenvalue of every free block positive; fixed blocks exactly zero."""
    cov = np.ascontiguousarray(np.asarray(cov, np.float64).reshape(-1, 6, 6))
    assert np.array_equal(cov.view(np.uint64), np.ascontiguousarray(cov.transpose(0, 2, 1)).view(np.uint64))
    assert not cov[m["is_fixed"]].any() and not np.signbit(cov[m["is_fixed"]]).any()
    if m["free"].size:
        lam = np.linalg.eigvalsh(cov[m["free"]])[:, 0]
        print("  (d) %s: the smallest eigenvalue of a free block is %.3e" % (m["name"], lam.min()))
        assert (lam > 0).all()


def check_e(cov, cov_chain, m, bound_b):
    """Order: information only adds, so Sigma_with <= Sigma_chain.  Each side stands entrywise within bound |.|_ab <= bound sqrt(S_aa S_bb) of its true
    value (check (b)), an error matrix whose largest eigenvalue is at most its Frobenius norm <= bound x trace(S): lambda_max(Sigma_with - Sigma_chain) per node
    is at most bound x trace(Sigma_chain)."""
    cov, cov_chain = np.asarray(cov).reshape(-1, 6, 6)[m["free"]], np.asarray(cov_chain).reshape(-1, 6, 6)[m["free"]]
    if cov.shape[0] == 0:
        return dict(e=0.0)
    lam = np.linalg.eigvalsh(cov - cov_chain)[:, -1]
    scale = np.einsum("kaa->k", cov_chain)
    worst = float((lam / scale).max())
    print("  (e) %s: lambda_max(cov - cov of the chain) / trace is at most %.3e (bound %.3e)" % (m["name"], worst, bound_b))
    assert (lam <= bound_b * scale).all()
    return dict(e=worst)


def check_failed(r, g, status, which):
    """After a failure: the status, every free node's block quiet NaN, every fixed node's zero."""
    is_fixed = pgm.fixed_mask(g["poses"].shape[0], g["fixed"])
    cov = np.asarray(r["cov"]).reshape(-1, 6, 6)
    assert r["status"] == status and r[which] == status, (r["status"], r["factor_status"], r["wm_status"], r["ks_status"])
    assert np.isnan(cov[~is_fixed]).all() and not cov[is_fixed].any()
    assert (cov[~is_fixed].view(np.uint64) == np.uint64(0x7ff8000000000000)).all()


# ---- the host build (tests/cpp/test_posegraph_marginals.cpp) ----------------------------------------------------------------------------------------------------
def build_and_run(tmp, fin, builds=pdm.BUILDS, mode=()):
    """The program built the ways of `builds` and run on the file fin: the outputs must be the same bytes, the sanitised runs must end clean.  Returns the path
    of the plain build's output."""
    src = os.path.join(ROOT, "tests", "cpp", "test_posegraph_marginals.cpp")
    outs = {}
    for name, flags in builds:
        exe = str(tmp / ("test_posegraph_marginals_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", ROOT, src, "-o", exe])
        fout = str(tmp / (name + ".bin"))
        r = subprocess.run([exe, *mode, fin, fout], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "ERROR" not in r.stderr, (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        outs[name] = open(fout, "rb").read()
        if name == "plain":
            print(r.stdout)
    assert all(v == outs["plain"] for v in outs.values())
    return str(tmp / "plain.bin")


def read_marginals(path, gs):
    """The program's output file, one dict per graph with the keys of Context.debug_pose_graph_marginals."""
    raw = open(path, "rb").read()
    pos, out = 0, []
    for g in gs:
        n, C = g["poses"].shape[0], len(g["closures"])
        hd = struct.unpack_from("<6i", raw, pos); pos += 24
        r = dict(zip(("status", "m", "factor_status", "wm_status", "ks_status"), hd))
        r["ends"] = np.frombuffer(raw, np.int32, r["m"], pos).copy(); pos += 4 * r["m"]
        for k, rows in (("D", n), ("B", n), ("A", C), ("band_cov", n), ("cov", n)):
            r[k] = np.frombuffer(raw, np.float64, rows * 36, pos).reshape(rows, 6, 6); pos += 288 * rows
        out.append(r)
    assert pos == len(raw)
    return out


def host_run(tmp, names, builds=pdm.BUILDS):
    """name -> result for the named graphs, their chains (name + "_chain" where the graph has closures) and the failing graphs, through the host build."""
    items = []
    for k in names:
        g = graphs()[k] if k in graphs() else FAILING[k][0]()
        items.append((k, g))
        if k in graphs() and g["closures"]:
            items.append((k + "_chain", chain_of(g)))
    fin = str(tmp / "graphs.bin")
    pc.write_graphs(fin, [(g, {}) for _, g in items])
    res = read_marginals(build_and_run(tmp, fin, builds), [g for _, g in items])
    return {k: r for (k, _), r in zip(items, res)}


def host_run_blocks(tmp, items):
    """items: [(graph, D, B, A)], a device's own blocks.  The plain host build from the band's factor on (`blocks` mode), one result per item."""
    fin = str(tmp / "blocks.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(items)))
        for g, D, B, A in items:
            pc._write_graph(f, g, {})
            for v in (D, B, A):
                f.write(np.ascontiguousarray(v, np.float64).tobytes())
    return read_marginals(build_and_run(tmp, fin, pdm.BUILDS[:1], ("blocks",)), [g for g, _, _, _ in items])
