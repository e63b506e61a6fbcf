"""ONE Gauss-Newton step with the pose-graph optimiser's DIRECT solve taken apart (DESIGN.md section 20 "The direct solve"): the hook icet_debug_pose_graph_direct
runs the optimiser's first iteration -- the production kernels in the production order -- and copies out the end nodes, D, B, A, g, Z = M^-1 U, Wm = U^T Z and its
factor L, Ks = I + L^T S L and its factor Lk, x0 (before the refinement), x, the trial poses.  Each comparison runs twice: on the CPU, on what the host build of the
same driver and bodies returns (tests/cpp/test_posegraph_direct.cpp, `step` mode: plain, sanitised and as four threads, the same bytes), and on the GPU (marked gpu).

eps = 2^-53, gamma(m) = m eps / (1 - m eps).  Everything is measured against the device's OWN D, B, A, g (tests/test_pose_graph_step.py pins those to the model):
 (a) ends is the model's list (pdm.ends_of), m its length.
 (b) Z: every column stands, in the M-norm and relative to its own M-norm, within 10 x the distance between two NumPy band solves of the same M (LU and
     Cholesky: pgm.band_solver), the pattern of section 20 (e).  That distance is ONE figure per graph, the largest relative M-norm distance of a column: taken
     per column it is no yardstick, because the two NumPy solves agree on single columns a thousand times better than on their neighbours (strong: 2e-24 beside
     1e-20), by chance.  A column's right-hand side is zero before its own node: the rows of M Z before that node are zero to within 10 x what the two NumPy solves
     leave there, or the rounding of evaluating M Z itself (gamma(18) |M||Z|, 18 products per row), whichever is larger.
 (c) Wm and Ks are bitwise symmetric.  Ks against I + L^T S L formed in numpy.longdouble from the returned L and A: entrywise within gamma(q + 12) (I + |L^T||S||L|)
     (a dot product of length <= q behind one of <= 12 products per incidence item, and the identity's addition; |S| from |A|).  L L^T against Wm and Lk Lk^T
     against Ks entrywise within gamma(q + 1) |L||L^T|: Cholesky's backward error bound.
 (d) x0 and x against numpy.linalg.solve(dense_from_band(D, B, A), -g), relative in the H-norm: each within 10 x the error of pdm.direct_solve (the same
     algorithm in NumPy, another summation order) on the same arrays; direct_solve's own error must be below 1e-9 (a condition on the reference).  The dense
     solve is polished by two steps of iterative refinement with its residual in numpy.longdouble, so that its own error (which is exactly direct_solve's on a
     graph without end nodes: the same LAPACK call, an "error" of 0) does not stand in for either side's.
 (e) the residual |H x + g| / |g| of x is at most twice that of x0.
 (f) the trial poses against T exp_se3(x): check (g) of tests/test_pose_graph_step.py, 20 eps; fixed nodes bit for bit.  q = H p: its check (d).
test_the_checks_bite corrupts a correct host result four ways and expects the named check to fail."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_direct_model as pdm      # noqa: E402
import pose_graph_model as pgm      # noqa: E402
import test_pose_graph_step as tps      # noqa: E402

EPS = 2.0 ** -53
LD = np.longdouble


def gamma(m):
    return m * EPS / (1 - m * EPS)


def graphs():
    """name -> graph, options: pc.step_graphs() (strong100 is strong with an option the direct solve does not read), ends288 and a graph without end nodes."""
    out = {k: v for k, v in pc.step_graphs().items() if k != "strong100"}
    out["ends288"] = (pdm.ends288_graph(), {})
    out["m0"] = (pdm.m0_graph(), {})
    return out


NAMES = list(graphs())


def p_vector(name):
    g, _ = graphs()[name]
    return np.random.default_rng(5).standard_normal((1, g["poses"].shape[0], 6))


_REF = {}


def ref(name, r):
    """What the checks need beside the hook's result r, from r's own D, B, A, g (cached per name and source)."""
    key = (name, id(r))
    if key in _REF:
        return _REF[key]
    g, o = graphs()[name]
    n = g["poses"].shape[0]
    edges = pgm.edge_list(n, g["closures"])
    is_fixed = pgm.fixed_mask(n, g["fixed"])
    free = np.nonzero(~is_fixed)[0]
    Hd = pgm.dense_from_band(r["D"], r["B"], r["A"], edges, is_fixed)
    gd = r["g"][free].reshape(-1)
    xstar = np.linalg.solve(Hd, -gd)
    for _ in range(2):
        xstar = xstar + np.linalg.solve(Hd, (-gd.astype(LD) - Hd.astype(LD) @ xstar.astype(LD)).astype(np.float64))
    m = dict(name=name, g=g, n=n, edges=edges, is_fixed=is_fixed, free=free, Hd=Hd, gd=gd, xstar=xstar,
             T=np.asarray(g["poses"], np.float32).reshape(n, 4, 4).astype(np.float64), ends=pdm.ends_of(n, g["closures"], is_fixed),
             ds=pdm.direct_solve(r["D"], r["B"], r["A"], r["g"], edges, is_fixed))
    _REF[key] = m
    return m


def check_a(r, m):
    print("  (a) %s: %d end nodes" % (m["name"], r["m"]))
    assert r["m"] == len(m["ends"]) and list(r["ends"]) == m["ends"]
    assert r["factor_status"] == 0 and r["wm_status"] == 0 and r["ks_status"] == 0 and r["trial"] == 1
    assert r["band_solves"] == (1 + pdm.REFINE if m["ends"] else 1)


def _mnorm(M, E):
    return np.sqrt(np.maximum(np.einsum("ij,ij->j", E, M @ E), 0.0))


def check_b(r, m):
    if not m["ends"]:
        assert r["Z"].size == 0
        return {}
    M = m["ds"]["M"]
    q = 6 * len(m["ends"])
    U = np.zeros((M.shape[0], q))
    for a, k in enumerate(m["ends"]):
        U[6 * k:6 * k + 6, 6 * a:6 * a + 6] = np.eye(6)
    Zl, Zc = pgm.band_solver(M)(U), pgm.band_solver(M, cholesky=True)(U)
    size = _mnorm(M, Zl)
    own, off = float((_mnorm(M, Zl - Zc) / size).max()), _mnorm(M, r["Z"] - Zl) / size
    # the rows before the column's node: a zero right-hand side
    before = np.arange(M.shape[0])[:, None] < 6 * np.repeat(m["ends"], 6)[None, :]
    Rd, Rl, Rc = (np.where(before, np.abs(M @ Z - U), 0.0).max(axis=0) for Z in (r["Z"], Zl, Zc))
    floor = np.where(before, gamma(18) * (np.abs(M) @ np.abs(r["Z"])), 0.0).max(axis=0)
    allowed = np.maximum(10 * np.maximum(Rl, Rc), floor)
    fig = dict(z_own=own, z_of_own=float(off.max() / own), z_before=float((Rd / np.maximum(allowed, 1e-300)).max()))
    print("  (b) %s: a column of Z is at most %.3f of the distance between two NumPy band solves (%.3e of a column's M-norm) from one of them (bound 10); M Z before the column's node: %.3f of what is allowed"
          % (m["name"], fig["z_of_own"], own, fig["z_before"]))
    assert own > 0 and (off <= 10 * own).all()
    assert (Rd <= allowed).all()
    assert not r["Z"][np.repeat(m["is_fixed"], 6)].any()
    return fig


def check_c(r, m):
    if not m["ends"]:
        return {}
    q = 6 * len(m["ends"])
    Wm, L, Ks, Lk = r["Wm"], r["L"], r["Ks"], r["Lk"]
    for X in (Wm, Ks):
        assert np.array_equal(X.view(np.uint64), X.T.copy().view(np.uint64))
    assert not np.triu(L, 1).any() and not np.triu(Lk, 1).any()
    S = pdm.s_matrix(r["A"], m["edges"], m["ends"], m["is_fixed"], m["n"], LD)
    Sa = pdm.s_matrix(np.abs(r["A"]), m["edges"], m["ends"], m["is_fixed"], m["n"], LD)
    Ll = L.astype(LD)
    dK = np.abs(Ks - (np.eye(q, dtype=LD) + Ll.T @ S @ Ll))
    bK = gamma(q + 12) * (np.eye(q, dtype=LD) + np.abs(Ll.T) @ Sa @ np.abs(Ll))
    dW = np.abs(Wm - Ll @ Ll.T); bW = gamma(q + 1) * (np.abs(Ll) @ np.abs(Ll.T))
    Lkl = Lk.astype(LD)
    dF = np.abs(Ks - Lkl @ Lkl.T); bF = gamma(q + 1) * (np.abs(Lkl) @ np.abs(Lkl.T))
    def of_bound(d, b):          # (a bound of exactly zero: the entry is a sum of exact zeros)
        return float((d[b > 0] / b[b > 0]).max())
    fig = dict(ks_of_bound=of_bound(dK, bK), llt_of_bound=of_bound(dW, bW), lklkt_of_bound=of_bound(dF, bF))
    print("  (c) %s: Ks is at most %.3f of its bound from I + L^T S L, L L^T %.3f of its bound from Wm, Lk Lk^T %.3f from Ks" % (m["name"], fig["ks_of_bound"], fig["llt_of_bound"], fig["lklkt_of_bound"]))
    assert (dK <= bK).all() and (dW <= bW).all() and (dF <= bF).all()
    return fig


def h_err(m, x):
    """|x - x*|_H / |x*|_H over the free nodes."""
    e = np.asarray(x)[m["free"]].reshape(-1) - m["xstar"]
    return float(np.sqrt(e @ m["Hd"] @ e) / np.sqrt(m["xstar"] @ m["Hd"] @ m["xstar"]))


def check_d(r, m):
    own0, own = h_err(m, m["ds"]["x0"]), h_err(m, m["ds"]["x"])
    e0, e = h_err(m, r["x0"]), h_err(m, r["x"])
    fig = dict(x0_err=e0, x_err=e, ref_x0_err=own0, ref_x_err=own)
    print("  (d) %s: x0 is %.3e of the dense solve off in the H-norm (NumPy's direct solve: %.3e, ratio %.2f), x %.3e (%.3e, ratio %.2f)"
          % (m["name"], e0, own0, e0 / own0 if own0 else 0.0, e, own, e / own if own else 0.0))
    assert m["ds"]["status"] == 0 and own0 < 1e-9 and own < 1e-9
    assert e0 <= 10 * own0 and e <= 10 * own
    assert not r["x"][m["is_fixed"]].any() and not r["x0"][m["is_fixed"]].any()
    return fig


def resid(m, x):
    xv = np.asarray(x)[m["free"]].reshape(-1)
    return float(np.linalg.norm(m["Hd"] @ xv + m["gd"]) / np.linalg.norm(m["gd"]))


def check_e(r, m):
    r0, r1 = resid(m, r["x0"]), resid(m, r["x"])
    print("  (e) %s: |H x + g| / |g| is %.3e before the refinement, %.3e behind it" % (m["name"], r0, r1))
    assert r1 <= 2 * r0
    return dict(resid_x0=r0, resid_x=r1)


def check_f(r, m, p):
    tps.check_g(r, m)
    tps.check_d(r, m, p)
    return {}


def check_all(r, m, p):
    fig = {}
    check_a(r, m)
    for f in (check_b, check_c, check_d, check_e):
        fig.update(f(r, m))
    check_f(r, m, p)
    return fig


# ---- CPU: the host build of the hook -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pg_direct_step")
    items = [(graphs()[k][0], graphs()[k][1], p_vector(k)) for k in NAMES]
    fin = str(tmp / "graphs.bin")
    pc.write_step_graphs(fin, items)
    return dict(zip(NAMES, pdm.read_direct_steps(pdm.build_and_run(tmp, fin, ("step",)), items)))


@pytest.mark.parametrize("name", NAMES)
def test_host_direct_step(host, name):
    r = host[name]
    check_all(r, ref(name, r), p_vector(name))


def test_the_named_graphs():
    assert len(pdm.graph_ends(graphs()["ends288"][0])) == 96 and pdm.graph_ends(graphs()["m0"][0]) == []
    assert pdm.graph_ends(graphs()["n2"][0]) == [] and pdm.graph_ends(graphs()["n3"][0]) == []


def _copy(r):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def test_the_checks_bite(host):
    """Four corruptions of a correct host result, pure NumPy: each fails the check it names (and the result it was made from passes it)."""
    # the A^T side of a reversed closure taken as A: Ks from such an S.  (On n65, closure (40, 8): on n6 the fixed node 4 cuts the chain between the reversed
    # closure's ends, L has no block between them, and the corrupted side never reaches the triangle of Ks that is computed.)
    r = host["n65"]; m = ref("n65", r)
    check_c(r, m)
    n, ends, q = m["n"], m["ends"], 6 * len(m["ends"])
    end_of = {k: a for a, k in enumerate(ends)}
    c, (i, j) = next((c, e) for c, e in enumerate(m["edges"][n - 1:]) if e[0] - e[1] >= 2 and not m["is_fixed"][e[0]] and not m["is_fixed"][e[1]])
    S = pdm.s_matrix(r["A"], m["edges"], ends, m["is_fixed"], n)
    a, b = end_of[i], end_of[j]
    S[6 * b:6 * b + 6, 6 * a:6 * a + 6] += r["A"][c] - r["A"][c].T
    bad = _copy(r); bad["Ks"] = pdm._mirror(np.eye(q) + r["L"].T @ (S @ r["L"]))
    with pytest.raises(AssertionError):
        check_c(bad, m)
    r = host["n6"]; m = ref("n6", r)
    check_a(r, m); check_c(r, m)
    ends = m["ends"]
    # one end dropped
    bad = _copy(r); bad["ends"] = r["ends"][:-1]; bad["m"] = r["m"] - 1
    with pytest.raises(AssertionError):
        check_a(bad, m)
    # a row of Wm gathered from the neighbouring node
    rows = np.concatenate([6 * k + np.arange(6) for k in ends])
    rows[:6] += 6
    bad = _copy(r); bad["Wm"] = pdm._mirror(r["Z"][rows])
    with pytest.raises(AssertionError):
        check_c(bad, m)
    # the refinement added with the wrong sign, where the refinement matters: the strong closures
    r = host["strong"]; m = ref("strong", r)
    fig = check_d(r, m)
    bad = _copy(r); bad["x"] = r["x0"] - (r["x"] - r["x0"])
    assert h_err(m, bad["x"]) > 10 * fig["ref_x_err"]
    with pytest.raises(AssertionError):
        check_d(bad, m)


# ---- GPU: the same checks through the hook -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import icet_amd
    c = icet_amd.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_direct_step(ctx, name):
    """Measured on an MI355X: DESIGN.md section 20 has the table."""
    g, o = graphs()[name]
    r = ctx.debug_pose_graph_direct(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], damping=o.get("damping", 0.0), p=p_vector(name))
    check_all(r, ref(name, r), p_vector(name))
    # the hook is the optimiser's first iteration: gn_iters = 1 with the direct solve returns its trial poses and its band solves
    w = ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], gn_iters=1, damping=o.get("damping", 0.0), solver="direct")
    assert r["chi2_trial"] < r["chi2_start"] and w["solver"] == 1
    assert w["pcg_iterations"] == r["band_solves"] and w["chi2_initial"] == r["chi2_start"] and w["chi2_final"] == r["chi2_trial"] and w["max_dx"] == r["max_dx"]
    assert np.array_equal(w["poses64"].view(np.uint64), pc.poses64_matrix(r["Pt"]).view(np.uint64))
