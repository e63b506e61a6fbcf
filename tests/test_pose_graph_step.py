"""ONE Gauss-Newton step of the pose-graph optimiser taken apart: the hook icet_debug_pose_graph_step runs the optimiser's first
iteration -- the production kernels in the production order, the production CG loop -- and copies out what a run to convergence heals by itself: the residuals,
the Jacobians, the band D, B and the off-band blocks A, g, the products q = H p, the CG scalars, x and the trial poses.  Every array is compared with the
dense NumPy model of tests/pose_graph_model.py under a bound that is derived below, not fitted.  Each comparison runs twice: on the CPU, on what the host build
of the same driver and bodies returns (tests/cpp/test_posegraph_optimize.cpp, `step` mode: plain, sanitised and as four threads, the same bytes), and on the
GPU (marked gpu) through the hook.  test_the_checks_bite corrupts a correct host result six ways and expects the named check to fail.

eps = 2^-53, gamma(m) = m eps / (1 - m eps).  The checks, all entrywise unless said otherwise:
 (a) res, chi: x_t = R_j^T (t_j - t_i) is a difference and a 3-term dot product: gamma(4) sum |R_j||t_j - t_i| per side.  An angle is atan2 / asin of entries of
     R_j^T R_i (3-term dot products: gamma(3) sum |R_j||R_i| each) -- the error of the entries over the distance r of (y, x) from the origin (cos(theta) for all
     three), plus 2 ulps of the angle for the library function.  Twice that for the two sides, and 4 eps (|xof| + |X|) for the subtraction and the wrap of
     each; the model's own wrap adds 4 eps to an angle (it rounds twice at the size of pi).  chi = e^T Omega e: 2 |e|^T |Omega| de + de^T |Omega| de + 2 gamma(13) |e|^T |Omega| |e|.
 (b) J: both sides are the same central differences; their rounding noise (about eps |xof| / 2 h) is independent.  The model's float64 Jacobian is measured
     against its numpy.longdouble twin on the graph; dJ = 4 x the largest entry of that difference, and dJ may not exceed 1e-6 of the largest entry of any edge's J.
 (c) H, g: per block sum over the edges of |J_a|^T |Omega| dJ + dJ^T |Omega| |J_b| + dJ^T |Omega| dJ, plus 2 gamma(m) sum |J_a|^T |Omega| |J_b| for the
     sums (m = 14 + the longest incidence list: 6 + 6 products, the edges, the damping); g alike with de of (a).  D bitwise symmetric.
 (d) q: against dense_from_band(D, B, A) @ p, the reference in longdouble so that the bound is the device's alone: gamma(m) |H||p|, m = 6 x the blocks the row
     walks.  A fixed node's row is p's, bit for bit.
 (e) the solve: x replayed in NumPy from the returned D, B, A, g with alpha = r.z / p.Hp and beta = r.z / the previous r.z taken from the returned scalars
     must agree with the returned x to better than HALF its last step, in the H-norm (a run stopped one iteration early is off by exactly one step), or, where
     the recurrence itself is less reproducible than that (it amplifies rounding by cond(M^-1 H) once the directions lose their orthogonality: the strong
     closures), to within 10 x the distance between two NumPy replays that differ only in their float64 band solver; the ending reason must match the scalars; ended by tolerance, the true preconditioned residual ratio
     against the model's H, g and band is at most 10 x max(pcg_tol, the reference CG's own ratio); band solves <= the reference's steps + 2 (one band solve
     behind the last step finds the end).
 (f) x against numpy.linalg.solve(H, -g) of the model, relative in the H-norm: the ratio bound of (e) x sqrt(cond(M^-1 H)).
 (g) Pt against T exp_se3(x) of the model at the returned x: Exp's entries carry about 6 eps (sin, cos, the divisions), the 3-term products gamma(3), both
     sides: 20 eps |R||Exp| for R, 20 eps (|t| + |R||V rho|) for t.  Fixed nodes bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_model as pgm      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
PCG_TOL = 1e-10          # the driver's default
TOL, ZERO, CAP, FAILED = 0, 1, 2, 3          # icet_pose_graph_step.cg_end
NAMES = list(pc.step_graphs())
EQUAL_INFORMATION = [k for k in NAMES if not k.startswith("strong")]
# The equal-information graphs on which the reference CG itself ends within the exact-arithmetic 12 c_offband + 1 steps; it takes one step more on n65 (38) and
# on the seam graph (26), which therefore carry every check but that one.
EXACT_STEPS = [k for k in EQUAL_INFORMATION if k not in ("n65", "seam")]


def gamma(m):
    return m * EPS / (1 - m * EPS)


# ---- the model's side, once per process and graph ------------------------------------------------------------------------------------------------------------
_MODEL = {}


def p_vectors(name):
    """K = 8 random vectors, then the unit vectors of the first node, of a closure's end i (side 0), of its end j (side 1) and of the last node."""
    g, _ = pc.step_graphs()[name]
    n = g["poses"].shape[0]
    is_fixed = pgm.fixed_mask(n, g["fixed"])
    off = [(c[0], c[1]) for c in g["closures"] if abs(c[0] - c[1]) >= 2 and not is_fixed[c[0]] and not is_fixed[c[1]]] or [(c[0], c[1]) for c in g["closures"]]
    p = [np.random.default_rng(5).standard_normal((8, n, 6))]
    for node in (0, off[0][0], off[0][1], n - 1):
        u = np.zeros((6, n, 6)); u[np.arange(6), node, np.arange(6)] = 1.0
        p.append(u)
    return np.concatenate(p)


def res_bound(T, edges, X):
    """(a): E x 6."""
    out = np.zeros((len(edges), 6))
    for q, (i, j) in enumerate(edges):
        Ri, Rj, d = T[i][:3, :3], T[j][:3, :3], T[j][:3, 3] - T[i][:3, 3]
        x = pgm.xof(T[i], T[j])
        RX, aRX = Rj.T @ Ri, np.abs(Rj.T) @ np.abs(Ri)
        side = np.zeros(6)
        side[:3] = gamma(4) * (np.abs(Rj.T) @ np.abs(d))
        side[3] = gamma(3) * (aRX[2, 1] + aRX[2, 2]) / np.hypot(RX[2, 1], RX[2, 2]) + 2 * EPS * abs(x[3])
        side[4] = gamma(3) * aRX[2, 0] / np.sqrt(1 - min(RX[2, 0] ** 2, 1 - 1e-12)) + 2 * EPS * abs(x[4])
        side[5] = gamma(3) * (aRX[1, 0] + aRX[0, 0]) / np.hypot(RX[1, 0], RX[0, 0]) + 2 * EPS * abs(x[5])
        out[q] = 2 * side + 4 * EPS * (np.abs(x) + np.abs(X[q]))
        out[q, 3:] += 4 * EPS          # the model's wrap forms pi - a and takes pi off again: two roundings at the size of pi (half an ulp there is 2 eps)
    return out


def chi_bound(e, info, de):
    return np.array([2 * np.abs(e[q]) @ np.abs(info[q]) @ de[q] + de[q] @ np.abs(info[q]) @ de[q] + 2 * gamma(13) * (np.abs(e[q]) @ np.abs(info[q]) @ np.abs(e[q]))
                     for q in range(len(e))])


def model(name):
    if name in _MODEL:
        return _MODEL[name]
    g, o = pc.step_graphs()[name]
    n = g["poses"].shape[0]
    closures = list(g["closures"])
    edges = pgm.edge_list(n, closures)
    X, info = pgm._measurements(n, g["odo_X"], g["odo_info"], closures)
    is_fixed = pgm.fixed_mask(n, g["fixed"])
    free = np.nonzero(~is_fixed)[0]
    T = np.asarray(g["poses"], np.float32).reshape(n, 4, 4).astype(np.float64)
    J, e, H, gv = pgm.linearise(T, edges, X, info, is_fixed, o.get("damping", 0.0))
    noise = max(float(np.abs(J[q] - pgm.jacobians_ld(T[i], T[j])).max()) for q, (i, j) in enumerate(edges))
    dJ = 4 * noise
    de = res_bound(T, edges, X)
    # (c): the bounds of H and g, accumulated as linearise accumulates H and g
    col = -np.ones(n, int); col[free] = np.arange(free.size)
    items = np.zeros(n, int)
    bH, aH, bg, ag = np.zeros_like(H), np.zeros_like(H), np.zeros_like(gv), np.zeros_like(gv)
    dj = np.full((6, 6), dJ)
    for q, (i, j) in enumerate(edges):
        W = np.abs(info[q])
        for (a, Ja) in ((i, np.abs(J[q][:, :6])), (j, np.abs(J[q][:, 6:]))):
            if col[a] < 0:
                continue
            items[a] += 1
            sa = slice(6 * col[a], 6 * col[a] + 6)
            bg[sa] += dj.T @ W @ np.abs(e[q]) + Ja.T @ W @ de[q] + dj.T @ W @ de[q]
            ag[sa] += Ja.T @ W @ np.abs(e[q])
            for (b, Jb) in ((i, np.abs(J[q][:, :6])), (j, np.abs(J[q][:, 6:]))):
                if col[b] >= 0:
                    sb = slice(6 * col[b], 6 * col[b] + 6)
                    bH[sa, sb] += Ja.T @ W @ dj + dj.T @ W @ Jb + dj.T @ W @ dj
                    aH[sa, sb] += Ja.T @ W @ Jb
    m_sum = 14 + int(items.max())
    bH += 2 * gamma(m_sum) * (aH + o.get("damping", 0.0) * np.eye(H.shape[0]))
    bg += 2 * gamma(m_sum) * ag
    M = pgm.band_of(H, is_fixed)
    c_off = sum(1 for (i, j) in edges[n - 1:] if abs(i - j) >= 2 and not is_fixed[i] and not is_fixed[j])
    tol = o.get("pcg_tol", 0.0) or PCG_TOL
    ref = pgm.pcg_reference(H, gv, M, tol, H.shape[0] + 8)          # (its own count: capped only by the dimension)
    L = np.linalg.cholesky(M)
    S = np.linalg.solve(L, np.linalg.solve(L, H).T)
    ev = np.linalg.eigvalsh(0.5 * (S + S.T))
    m = dict(name=name, g=g, o=o, n=n, edges=edges, X=X, info=info, is_fixed=is_fixed, free=free, T=T, J=J, e=e, H=H, gv=gv, chi=pgm.edge_chi2(T, edges, X, info),
             noise=noise, dJ=dJ, de=de, bH=bH, bg=bg, M=M, c_off=c_off, tol=tol, ref=ref, xstar=np.linalg.solve(H, -gv), cond=float(ev[-1] / ev[0]),
             cap=1 if c_off == 0 else (o.get("max_pcg", 0) or 12 * c_off + 8))
    _MODEL[name] = m
    return m


# ---- the checks: each takes a result of the hook (host build or device) and the model, prints its figures, asserts, and returns the figures ---------------------
def check_a(r, m):
    d_res = np.abs(r["res"] - m["e"])
    d_chi = np.abs(r["chi_start"] - m["chi"])
    bc = chi_bound(m["e"], m["info"], m["de"])
    fig = dict(res=float(d_res.max()), res_of_bound=float((d_res / m["de"]).max()), chi_of_bound=float((d_chi / np.maximum(bc, 1e-300)).max()))
    print("  (a) %s: res differs by at most %.3e (%.2f of its bound), chi by %.2f of its bound" % (m["name"], fig["res"], fig["res_of_bound"], fig["chi_of_bound"]))
    assert (d_res <= m["de"]).all() and (d_chi <= bc).all()
    assert abs(r["chi2_start"] - m["chi"].sum()) <= bc.sum() + gamma(len(bc) + 8) * np.abs(m["chi"]).sum()
    if r["trial"]:      # the trial poses' chi2, against the model at the returned trial poses
        Tt = pc.poses64_matrix(r["Pt"])
        et = np.array([pgm.residual(Tt[i], Tt[j], m["X"][q]) for q, (i, j) in enumerate(m["edges"])]).reshape(-1, 6)
        bt = chi_bound(et, m["info"], res_bound(Tt, m["edges"], m["X"]))
        assert (np.abs(r["chi_trial"] - pgm.edge_chi2(Tt, m["edges"], m["X"], m["info"])) <= bt).all()
    return fig


def check_b(r, m):
    d = np.abs(r["J"] - m["J"])
    largest = np.abs(m["J"]).reshape(len(m["edges"]), -1).max(axis=1)
    fig = dict(noise=m["noise"], dJ=float(d.max()), bound=m["dJ"], rel=float(m["dJ"] / largest.min()))
    print("  (b) %s: J differs by at most %.3e; the model's float64 J is %.3e from its longdouble twin, bound %.3e (%.2e of the smallest edge's largest entry)"
          % (m["name"], fig["dJ"], fig["noise"], fig["bound"], fig["rel"]))
    assert m["dJ"] <= 1e-6 * largest.min()
    assert (d <= m["dJ"]).all()
    return fig


def check_c(r, m):
    Hd = pgm.dense_from_band(r["D"], r["B"], r["A"], m["edges"], m["is_fixed"])
    dH, dg = np.abs(Hd - m["H"]), np.abs(r["g"][m["free"]].reshape(-1) - m["gv"])
    fig = dict(dH=float(dH.max()), H_of_bound=float((dH / np.maximum(m["bH"], 1e-300)).max()) if dH.size else 0.0,
               dg=float(dg.max()) if dg.size else 0.0, g_of_bound=float((dg / np.maximum(m["bg"], 1e-300)).max()) if dg.size else 0.0)
    print("  (c) %s: H differs by at most %.3e (%.3f of its bound), g by %.3e (%.3f of its bound)" % (m["name"], fig["dH"], fig["H_of_bound"], fig["dg"], fig["g_of_bound"]))
    assert (dH <= m["bH"]).all() and (dg <= m["bg"]).all()
    D = r["D"].reshape(-1, 6, 6)
    assert np.array_equal(D.view(np.uint64), D.transpose(0, 2, 1).copy().view(np.uint64))
    # a fixed node: D = I, no coupling to it or from it, g = 0
    for k in np.nonzero(m["is_fixed"])[0]:
        assert np.array_equal(D[k], np.eye(6)) and not r["B"][k].any() and not r["g"][k].any() and (k + 1 >= m["n"] or not r["B"][k + 1].any())
    return fig


def row_terms(m):
    """Per node the products a row of q = H p sums: 6 per block the kernel walks (D, the two couplings, the node's off-band closure items)."""
    n = m["n"]
    t = np.array([6 * (1 + (k > 0) + (k < n - 1)) for k in range(n)])
    for (i, j) in m["edges"][n - 1:]:
        if abs(i - j) >= 2:
            t[i] += 6; t[j] += 6
    return t


def check_d(r, m, p):
    Hd = pgm.dense_from_band(r["D"], r["B"], r["A"], m["edges"], m["is_fixed"], np.longdouble)
    free, fixed = m["free"], np.nonzero(m["is_fixed"])[0]
    gm = np.repeat(np.array([gamma(int(t)) for t in row_terms(m)[free]]), 6)
    worst = 0.0
    for k in range(p.shape[0]):
        pf = p[k][free].reshape(-1).astype(np.longdouble)
        d = np.abs(r["q"][k][free].reshape(-1) - Hd @ pf)
        b = gm * (np.abs(Hd) @ np.abs(pf))
        worst = max(worst, float((d / np.maximum(b, np.longdouble(1e-300))).max()) if d.size else 0.0)
        assert (d <= b).all(), (m["name"], k)
        assert np.array_equal(r["q"][k][fixed].view(np.uint64), p[k][fixed].view(np.uint64))
    print("  (d) %s: q = H p over %d vectors: at most %.3f of gamma(m) |H||p|" % (m["name"], p.shape[0], worst))
    return dict(q_of_bound=worst)


def replay(r, m, solves=None, cholesky=False):
    """x of the CG recurrence in NumPy on the returned D, B, A and g, with alpha and beta from the returned scalars.  (x, its last step's H-norm, H).  The band
    solve is pgm.band_solver: the LU of numpy.linalg.solve, or with `cholesky` the band's Cholesky factor: another float64 solver of the same system."""
    Hd = pgm.dense_from_band(r["D"], r["B"], r["A"], m["edges"], m["is_fixed"])
    Md = pgm.band_of(Hd, m["is_fixed"])
    solve = pgm.band_solver(Md, cholesky)
    gd = r["g"][m["free"]].reshape(-1)
    sc = r["cg_scalars"]
    x, rr, p, last = np.zeros_like(gd), -gd.copy(), None, 0.0
    for i in range(sc.shape[0] if solves is None else solves):
        z = solve(rr)
        p = z if i == 0 else z + (sc[i, 0] / sc[i - 1, 0]) * p
        if np.isnan(sc[i, 1]):
            break
        alpha = sc[i, 0] / sc[i, 1]
        x, rr = x + alpha * p, rr - alpha * (Hd @ p)
        last = abs(alpha) * np.sqrt(sc[i, 1])
    return x, last, Hd


def check_e(r, m):
    sc, tol = r["cg_scalars"], m["tol"]
    nb = r["band_solves"]
    assert sc.shape[0] == nb and r["cap"] == m["cap"] and r["c_offband"] == m["c_off"] and r["factor_status"] == 0 and r["cg_status"] == 0
    rz, pq = sc[:, 0], sc[:, 1]
    ratios = np.sqrt(rz / rz[0])
    # the ending reason against the scalars
    assert np.isfinite(rz).all() and (rz[:-1] > 0).all() and (pq[:-1] > 0).all() and (ratios[1:-1] > tol).all()
    if r["cg_end"] == TOL:
        assert nb >= 2 and ratios[-1] <= tol and np.isnan(pq[-1]) and rz[-1] > 0
    elif r["cg_end"] == ZERO:
        assert rz[-1] == 0.0 and np.isnan(pq[-1])
    else:
        assert r["cg_end"] == CAP and nb == r["cap"] and pq[-1] > 0 and rz[-1] > 0 and (nb == 1 or ratios[-1] > tol)
    # x from the history
    xr, last, Hd = replay(r, m)
    xc = replay(r, m, cholesky=True)[0]
    own = float(np.sqrt((xc - xr) @ Hd @ (xc - xr)))          # the replay's own error: the same recurrence with another float64 band solver
    xd = r["x"][m["free"]].reshape(-1)
    off = float(np.sqrt((xd - xr) @ Hd @ (xd - xr)))
    xn = float(np.sqrt(xd @ Hd @ xd))
    true_ratio = pgm.precond_ratio(m["H"], m["gv"], m["M"], xd)
    bound = 10 * max(tol, m["ref"]["ratio"])
    fig = dict(band_solves=nb, ref_solves=m["ref"]["iterations"], ratio=true_ratio, ref_ratio=m["ref"]["ratio"], end=r["cg_end"], replay_off=off / last if last else 0.0,
               replay_own=own / last if last else 0.0)
    print("  (e) %s: %d band solves (the reference: %d steps, cap %d), end %d; true ratio %.3e (reference %.3e, bound %.3e); the replay is %.3e of the last step off, two replays %.3e of it apart (|x|_H %.3e, last step %.3e)"
          % (m["name"], nb, m["ref"]["iterations"], r["cap"], r["cg_end"], true_ratio, m["ref"]["ratio"], bound, fig["replay_off"], fig["replay_own"], xn, last))
    assert not r["x"][m["is_fixed"]].any()
    assert off <= max(0.5 * last, 10 * own)
    if r["cg_end"] == TOL or m["c_off"] == 0:
        assert true_ratio <= bound
    assert nb <= m["ref"]["iterations"] + 2
    if m["name"] in EXACT_STEPS:
        assert m["ref"]["iterations"] <= 12 * m["c_off"] + 1
    if m["name"] in EQUAL_INFORMATION:
        assert r["cg_end"] == (TOL if m["c_off"] else CAP)
    return fig


def check_f(r, m):
    if not (r["cg_end"] == TOL or m["c_off"] == 0):
        return {}
    xd, xs, H = r["x"][m["free"]].reshape(-1), m["xstar"], m["H"]
    rel = float(np.sqrt((xd - xs) @ H @ (xd - xs)) / np.sqrt(xs @ H @ xs))
    bound = 10 * max(m["tol"], m["ref"]["ratio"]) * np.sqrt(m["cond"])
    print("  (f) %s: x is %.3e of the dense solve off in the H-norm; bound %.3e (cond(M^-1 H) %.3e)" % (m["name"], rel, bound, m["cond"]))
    assert rel <= bound
    return dict(x_rel=rel, x_bound=float(bound), cond=m["cond"])


def check_g(r, m):
    Pt = pc.poses64_matrix(r["Pt"])
    worst = 0.0
    for k in range(m["n"]):
        if m["is_fixed"][k]:
            assert np.array_equal(Pt[k].view(np.uint64), m["T"][k].view(np.uint64))
            continue
        Ex = pgm.exp_se3(r["x"][k])
        ref = m["T"][k] @ Ex
        b = np.zeros((3, 4))
        b[:, :3] = 20 * EPS * (np.abs(m["T"][k][:3, :3]) @ np.abs(Ex[:3, :3]))
        b[:, 3] = 20 * EPS * (np.abs(m["T"][k][:3, 3]) + np.abs(m["T"][k][:3, :3]) @ np.abs(Ex[:3, 3]))
        d = np.abs(Pt[k][:3] - ref[:3])
        worst = max(worst, float((d / b).max()))
        assert (d <= b).all(), (m["name"], k)
    print("  (g) %s: Pt is at most %.3f of its bound from T exp_se3(x)" % (m["name"], worst))
    return dict(Pt_of_bound=worst)


def check_all(r, m, p):
    fig = {}
    for f in (check_a, check_b, check_c, lambda r_, m_: check_d(r_, m_, p), check_e, check_f, check_g):
        fig.update(f(r, m))
    return fig


def check_strong(name, r):
    """The documented finding: with closure information 4e4 times the odometry's the default cap ends the solve, max_pcg = 100 lets it reach pcg_tol."""
    if name == "strong":
        assert r["cg_end"] == CAP and r["band_solves"] == r["cap"] == 12 * r["c_offband"] + 8
    if name == "strong100":
        assert r["cg_end"] == TOL and r["cap"] == 100


def seam_sides(g):
    """Per seam closure (the yaw the start poses predict, the measured yaw)."""
    T = np.asarray(g["poses"], np.float64)
    return [(float(pgm.xof(T[c[0]], T[c[1]])[5]), float(c[2][5])) for c in g["closures"]]


# ---- CPU: the model's own pieces ---------------------------------------------------------------------------------------------------------------------------------
def _inline_assembly(T, edges, X, info, is_fixed, damping):
    """The assembly loop as pgm.optimise had it inline before linearise was split out, word for word."""
    free = np.nonzero(~is_fixed)[0]
    col = -np.ones(len(is_fixed), int); col[free] = np.arange(free.size)
    m = 6 * free.size
    H, g = np.zeros((m, m)), np.zeros(m)
    for q, (i, j) in enumerate(edges):
        J = pgm.jacobians(T[i], T[j])
        e = pgm.residual(T[i], T[j], X[q])
        for (a, Ja) in ((i, J[:, :6]), (j, J[:, 6:])):
            if col[a] < 0:
                continue
            sa = slice(6 * col[a], 6 * col[a] + 6)
            g[sa] += Ja.T @ info[q] @ e
            for (b, Jb) in ((i, J[:, :6]), (j, J[:, 6:])):
                if col[b] >= 0:
                    H[sa, 6 * col[b]:6 * col[b] + 6] += Ja.T @ info[q] @ Jb
    H += damping * np.eye(m)
    return H, g


@pytest.mark.parametrize("case", range(len(pc.CASES)), ids=["n%d_c%d" % (c[0], len(c[1])) for c in pc.CASES])
def test_linearise_is_the_loop_optimise_had(case):
    """pgm.linearise returns the bits of the loop it was lifted from, at the start poses and at the poses the model ends on, with and without damping."""
    n, pairs, fx = pc.CASES[case]
    g = pc.graph(n, pairs, fx, True)
    edges = pgm.edge_list(n, g["closures"])
    X, info = pgm._measurements(n, g["odo_X"], g["odo_info"], g["closures"])
    is_fixed = pgm.fixed_mask(n, g["fixed"])
    for T in (np.asarray(g["poses"], np.float64), pc.model(("loop", n, pairs, fx, True), g)["poses64"]):
        for damping in (0.0, 1e-3):
            _, _, H, gv = pgm.linearise(T, edges, X, info, is_fixed, damping)
            H0, g0 = _inline_assembly(T, edges, X, info, is_fixed, damping)
            assert np.array_equal(H.view(np.uint64), H0.view(np.uint64)) and np.array_equal(gv.view(np.uint64), g0.view(np.uint64))


def test_the_seam_graph_straddles_the_seam():
    g = pc.seam_graph()
    sides = seam_sides(g)
    print("seam closures (predicted, measured yaw):", sides)
    assert all(abs(abs(a) - np.pi) < 1e-3 + 5e-3 and abs(abs(b) - np.pi) < 1e-3 for a, b in sides)      # (the prediction carries the chain's drift)
    assert sum(1 for a, b in sides if (a > 0) != (b > 0)) >= 2
    T = np.asarray(g["poses"], np.float64)
    for c in g["closures"]:
        raw = pgm.xof(T[c[0]], T[c[1]])[5] - float(c[2][5])
        assert abs(raw) > 6.0 and abs(pgm.residual(T[c[0]], T[c[1]], c[2])[5]) < 0.02


def test_the_reference_cg_meets_the_exact_arithmetic_bound():
    """The textbook CG ends by tolerance on every graph, on the graphs of EXACT_STEPS within 12 c_offband + 1 steps (H = M + a term of rank <= 12 c_offband)."""
    for name in NAMES:
        m = model(name)
        print(name, "c_offband", m["c_off"], "reference steps", m["ref"]["iterations"], "ratio %.3e" % m["ref"]["ratio"], "cond(M^-1 H) %.3e" % m["cond"])
        assert m["ref"]["end"] == "tolerance"
        if name in EXACT_STEPS:
            assert m["ref"]["iterations"] <= 12 * m["c_off"] + 1


# ---- CPU: the host build of the hook -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """name -> the hook's result from the host build; the plain, the sanitised and the four-thread builds write the same bytes."""
    tmp = tmp_path_factory.mktemp("pg_step")
    src = os.path.join(ROOT, "tests", "cpp", "test_posegraph_optimize.cpp")
    items = [(pc.step_graphs()[k][0], pc.step_graphs()[k][1], p_vectors(k)) for k in NAMES]
    fin = str(tmp / "graphs.bin")
    pc.write_step_graphs(fin, items)
    outs = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ("emu", ["-O2", "-DICET_PG_EMU", "-pthread"])):
        exe = str(tmp / ("test_posegraph_step_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", ROOT, src, "-o", exe])
        fout = str(tmp / (name + ".bin"))
        r = subprocess.run([exe, "step", fin, fout], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        outs[name] = open(fout, "rb").read()
        if name == "plain":
            print(r.stdout)
    assert outs["plain"] == outs["san"] == outs["emu"]
    return dict(zip(NAMES, pc.read_step_results(str(tmp / "plain.bin"), items)))


@pytest.mark.parametrize("name", NAMES)
def test_host_step_against_the_model(host, name):
    r, m = host[name], model(name)
    check_all(r, m, p_vectors(name))
    check_strong(name, r)


def _copy(r):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def test_the_checks_bite(host):
    """Six corruptions of a correct host result, pure NumPy: each fails the check it names (and the result it was made from passes it)."""
    # one A block transposed; one incidence item dropped from D; the B contribution of the reversed neighbour closure (3, 2) transposed
    r, m = host["n6"], model("n6")
    check_c(r, m)
    n = m["n"]
    c = next(q for q, (i, j) in enumerate(m["edges"][n - 1:]) if abs(i - j) >= 2 and not m["is_fixed"][i] and not m["is_fixed"][j])
    bad = _copy(r); bad["A"][c] = bad["A"][c].T.copy()
    with pytest.raises(AssertionError):
        check_c(bad, m)
    q = n - 1 + c
    i = m["edges"][q][0]
    bad = _copy(r); bad["D"][i] -= m["J"][q][:, :6].T @ m["info"][q] @ m["J"][q][:, :6]
    with pytest.raises(AssertionError):
        check_c(bad, m)
    q = m["edges"].index((3, 2))
    blk = m["J"][q][:, :6].T @ m["info"][q] @ m["J"][q][:, 6:]          # the closure's block at (3, 2)
    bad = _copy(r); bad["B"][3] += blk.T - blk
    with pytest.raises(AssertionError):
        check_c(bad, m)
    # the residual of a seam edge left unwrapped
    r, m = host["seam"], model("seam")
    check_a(r, m)
    q = next(q for q in range(m["n"] - 1, len(m["edges"])) if abs(pgm.xof(m["T"][m["edges"][q][0]], m["T"][m["edges"][q][1]])[5] - m["X"][q][5]) > 6.0)
    bad = _copy(r); bad["res"][q, 5] = pgm.xof(m["T"][m["edges"][q][0]], m["T"][m["edges"][q][1]])[5] - m["X"][q][5]
    with pytest.raises(AssertionError):
        check_a(bad, m)
    # q with one closure side skipped (the end j of the first off-band closure: the transposed block)
    r, m, p = host["n33"], model("n33"), p_vectors("n33")
    check_d(r, m, p)
    c = next(q for q, (i, j) in enumerate(m["edges"][m["n"] - 1:]) if abs(i - j) >= 2 and not m["is_fixed"][i] and not m["is_fixed"][j])
    i, j = m["edges"][m["n"] - 1 + c]
    bad = _copy(r)
    for k in range(p.shape[0]):
        bad["q"][k][j] -= r["A"][c].T @ p[k][i]
    with pytest.raises(AssertionError):
        check_d(bad, m, p)
    # x from a CG stopped one iteration early, the scalars as returned
    assert check_e(r, m)["replay_own"] < 0.05          # (here the replay resolves the last step: the half-step bound is the one in force)
    steps = int(np.isfinite(r["cg_scalars"][:, 1]).sum())
    x_early = replay(r, m, steps - 1)[0]
    bad = _copy(r); bad["x"][m["free"]] = x_early.reshape(-1, 6)
    with pytest.raises(AssertionError):
        check_e(bad, m)


def test_corrupted_jacobians_fail(host):
    """A 5 % error of the rotation columns and a one-sided difference, applied to a copy of the model's J: both fail (b), and H built from them fails (c)."""
    r, m = host["n33"], model("n33")
    check_b(r, m)
    T = m["T"]
    one_sided = np.zeros_like(m["J"])
    for q, (i, j) in enumerate(m["edges"]):
        for c in range(6):
            d = np.zeros(6); d[c] = pgm.JAC_STEP
            a = pgm.xof(T[i] @ pgm.exp_se3(d), T[j]) - pgm.xof(T[i], T[j]); a[3:] = pgm.wrap(a[3:])
            b = pgm.xof(T[i], T[j] @ pgm.exp_se3(d)) - pgm.xof(T[i], T[j]); b[3:] = pgm.wrap(b[3:])
            one_sided[q][:, c], one_sided[q][:, 6 + c] = a / pgm.JAC_STEP, b / pgm.JAC_STEP
    scaled = m["J"].copy(); scaled[:, :, 3:6] *= 1.05; scaled[:, :, 9:12] *= 1.05
    for Jbad in (scaled, one_sided):
        with pytest.raises(AssertionError):
            check_b(dict(r, J=Jbad), m)
        # H from the corrupted J, in the device's layout: only the diagonal blocks are needed to fail (c)
        bad = _copy(r)
        for k in m["free"]:
            bad["D"][k] = 0.0
        for q, (i, j) in enumerate(m["edges"]):
            for (a, Ja) in ((i, Jbad[q][:, :6]), (j, Jbad[q][:, 6:])):
                if not m["is_fixed"][a]:
                    bad["D"][a] += Ja.T @ m["info"][q] @ Ja
        bad["D"] = 0.5 * (bad["D"] + bad["D"].transpose(0, 2, 1))
        with pytest.raises(AssertionError):
            check_c(bad, m)


# ---- GPU: the same checks through the hook -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import icet_amd
    c = icet_amd.Context(0)
    yield c
    c.close()


def _device_step(ctx, name):
    g, o = pc.step_graphs()[name]
    return ctx.debug_pose_graph_step(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], p=p_vectors(name), **o)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_step_against_the_model(ctx, name):
    """Measured on an MI355X: DESIGN.md section 20 has the table."""
    r, m = _device_step(ctx, name), model(name)
    check_all(r, m, p_vectors(name))
    check_strong(name, r)
    # the hook is the optimiser's first iteration: gn_iters = 1 returns its trial poses (the step lowers chi2 on every graph here) and its band solves
    g, o = pc.step_graphs()[name]
    w = ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], gn_iters=1, **o)
    assert r["chi2_trial"] < r["chi2_start"]
    assert w["pcg_iterations"] == r["band_solves"] and w["chi2_initial"] == r["chi2_start"] and w["chi2_final"] == r["chi2_trial"] and w["max_dx"] == r["max_dx"]
    assert np.array_equal(w["poses64"].view(np.uint64), pc.poses64_matrix(r["Pt"]).view(np.uint64))
    assert np.array_equal(w["edge_chi2"][0], r["chi_start"]) and np.array_equal(w["edge_chi2"][1], r["chi_trial"])


@pytest.mark.gpu
def test_device_strong_closures_whole_run(ctx):
    """The finding as a test: with max_pcg = 100 the whole run takes the model's iterations (+-1) to the model's optimum."""
    g, _ = pc.step_graphs()["strong"]
    m = pc.model(("strong",), g)
    r = ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL, max_pcg=100)
    pc.compare("strong closures, max_pcg = 100", r, m, g)
    d = ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL, gn_iters=30)
    print("    default cap: %d iterations, %d band solves, status %d (the model: %d iterations)" % (d["gn_iterations"], d["pcg_iterations"], d["status"], m["gn_iterations"]))
