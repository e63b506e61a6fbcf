"""The pose graph's COVARIANCE COLUMNS and GATE restated in float64 NumPy (DESIGN.md section 20 "Covariance columns and the gate"): block (k, t) of H^-1 from the
dense inverse and from M^-1 - P P^T + Q Q^T, the residual covariance S and the Mahalanobis distance d2 of a candidate closure; the scaled measure; the targets
and candidates per graph, the file format of tests/cpp/test_posegraph_cross.cpp and the checks that tests/test_pose_graph_cross_host.py runs on the host build's
output and tests/test_pose_graph_cross.py on the device's.  It builds on the graphs and references of pose_graph_marginals_model.py; nothing here is shared with
the device code.

THE MEASURE.  scaled_x(S, F) = max over the free nodes k, the free targets t and the entries a, b of |S[t][k] - F_kt|_ab / sqrt(F_kk,aa F_tt,bb): an error of a
covariance in units of the two standard deviations it is about.
THE BOUNDS follow the marginals' rule.  own_x(X) is scaled_x between numpy.linalg.inv and the inverse through a Cholesky factor on the matrix X that a check
inverts; a check allows MARGIN x own_x; against the model's H it also allows 4 x the Jacobian term (pgm.jacobians against pgm.jacobians_ld).  No bound may
exceed CAP."""
import os
import struct
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_direct_model as pdm      # noqa: E402
import pose_graph_marginals_model as pmm      # noqa: E402
import pose_graph_model as pgm      # noqa: E402

ROOT = pdm.ROOT
CAP, MARGIN = pmm.CAP, pmm.MARGIN
GATE_CAP = 1e-5
MAX_TARGETS = 32
DEFAULT_THRESHOLD = 16.8119
QNAN = np.uint64(0x7ff8000000000000)

# the targets per graph: the fixed node, either side of a staged chunk of 32, the last node, end nodes and nodes that are none
TARGETS = {"n1": [0], "n2": [1], "n3": [2, 1], "n6": [4, 0, 5, 1, 3], "n33": [0, 31, 32, 30, 5], "n65": [0, 31, 32, 33, 64], "chain65": [0, 31, 32, 33, 64, 20, 50],
           "m0": [1, 3], "rank5": [11, 5], "strong": [30, 1, 17], "ends288": [1, 55, 114, 119], "ends128": list(range(1, 140, 4))[:29] + [70, 139, 0], "n257": [256]}
# (T = 1 on n1, n2 and n257; T = 32 on ends128 with q = 768: both limits at once)
assert len(TARGETS["ends128"]) == MAX_TARGETS and len(set(TARGETS["ends128"])) == MAX_TARGETS


def graphs():
    return pmm.graphs()


# ---- the references and the measure ----------------------------------------------------------------------------------------------------------------------------
def embed(Xf, is_fixed):
    """The 6n x 6n covariance from the one over the free nodes: zero rows and columns at the fixed nodes."""
    is_fixed = np.asarray(is_fixed, bool)
    n = is_fixed.size
    idx = (6 * np.nonzero(~is_fixed)[0][:, None] + np.arange(6)).reshape(-1)
    F = np.zeros((6 * n, 6 * n))
    F[np.ix_(idx, idx)] = Xf
    return F


def cols_of(F, targets):
    """T x n x 6 x 6: [t][k] is block (k, targets[t]) of F."""
    n = F.shape[0] // 6
    return np.stack([F[:, 6 * t:6 * t + 6].reshape(n, 6, 6) for t in targets])


def chol_inv(X):
    Ci = np.linalg.solve(np.linalg.cholesky(X), np.eye(X.shape[0]))
    return Ci.T @ Ci


def scaled_x(S, F, targets, is_fixed):
    """The measure above: S is T x n x 6 x 6, F the 6n x 6n reference."""
    is_fixed = np.asarray(is_fixed, bool)
    n = is_fixed.size
    S = np.asarray(S, np.float64).reshape(len(targets), n, 6, 6)
    sd = np.sqrt(np.diag(F)).reshape(n, 6)
    R = cols_of(F, targets)
    free = np.nonzero(~is_fixed)[0]
    worst = 0.0
    for ti, t in enumerate(targets):
        if is_fixed[t] or free.size == 0:
            continue
        den = sd[free][:, :, None] * sd[t][None, None, :]
        worst = max(worst, float((np.abs(S[ti][free] - R[ti][free]) / den).max()))
    return worst


def own_x(H, targets, is_fixed):
    """(the scaled distance between the two NumPy references on H over the targets' columns, the first of them as 6n x 6n)."""
    if H.size == 0:
        return 0.0, embed(H, is_fixed)
    F = embed(np.linalg.inv(H), is_fixed)
    return scaled_x(cols_of(embed(chol_inv(H), is_fixed), targets), F, targets, is_fixed), F


_MODEL = {}


def model_ref(name, g):
    """(F of the model's H, own_x, the Jacobian term, F of the model's H from pgm.jacobians_ld) over the graph's targets, once per process and name."""
    if name not in _MODEL:
        is_fixed = pgm.fixed_mask(g["poses"].shape[0], g["fixed"])
        t = TARGETS[name]
        o, F = own_x(pmm.model_H(g), t, is_fixed)
        Hl = pmm.model_H(g, ld=True)
        Fl = embed(np.linalg.inv(Hl), is_fixed) if Hl.size else F
        _MODEL[name] = (F, o, scaled_x(cols_of(Fl, t), F, t, is_fixed), Fl)
    return _MODEL[name]


# ---- the NumPy restatement of the device's formula ----------------------------------------------------------------------------------------------------------------
def restate(D, B, A, edges, is_fixed, targets, drop_qq=False, transpose_block=False, swap_kt=False, skip_end=None):
    """cols (T x n x 6 x 6) from D, B, A by block (k, t) = [M^-1](k, t) - P_k P_t^T + Q_k Q_t^T.  The keywords are the corruptions of "the checks bite"."""
    D = np.asarray(D, np.float64).reshape(-1, 6, 6)
    n = D.shape[0]
    is_fixed = np.asarray(is_fixed, bool)
    M = pdm.dense_band(D, B)
    Minv = np.linalg.inv(M)
    ends = pdm.ends_of(n, edges[n - 1:], is_fixed)
    q = 6 * len(ends)
    P, Q = np.zeros((6 * n, q)), np.zeros((6 * n, q))
    if ends:
        U = np.zeros((6 * n, q))
        for a, k in enumerate(ends):
            U[6 * k:6 * k + 6, 6 * a:6 * a + 6] = np.eye(6)
        S = pdm.s_matrix(A, edges, ends, is_fixed, n)
        Z = Minv @ U
        L = np.linalg.cholesky(pdm._mirror(U.T @ Z))
        Lk = np.linalg.cholesky(pdm._mirror(np.eye(q) + L.T @ (S @ L)))
        P = np.linalg.solve(L, Z.T).T
        Q = np.linalg.solve(Lk, P.T).T
        if skip_end is not None:
            P[:, 6 * skip_end:6 * skip_end + 6] = 0; Q[:, 6 * skip_end:6 * skip_end + 6] = 0
    out = np.zeros((len(targets), n, 6, 6))
    for ti, t in enumerate(targets):
        for k in range(n):
            if is_fixed[k] or is_fixed[t]:
                continue
            Pk, Pt, Qk, Qt = P[6 * k:6 * k + 6], P[6 * t:6 * t + 6], Q[6 * k:6 * k + 6], Q[6 * t:6 * t + 6]
            corr = -(Pt @ Pk.T if swap_kt else Pk @ Pt.T) + (0 if drop_qq else (Qt @ Qk.T if swap_kt else Qk @ Qt.T))
            blk = Minv[6 * k:6 * k + 6, 6 * t:6 * t + 6] + corr
            out[ti, k] = blk.T if transpose_block else blk
    return out


# ---- the gate -----------------------------------------------------------------------------------------------------------------------------------------------------
GATE_COV = np.diag(np.array([0.005, 0.005, 0.005, 0.0005, 0.0005, 0.0005]) ** 2).astype(np.float32)      # diag(5 mm, 0.5 mrad)^2
GATE_SIGMA = np.sqrt(np.diag(GATE_COV).astype(np.float64))


def _T64(g):
    return np.asarray(g["poses"], np.float32).reshape(-1, 4, 4).astype(np.float64)


def revisit(g, i, j, frac=0.3, shift=0.0, cov=GATE_COV):
    """The candidate (i, j, X, cov) whose X is what the poses predict plus frac of a sigma per component (and `shift` metres along x)."""
    T = _T64(g)
    X = pgm.xof(T[i], T[j]) + frac * GATE_SIGMA * np.array([1, -1, 1, -1, 1, -1.0])
    X[0] += shift
    return (i, j, X.astype(np.float32), np.asarray(cov, np.float32))


def candidates(name):
    """The candidates of the gate's graphs: true revisits with i < j and i > j, the same moved by 1 m, one on the fixed node 0, both ends fixed with a positive
    definite and with a zero covariance (n6: nodes 0 and 4 are fixed).  None of them is an edge of its graph."""
    g = graphs()[name]
    n = g["poses"].shape[0]
    a, b = (1, 3) if name == "n6" else (3, n - 2)
    out = [revisit(g, a, b), revisit(g, b, a), revisit(g, a, b, shift=1.0), revisit(g, 0, n - 1 if name == "n6" else b), revisit(g, 2, 0), revisit(g, 3, n - 1)]
    if name == "n6":
        out += [revisit(g, 0, 4), revisit(g, 4, 0, cov=np.zeros((6, 6), np.float32)), revisit(g, 2, 4)]
    return out


GATE_GRAPHS = ("n6", "n33", "strong")


def gate_targets(cands):
    return sorted({int(c[1]) for c in cands})


def gate_model(g, cands, F, jac=pgm.jacobians, cross=True):
    """(d2 n_cand, S n_cand x 6 x 6) of the candidates under the 6n x 6n covariance F.  cross=False: the corruption that leaves the cross term out."""
    T = _T64(g)
    d2, Ss = [], []
    for (i, j, X, cov) in cands:
        J = np.asarray(jac(T[i], T[j]), np.float64)
        e = pgm.residual(T[i], T[j], np.asarray(X, np.float32).astype(np.float64))
        si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
        Sg = np.zeros((12, 12))
        Sg[:6, :6], Sg[6:, 6:] = F[si, si], F[sj, sj]
        if cross:
            Sg[:6, 6:], Sg[6:, :6] = F[si, sj], F[sj, si]
        c = np.asarray(cov, np.float32).astype(np.float64).reshape(6, 6)
        S = J @ Sg @ J.T + 0.5 * (c + c.T)
        Ss.append(S)
        d2.append(float(e @ np.linalg.solve(S, e)) if np.linalg.eigvalsh(S)[0] > 0 else np.nan)
    return np.array(d2), np.array(Ss)


def scaled_s(S, R):
    """max |S - R|_ab / sqrt(R_aa R_bb) over the candidates whose reference is positive on its diagonal."""
    S, R = np.asarray(S).reshape(-1, 6, 6), np.asarray(R).reshape(-1, 6, 6)
    ok = np.einsum("kaa->ka", R).min(axis=1) > 0
    if not ok.any():
        return 0.0
    d = np.sqrt(np.einsum("kaa->ka", R[ok]))
    return float((np.abs(S[ok] - R[ok]) / (d[:, :, None] * d[:, None, :])).max())


def check_gate(name, r, cands, threshold=DEFAULT_THRESHOLD):
    """d2 and S of a gate result r = dict(d2, res_cov, cand_status, rejected) against the model: relative bound MARGIN x the spread between the model with
    pgm.jacobians and with pgm.jacobians_ld, plus 10 x own_x, at most GATE_CAP."""
    g = graphs()[name]
    is_fixed = pgm.fixed_mask(g["poses"].shape[0], g["fixed"])
    t = gate_targets(cands)
    o, F = own_x(pmm.model_H(g), t, is_fixed)
    Fl = embed(np.linalg.inv(pmm.model_H(g, ld=True)), is_fixed)
    d2m, Sm = gate_model(g, cands, F)
    d2l, Sl = gate_model(g, cands, Fl, jac=pgm.jacobians_ld)
    live = np.isfinite(d2m)
    spread_d = float((np.abs(d2l - d2m)[live] / d2m[live]).max())
    spread_s = scaled_s(Sl, Sm)
    bd, bs = MARGIN * spread_d + 10 * o, MARGIN * spread_s + 10 * o
    dd = float((np.abs(np.asarray(r["d2"]) - d2m)[live] / d2m[live]).max())
    ds = scaled_s(r["res_cov"], Sm)
    print("  gate %s: d2 is %.3e (relative) from the model's, bound %.3e (spread %.3e, own %.3e); S is %.3e (scaled), bound %.3e (spread %.3e)"
          % (name, dd, bd, spread_d, o, ds, bs, spread_s))
    print("  gate %s: d2 = %s, the smallest eigenvalue of S %.3e" % (name, np.array2string(np.asarray(r["d2"]), precision=4), min(np.linalg.eigvalsh(s)[0] for s in Sm[live])))
    assert bd <= GATE_CAP and bs <= GATE_CAP
    assert dd <= bd and ds <= bs
    st = np.asarray(r["cand_status"])
    assert (st[live] == 0).all() and (st[~live] == pgm.NOT_POSITIVE_DEFINITE).all()
    assert (np.asarray(r["d2"])[~live].view(np.uint64) == QNAN).all()
    # the decisions: the model's, and the count
    assert np.array_equal(np.asarray(r["d2"])[live] < threshold, d2m[live] < threshold)
    assert r["rejected"] == int((~(np.asarray(r["d2"]) < threshold)).sum())
    return dict(d2=dd, d2_bound=bd, S=ds, S_bound=bs, d2m=d2m, Sm=Sm)


def check_symmetric_bits(S):
    """Every block symmetric bit for bit (the library's results; the NumPy model's are not)."""
    S = np.ascontiguousarray(np.asarray(S, np.float64).reshape(-1, 6, 6))
    assert np.array_equal(S.view(np.uint64), np.ascontiguousarray(S.transpose(0, 2, 1)).view(np.uint64))


def anchor_graphs():
    """chain65 and its sub-chain 20 .. 50 (node 20 becomes the fixed node 0), with the candidates (20, 50) and (0, 30) of the same measurement."""
    g = graphs()["chain65"]
    sub = dict(g, poses=g["poses"][20:51], odo_X=g["odo_X"][20:50], odo_info=g["odo_info"][20:50], closures=[], fixed=None)
    c = revisit(g, 20, 50)
    return g, [c], sub, [(0, 30, c[2], c[3])]


def anchor_bound():
    """The bound of (b) on chain65."""
    _, o, jac, _ = model_ref("chain65", graphs()["chain65"])
    return MARGIN * o + 4 * jac


# ---- the checks, on cols (T x n x 6 x 6) and a marginals-hook result r = dict(D, B, A, cov, ...) ------------------------------------------------------------------
def context(name, g):
    m = pmm.context(name, g, None)
    return dict(m, targets=TARGETS[name])


def check_a(cols, r, m):
    """cols against the blocks of the inverse of dense_from_band(D, B, A), the run's own.  Returns the bound."""
    if m["free"].size == 0:
        return 0.0
    o, F = own_x(pgm.dense_from_band(r["D"], r["B"], r["A"], m["edges"], m["is_fixed"]), m["targets"], m["is_fixed"])
    d = scaled_x(cols, F, m["targets"], m["is_fixed"])
    print("  (a) %s: cols is %.3e from inv(H) of its own D, B, A; the two NumPy references are %.3e apart (bound %.3e)" % (m["name"], d, o, MARGIN * o))
    assert MARGIN * o <= CAP and d <= MARGIN * o
    return MARGIN * o


def check_b(cols, m):
    """cols against the model's H."""
    if m["free"].size == 0:
        return 0.0
    F, o, jac, _ = model_ref(m["name"], m["g"])
    d = scaled_x(cols, F, m["targets"], m["is_fixed"])
    bound = MARGIN * o + 4 * jac
    print("  (b) %s: cols is %.3e from the model's; references %.3e apart, Jacobian term %.3e (bound %.3e)" % (m["name"], d, o, jac, bound))
    assert bound <= CAP and d <= bound
    return bound


def check_c(cols, cov, m, bound_a):
    """For two targets t, t': cols[t][t'] against cols[t'][t]^T within 2 x the bound of (a), in units of the two marginals' standard deviations."""
    t = m["targets"]
    sd = np.sqrt(np.einsum("kaa->ka", np.asarray(cov).reshape(-1, 6, 6)))
    worst = 0.0
    for a in range(len(t)):
        for b in range(a + 1, len(t)):
            if m["is_fixed"][t[a]] or m["is_fixed"][t[b]]:
                continue
            d = np.abs(cols[a][t[b]] - cols[b][t[a]].T) / (sd[t[b]][:, None] * sd[t[a]][None, :])
            worst = max(worst, float(d.max()))
    print("  (c) %s: cols[t][t'] and cols[t'][t]^T differ by at most %.3e (bound %.3e)" % (m["name"], worst, 2 * bound_a))
    assert worst <= 2 * bound_a
    return worst


def check_d(cols, cov, m, bound_a):
    """For every free node k != t: [[Sigma_kk, Sigma_kt], [Sigma_tk, Sigma_tt]] has lambda_min >= -(bound of (a)) x its trace."""
    cov = np.asarray(cov).reshape(-1, 6, 6)
    worst = np.inf
    for ti, t in enumerate(m["targets"]):
        if m["is_fixed"][t]:
            continue
        for k in m["free"]:
            if k == t:
                continue
            J = np.block([[cov[k], cols[ti][k]], [cols[ti][k].T, cov[t]]])
            lam = np.linalg.eigvalsh(J)[0] / np.trace(J)
            worst = min(worst, float(lam))
    if not np.isfinite(worst):
        return 0.0
    print("  (d) %s: the smallest eigenvalue of a joint 12 x 12 covariance over its trace is at least %.3e (bound %.3e)" % (m["name"], worst, -bound_a))
    assert worst >= -bound_a
    return worst


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def check_e(cols, cov, m):
    """Exact: the block at k = target is the marginals'; +0.0 at fixed rows and targets."""
    cols = np.asarray(cols).reshape(len(m["targets"]), m["n"], 6, 6)
    cov = np.asarray(cov).reshape(-1, 6, 6)
    for ti, t in enumerate(m["targets"]):
        assert np.array_equal(bits(cols[ti][t]), bits(cov[t]))
        z = cols[ti] if m["is_fixed"][t] else cols[ti][m["is_fixed"]]
        assert not bits(z).any()


def check_f(cols, ref, m, bound_a):
    """The device against the plain host build started from the device's D, B, A."""
    cov = ref["cov"]          # (the reference's own marginals scale the measure; its columns are the reference)
    worst = 0.0
    sd = np.sqrt(np.einsum("kaa->ka", cov))
    for ti, t in enumerate(m["targets"]):
        if m["is_fixed"][t] or m["free"].size == 0:
            continue
        den = sd[m["free"]][:, :, None] * sd[t][None, None, :]
        worst = max(worst, float((np.abs(cols[ti][m["free"]] - ref["cols"][ti][m["free"]]) / den).max()))
    print("  (f) %s: the device's cols are %.3e from the host build's (bound %.3e)" % (m["name"], worst, bound_a))
    assert worst <= bound_a
    return worst


def check_failed(cols, cov, g, targets):
    """After a failure: every block between two free nodes quiet NaN, every block that touches a fixed node zero; cov as the marginals'."""
    n = g["poses"].shape[0]
    is_fixed = pgm.fixed_mask(n, g["fixed"])
    cols = np.asarray(cols).reshape(len(targets), n, 6, 6)
    for ti, t in enumerate(targets):
        if is_fixed[t]:
            assert not bits(cols[ti]).any()
        else:
            assert (bits(cols[ti][~is_fixed]) == QNAN).all() and not bits(cols[ti][is_fixed]).any()
    if cov is not None:
        cov = np.asarray(cov).reshape(n, 6, 6)
        assert (bits(cov[~is_fixed]) == QNAN).all() and not bits(cov[is_fixed]).any()


FAILING_TARGETS = [0, 3, 11, 5]


# ---- the host build (tests/cpp/test_posegraph_cross.cpp) ------------------------------------------------------------------------------------------------------------
def build_and_run(tmp, fin, builds=pdm.BUILDS, mode=()):
    """The program built the ways of `builds` and run on fin: the outputs must be the same bytes, the sanitised runs must end clean."""
    src = os.path.join(ROOT, "tests", "cpp", "test_posegraph_cross.cpp")
    outs = {}
    for name, flags in builds:
        exe = str(tmp / ("test_posegraph_cross_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", ROOT, src, "-o", exe])
        fout = str(tmp / (name + ".bin"))
        r = subprocess.run([exe, *mode, fin, fout], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "ERROR" not in r.stderr, (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        outs[name] = open(fout, "rb").read()
        if name == "plain":
            print(r.stdout)
    assert all(v == outs["plain"] for v in outs.values())
    return str(tmp / "plain.bin")


def write_items(path, items, blocks=False):
    """items: [(graph, targets, candidates, (D, B, A) or None)]."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(items)))
        for g, targets, cands, dba in items:
            pc._write_graph(f, g, {})
            f.write(struct.pack("<i", len(targets))); f.write(np.asarray(targets, np.int32).tobytes())
            f.write(struct.pack("<i", len(cands)))
            f.write(np.array([c[0] for c in cands], np.int32).tobytes()); f.write(np.array([c[1] for c in cands], np.int32).tobytes())
            f.write(np.array([c[2] for c in cands], np.float32).tobytes()); f.write(np.array([c[3] for c in cands], np.float32).tobytes())
            f.write(struct.pack("<d", 0.0))
            if blocks:
                for v in dba:
                    f.write(np.ascontiguousarray(v, np.float64).tobytes())


def read_items(path, items):
    raw = open(path, "rb").read()
    pos, out = 0, []
    for g, targets, cands, _ in items:
        n, C, T, nc = g["poses"].shape[0], len(g["closures"]), len(targets), len(cands)
        hd = struct.unpack_from("<6i", raw, pos); pos += 24
        r = dict(zip(("status", "m", "factor_status", "wm_status", "ks_status"), hd))
        r["ends"] = np.frombuffer(raw, np.int32, r["m"], pos).copy(); pos += 4 * r["m"]
        for k, rows in (("D", n), ("B", n), ("A", C), ("band_cov", n), ("cov", n)):
            r[k] = np.frombuffer(raw, np.float64, rows * 36, pos).reshape(rows, 6, 6); pos += 288 * rows
        r["cols"] = np.frombuffer(raw, np.float64, T * n * 36, pos).reshape(T, n, 6, 6); pos += 288 * T * n
        if nc:
            gs, nt, rej = struct.unpack_from("<3i", raw, pos); pos += 12
            gate = dict(status=gs, n_targets=nt, rejected=rej)
            gate["d2"] = np.frombuffer(raw, np.float64, nc, pos).copy(); pos += 8 * nc
            gate["res_cov"] = np.frombuffer(raw, np.float64, nc * 36, pos).reshape(nc, 6, 6); pos += 288 * nc
            gate["cand_status"] = np.frombuffer(raw, np.int32, nc, pos).copy(); pos += 4 * nc
            r["gate"] = gate
        out.append(r)
    assert pos == len(raw)
    return out


def host_run(tmp, names, builds=pdm.BUILDS):
    """name -> result through the host build: the named graphs with their targets (and candidates on the gate's graphs), the failing graphs, the two anchor graphs."""
    items, keys = [], []
    for k in names:
        if k in graphs():
            items.append((graphs()[k], TARGETS[k], candidates(k) if k in GATE_GRAPHS else [], None))
        else:
            items.append((pmm.FAILING[k][0](), FAILING_TARGETS, [], None))
        keys.append(k)
    g, c, sub, cs = anchor_graphs()
    items += [(g, [50], c, None), (sub, [30], cs, None)]; keys += ["anchor_full", "anchor_sub"]
    fin = str(tmp / "graphs.bin")
    write_items(fin, items)
    return dict(zip(keys, read_items(build_and_run(tmp, fin, builds), items)))


def host_run_blocks(tmp, items):
    """items: [(graph, targets, D, B, A)], a device's own blocks: the plain host build from the band's factor on, one result per item."""
    full = [(g, t, [], (D, B, A)) for g, t, D, B, A in items]
    fin = str(tmp / "blocks.bin")
    write_items(fin, full, blocks=True)
    return read_items(build_and_run(tmp, fin, pdm.BUILDS[:1], ("blocks",)), full)
