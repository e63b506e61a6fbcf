"""A NumPy restatement of the registration against a shaped voxel map (include/icet_hip.h icet_voxel_map_register_*; the device compiles
icet_amd/csrc/icet_map_register.h), on top of tests/map_model.py, tests/map_shape_model.py and tests/deskew_model.py, written from the rule and not from the
header's text: a cell's Gaussian with Python floats, the per-row terms element-wise in float64 (one rounding per operation, in the rule's order, so they agree
with the header bit for bit), the damped 6 x 6 solve and the retraction with Python floats, and the Levenberg-Marquardt state machine of one query.  The SUMS
over rows are NumPy's here (or the reverse order, or math.fsum): the rule fixes the terms, the kernels fix an order of their own."""
import math

import numpy as np

import deskew_model as dm
import map_model as mm
import map_shape_model as sm

CONVERGED, ITERATION_CAP, STALLED, NO_OVERLAP, BAD_POSE = 0, 1, 2, 3, 4
STATUS_NAMES = ("CONVERGED", "ITERATION_CAP", "STALLED", "NO_OVERLAP", "BAD_POSE")
EMPTY = (1 << 64) - 1
SUMS = 28                                                             # F | g[6] | H[21]
LAMBDA_MIN, LAMBDA_MAX, LAMBDA_STEP, SOLVE_TRIES = 1e-9, 1e9, 10.0, 8
PIVOT_REL = 1e-13                                                     # icet_pg_rule::kPivotRel
CHUNK = 2048
DEFAULTS = dict(min_range=0.0, max_range=0.0, sigma_min=0.02, scale=11.3449, tol_t=1e-4, tol_r=1e-5, lambda0=1e-3, min_points=5, min_matched=50, max_iters=20)
TRI = [(i, j) for i in range(6) for j in range(i, 6)]                # the 21 places of the upper triangle, by rows


def params(**kw):
    assert not set(kw) - set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


# ---- a cell's Gaussian ----------------------------------------------------------------------------------------------------------------------------------------------

def gauss(key, n, sums, words, cell, sigma_min=0.02, min_points=5):
    """(mu [3], W [6] as xx xy xz yy yz zz) of the entry, Python floats, or None for an entry that takes no part.  n: the count as a signed integer; sums and
    words: the entry's words, taken as uint64 whatever they mean."""
    n = int(n)
    if n < max(1, int(min_points)):
        return None
    c = mm.key_cells(np.uint64(key))
    cellf = float(np.float32(cell))
    den = float(n) * mm.TWO32
    mu = [(float(int(c[a])) + float(int(sums[a]) & sm.MASK) / den) * cellf for a in range(3)]
    C = [float(v) for v in sm.cov(n, words, cell)]
    s2 = float(sigma_min) * float(sigma_min)
    C[0] = C[0] + s2; C[3] = C[3] + s2; C[5] = C[5] + s2
    a00 = C[3] * C[5] - C[4] * C[4]
    a01 = C[2] * C[4] - C[1] * C[5]
    a02 = C[1] * C[4] - C[2] * C[3]
    a11 = C[0] * C[5] - C[2] * C[2]
    a12 = C[1] * C[2] - C[0] * C[4]
    a22 = C[0] * C[3] - C[1] * C[1]
    det = (C[0] * a00 + C[1] * a01) + C[2] * a02
    if not (det > 0.0) or not math.isfinite(det):
        return None
    W = [a / det for a in (a00, a01, a02, a11, a12, a22)]
    if not all(math.isfinite(v) for v in W):
        return None
    return mu, W


class Gaussians:
    """The usable cells of a ShapeMap as sorted arrays: key (K,), mu (K, 3), W (K, 6)."""

    def __init__(self, shape_map, sigma_min=0.02, min_points=5):
        rows = []
        for k in sorted(shape_map.cells):
            e = shape_map.cells[k]
            g = gauss(k, e[0], e[1:4], shape_map.words(k) if k in shape_map.mom else [0] * 9, shape_map.cell, sigma_min, min_points)
            if g is not None:
                rows.append((k, g[0], g[1]))
        self.cell = shape_map.cell
        self.key = np.array([r[0] for r in rows], np.uint64)
        self.mu = np.array([r[1] for r in rows], np.float64).reshape(-1, 3)
        self.W = np.array([r[2] for r in rows], np.float64).reshape(-1, 6)

    def find(self, key):
        """Per key the row of its Gaussian, and whether there is one."""
        if self.key.shape[0] == 0:
            return np.zeros(key.shape, np.int64), np.zeros(key.shape, bool)
        i = np.minimum(np.searchsorted(self.key, key), self.key.shape[0] - 1)
        return i, self.key[i] == key


# ---- one row at a pose ----------------------------------------------------------------------------------------------------------------------------------------------

def pose64(T):
    """(R (3, 3), t (3,)) in float64 from a 4 x 4 float32 pose."""
    T = np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)
    return T[:3, :3].copy(), T[:3, 3].copy()


def pose32(R, t):
    T = np.zeros((4, 4), np.float32)
    T[:3, :3] = np.asarray(R, np.float64).astype(np.float32); T[:3, 3] = np.asarray(t, np.float64).astype(np.float32); T[3, 3] = 1.0
    return T


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def row_terms(scan, R, t, G, scale=11.3449, min_range=0.0, max_range=0.0):
    """Per row of ``scan`` (N x 3 float32) at the float64 pose (R, t) against the Gaussians G: a dict of cls (map_model's classes; KEPT and OUTSIDE rows are
    scored), key (EMPTY unless the row has a cell), matched, s, omega, rho, v (N, 28) = rho | omega J^T a | the upper triangle of omega J^T W J.  A miss has
    s = omega = 0, rho = scale; a row that is not scored has zeros."""
    p = np.asarray(scan, np.float32).reshape(-1, 3).astype(np.float64)
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    inv = 1.0 / float(np.float32(G.cell))
    mn, mx = float(np.float32(min_range)), float(np.float32(max_range))
    c = float(scale)
    n = p.shape[0]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        d2 = (x * x + y * y) + z * z
        in_range = (d2 > mn * mn) & ((mx <= 0) | (d2 <= mx * mx))
        r = [(R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z for a in range(3)]
        w = [r[a] + t[a] for a in range(3)]
        inside = np.ones(n, bool)
        cells = np.zeros((n, 3), np.int64)
        for a in range(3):
            ca = np.floor(w[a] * inv)
            ok = np.abs(ca) < mm.LIMIT                                # (a NaN compares false)
            cells[:, a] = np.where(ok, ca, 0.0).astype(np.int64)
            inside &= ok
        cls = np.full(n, mm.KEPT, np.int64)
        cls[~inside] = mm.OUTSIDE
        cls[~in_range] = mm.RANGE                                     # (the order of the rule: non-finite, range, outside)
        cls[~finite] = mm.NONFINITE
        cc = (cells + mm.LIMIT).astype(np.uint64)
        key = (cc[:, 0] << np.uint64(42)) | (cc[:, 1] << np.uint64(21)) | cc[:, 2]
        key[cls != mm.KEPT] = np.uint64(EMPTY)
        idx, found = G.find(key)
        matched = found & (cls == mm.KEPT)
        if G.key.shape[0] == 0:
            mu = np.zeros((n, 3)); W = np.zeros((n, 6))
        else:
            mu = G.mu[idx]; W = G.W[idx]
        d = [w[a] - mu[:, a] for a in range(3)]
        Wf = [[W[:, 0], W[:, 1], W[:, 2]], [W[:, 1], W[:, 3], W[:, 4]], [W[:, 2], W[:, 4], W[:, 5]]]
        a_ = [(Wf[i][0] * d[0] + Wf[i][1] * d[1]) + Wf[i][2] * d[2] for i in range(3)]
        s = (d[0] * a_[0] + d[1] * a_[1]) + d[2] * a_[2]
        tt = c / (c + s)
        pos = s > 0.0
        omega = np.where(pos, tt * tt, 1.0)
        rho = np.where(pos, c * s / (c + s), s)
        ra = _cross(r, a_)
        M = [[Wf[i][2] * r[1] - Wf[i][1] * r[2], Wf[i][0] * r[2] - Wf[i][2] * r[0], Wf[i][1] * r[0] - Wf[i][0] * r[1]] for i in range(3)]
        RR = [[r[1] * M[2][k] - r[2] * M[1][k] for k in range(3)], [r[2] * M[0][k] - r[0] * M[2][k] for k in range(3)], [r[0] * M[1][k] - r[1] * M[0][k] for k in range(3)]]
        full = [[Wf[0][0], Wf[0][1], Wf[0][2], M[0][0], M[0][1], M[0][2]],
                [None, Wf[1][1], Wf[1][2], M[1][0], M[1][1], M[1][2]],
                [None, None, Wf[2][2], M[2][0], M[2][1], M[2][2]],
                [None, None, None, RR[0][0], RR[0][1], RR[0][2]],
                [None, None, None, None, RR[1][1], RR[1][2]],
                [None, None, None, None, None, RR[2][2]]]
        v = np.zeros((n, SUMS), np.float64)
        v[:, 0] = rho
        for i in range(3):
            v[:, 1 + i] = omega * a_[i]
            v[:, 4 + i] = omega * ra[i]
        for j, (i, k) in enumerate(TRI):
            v[:, 7 + j] = omega * full[i][k]
    scored = (cls == mm.KEPT) | (cls == mm.OUTSIDE)
    miss = scored & ~matched
    v[~matched] = 0.0                                                 # (a miss is counted, not summed: totals)
    s = np.where(matched, s, 0.0); omega = np.where(matched, omega, 0.0); rho = np.where(matched, rho, np.where(miss, c, 0.0))
    return dict(cls=cls, key=key, matched=matched, scored=scored, s=s, omega=omega, rho=rho, v=v)


def totals(terms, order="forward", scale=None):
    """(v (28,), rows_scored, rows_matched) of the scored rows: the matched rows' terms summed in row order, in reverse row order, per chunk, or exactly
    (math.fsum, rounded once), and in v[0] the cost, + scale x the misses (``scale`` None: the misses' own rho, which is the scale)."""
    if order != "exact":
        tot, ns, nm = _sums(terms, order)
        c = float(terms["rho"][terms["scored"] & ~terms["matched"]][0]) if scale is None and ns > nm else float(scale or 0.0)
        tot[0] = tot[0] + c * float(ns - nm)
        return tot, ns, nm
    v = terms["v"][terms["scored"]].copy()
    v[:, 0] = terms["rho"][terms["scored"]]
    return np.array([math.fsum(v[:, j]) for j in range(SUMS)], np.float64), int(terms["scored"].sum()), int(terms["matched"].sum())


def _sums(terms, order):
    if order == "chunks":                                             # a running sum per chunk of CHUNK rows of the scan, then the chunks' sums in order from zero
        tot = np.zeros(SUMS, np.float64)
        for c0 in range(0, terms["v"].shape[0], CHUNK):
            part = {k: a[c0:c0 + CHUNK] for k, a in terms.items()}
            tot = tot + _sums(part, "forward")[0]
        return tot, int(terms["scored"].sum()), int(terms["matched"].sum())
    v = terms["v"][terms["scored"]]
    if order == "reverse":
        v = v[::-1]
    tot = np.zeros(SUMS, np.float64)
    for j in range(SUMS):
        tot[j] = np.add.accumulate(np.concatenate([[0.0], v[:, j]]))[-1]      # (a running sum from zero: one rounding per row)
    return tot, int(terms["scored"].sum()), int(terms["matched"].sum())


def info_matrix(h21):
    H = np.zeros((6, 6), np.float64)
    for j, (i, k) in enumerate(TRI):
        H[i, k] = H[k, i] = h21[j]
    return H


# ---- the damped solve and the retraction ---------------------------------------------------------------------------------------------------------------------------

def solve_damped(h21, g, lam):
    """delta of (H + lam diag(H)) delta = -g by a Cholesky factorisation in Python floats, or None when a pivot is not above PIVOT_REL x its diagonal entry."""
    A = [[float(v) for v in row] for row in info_matrix(h21)]
    lam = float(lam)
    for i in range(6):
        A[i][i] = A[i][i] + lam * A[i][i]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not (s > PIVOT_REL * abs(A[j][j])):
            return None
        l = math.sqrt(s)
        L[j][j] = l
        for i in range(j + 1, 6):
            u = A[i][j]
            for k in range(j):
                u = u - L[i][k] * L[j][k]
            L[i][j] = u / l
    yv = [0.0] * 6
    for i in range(6):
        u = -float(g[i])
        for k in range(i):
            u = u - L[i][k] * yv[k]
        yv[i] = u / L[i][i]
    delta = [0.0] * 6
    for i in range(5, -1, -1):
        u = yv[i]
        for k in range(i + 1, 6):
            u = u - L[k][i] * delta[k]
        delta[i] = u / L[i][i]
    return delta


def step_rotation(om):
    """E (3 x 3 nested lists): the rotation of pose_from_twist((0, om), 1) by the deskewer's series, or None when om . om > 1 or is not a number."""
    om = [float(v) for v in om]
    u = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]
    if not (u <= 1.0):
        return None
    A, B = float(dm.horner(dm.FA, u)), float(dm.horner(dm.FB, u))
    E = [[0.0] * 3 for _ in range(3)]
    for j in range(3):
        e = [0.0, 0.0, 0.0]; e[j] = 1.0
        c1 = _cross(om, e); c2 = _cross(om, c1)
        for a in range(3):
            E[a][j] = (e[a] + A * c1[a]) + B * c2[a]
    return E


def retract(R, t, delta):
    """(R', t') = (E(om) R, t + rho), or None for a failed step."""
    delta = [float(v) for v in delta]
    if not all(math.isfinite(v) for v in delta):
        return None
    E = step_rotation(delta[3:])
    if E is None:
        return None
    R = [[float(v) for v in row] for row in np.asarray(R).reshape(3, 3)]
    Q = np.array([[(E[a][0] * R[0][b] + E[a][1] * R[1][b]) + E[a][2] * R[2][b] for b in range(3)] for a in range(3)], np.float64)
    return Q, np.array([float(t[a]) + delta[a] for a in range(3)], np.float64)


def _norm2(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------------------------------------

class Query:
    """The state machine of one query: feed it the totals of pass 0 at the start pose, then of every trial pose it proposes (``trial``), until ``running`` is
    False or max_iters passes are done.  ``record()`` is the record after the last pass."""

    def __init__(self, start, P):
        self.P = P
        self.start = np.asarray(start, np.float32).reshape(4, 4).copy()
        self.status = ITERATION_CAP
        self.iterations = 0; self.accepted = 0
        self.delta = [0.0] * 6

    @property
    def running(self):
        return self.status == ITERATION_CAP

    def _propose(self):
        for _ in range(SOLVE_TRIES):
            d = solve_damped(self.v[7:], self.v[1:7], self.lam)
            q = retract(self.cur[0], self.cur[1], d) if d is not None else None
            if q is not None:
                self.delta = d; self.trial = q
                return
            self.lam = self.lam * LAMBDA_STEP
            if self.lam > LAMBDA_MAX:
                break
        self.status = STALLED

    def step(self, k, tot):
        v, scored, matched = tot
        P = self.P
        if k == 0:
            self.cur = pose64(self.start); self.trial = self.cur
            self.v = v.copy(); self.scored = scored; self.matched = matched
            self.lam = float(P["lambda0"]); self.cost_start = float(v[0])
            if not (np.isfinite(self.cur[0]).all() and np.isfinite(self.cur[1]).all()):
                self.status = BAD_POSE
            elif matched < P["min_matched"]:
                self.status = NO_OVERLAP
            elif P["max_iters"] > 0:
                self._propose()
            return
        assert self.running
        self.iterations = k
        F = float(v[0])
        if math.isfinite(F) and F < float(self.v[0]):
            self.cur = self.trial
            self.v = v.copy(); self.scored = scored; self.matched = matched; self.accepted += 1
            self.lam = max(self.lam / LAMBDA_STEP, LAMBDA_MIN)
            if _norm2(self.delta[:3]) <= float(P["tol_t"]) * float(P["tol_t"]) and _norm2(self.delta[3:]) <= float(P["tol_r"]) * float(P["tol_r"]):
                self.status = CONVERGED
        else:
            self.lam = self.lam * LAMBDA_STEP
            if self.lam > LAMBDA_MAX:
                self.status = STALLED
        if self.running and k < P["max_iters"]:
            self._propose()

    def record(self):
        pose = self.start.copy() if self.accepted == 0 else pose32(*self.cur)
        return dict(pose=pose, pose64=(np.array(self.cur[0]), np.array(self.cur[1])), info=self.v[7:].copy(), g=self.v[1:7].copy(), cost=float(self.v[0]),
                    cost_start=self.cost_start, rows_scored=self.scored, rows_matched=self.matched, iterations=self.iterations, accepted=self.accepted,
                    status=self.status, **{"lambda": self.lam})


def register(scan, pose, G, order="forward", **kw):
    """The whole loop for one scan from one start pose against the Gaussians G: the record as a dict."""
    P = params(**kw)
    q = Query(pose, P)
    ev = lambda R, t: totals(row_terms(scan, R, t, G, P["scale"], P["min_range"], P["max_range"]), order)
    q.step(0, ev(*pose64(pose)))
    for k in range(1, P["max_iters"] + 1):
        if not q.running:
            break
        q.step(k, ev(*q.trial))
    return q.record()


def cost(scan, R, t, G, **kw):
    """F alone at the float64 pose (R, t): for the central differences of the tests."""
    P = params(**kw)
    return totals(row_terms(scan, R, t, G, P["scale"], P["min_range"], P["max_range"]), "exact")[0][0]
