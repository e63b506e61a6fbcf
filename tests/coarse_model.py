"""NumPy model of the coarse alignment's rule (include/icet_hip.h "coarse alignment"; icet_amd/csrc/icet_coarse.h), written from the rule's text alone: the
cell and height code of a point, the spanning cells, the grid of a scan under a yaw hypothesis, the score of every shift, the order of the winners and the
start pose of one.  tests/test_coarse.py holds the header (on the host) and the kernels (on the GPU) to it."""
import numpy as np

import closure_model as cm

F = np.float32
D = np.float64
PI = D(3.141592653589793)
MAX_WINDOW = 32


class Params:
    """The parameters enable fixes, and what the host derives from them in double."""

    def __init__(self, cells=256, cell=0.25, z_lo=-3.0, z_hi=12.0, min_span=0.5):
        self.G, self.W = int(cells), int(cells) // 32
        self.cell, self.z_lo, self.z_hi, self.min_span = F(cell), F(z_lo), F(z_hi), F(min_span)
        kz = D(254.0) / (D(self.z_hi) - D(self.z_lo))
        self.kc = F(D(1.0) / D(self.cell))
        self.kz = F(kz)
        self.span_codes = int(np.ceil(D(self.min_span) * kz))

    def args(self):
        return [str(self.G), repr(float(self.cell)), repr(float(self.z_lo)), repr(float(self.z_hi)), repr(float(self.min_span))]


def coord_cell(P, v):
    """(inside, index) of float32 coordinates: u = fl(fl(v kc) + G / 2), inside when 0 <= u < G (a NaN is outside), index floor(u)."""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        u = (v * P.kc) + F(P.G // 2)
        ok = (u >= 0) & (u < F(P.G))
        i = np.where(ok, np.floor(u), 0).astype(np.int64)
    return ok, i


def count_points(P, pts):
    """(counts, ix, iy, q) of the points (n, 3) float32; the last three are zero where a point does not count."""
    p = np.asarray(pts, F).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        rho2 = (x * x) + (y * y)
        okx, ix = coord_cell(P, x)
        oky, iy = coord_cell(P, y)
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (rho2 > 0) & okx & oky
        zc = np.minimum(np.maximum(z, P.z_lo), P.z_hi)
        q = np.where(ok, np.floor((zc - P.z_lo) * P.kz), 0).astype(np.int64)
    z0 = np.zeros_like(ix)
    return ok, np.where(ok, ix, z0), np.where(ok, iy, z0), np.where(ok, q, z0)


def spanning(P, pts):
    """The (G, G) bool array of the cells that span: largest minus smallest code of the counting points >= span_codes."""
    ok, ix, iy, q = count_points(P, pts)
    lo = np.full((P.G, P.G), 1 << 30, np.int64); hi = np.full((P.G, P.G), -1, np.int64)
    np.minimum.at(lo, (ix[ok], iy[ok]), q[ok])
    np.maximum.at(hi, (ix[ok], iy[ok]), q[ok])
    return (hi >= 0) & (hi - lo >= P.span_codes)


def structure(P, pts):
    """Which points are structure points: counting points whose own cell spans."""
    ok, ix, iy, _ = count_points(P, pts)
    return ok & spanning(P, pts)[ix, iy]


def words(cells):
    """A (G, G) bool grid as (G, G / 32) uint32 words: bit iy & 31 of word iy >> 5 of row ix."""
    c = np.asarray(cells, bool)
    G = c.shape[0]
    w = (c.reshape(G, G // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(2)
    return w.astype(np.uint32)


def unwords(w):
    w = np.asarray(w, np.uint32)
    G = w.shape[0]
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(G, G)


def keyframe_grid(P, pts):
    """A keyframe's grid: the identity transform, so exactly its spanning cells."""
    return spanning(P, pts)


def n_hypotheses(Y, half_turn):
    return (2 if half_turn else 1) * (2 * Y + 1)


def hypothesis_of(h, Y):
    """(y, f) of hypothesis h = f (2 Y + 1) + (y + Y)."""
    return h % (2 * Y + 1) - Y, h // (2 * Y + 1)


def hypothesis_rotation(X0, y, f, yaw_step):
    """R_h = R(X0) Rz(delta_h) in double, delta_h = (double)y yaw_step + f pi, sums left to right."""
    X0 = np.asarray(X0, F)
    delta = D(y) * D(F(yaw_step)) + D(f) * PI
    R0 = cm.euler_R(D(X0[3]), D(X0[4]), D(X0[5]))
    Rz = cm.euler_R(D(0.0), D(0.0), delta)
    Rh = np.empty((3, 3), D)
    for a in range(3):
        for b in range(3):
            Rh[a, b] = (R0[a, 0] * Rz[0, b] + R0[a, 1] * Rz[1, b]) + R0[a, 2] * Rz[2, b]
    return Rh


def transform_xy(Rh, X0, pts):
    """x', y' (float32) of the points: M = R_h^T rounded to float32, u = fl(p + X0_t), x' = fl(fl(fl(M00 ux) + fl(M01 uy)) + fl(M02 uz))."""
    M = Rh.T.astype(F)
    p = np.asarray(pts, F).reshape(-1, 3)
    t = np.asarray(X0, F)[:3]
    with np.errstate(all="ignore"):
        ux, uy, uz = p[:, 0] + t[0], p[:, 1] + t[1], p[:, 2] + t[2]
        xo = ((M[0, 0] * ux) + (M[0, 1] * uy)) + (M[0, 2] * uz)
        yo = ((M[1, 0] * ux) + (M[1, 1] * uy)) + (M[1, 2] * uz)
    return xo, yo


def live_grid(P, pts, X0, y, f, yaw_step, st=None):
    """The (G, G) bool grid of a live scan under hypothesis (y, f): the cells its structure points hit after the transform."""
    st = structure(P, pts) if st is None else st
    xo, yo = transform_xy(hypothesis_rotation(X0, y, f, yaw_step), X0, np.asarray(pts, F).reshape(-1, 3)[st])
    okx, jx = coord_cell(P, xo)
    oky, jy = coord_cell(P, yo)
    ok = okx & oky
    g = np.zeros((P.G, P.G), bool)
    g[jx[ok], jy[ok]] = True
    return g


def scores(live, key, window):
    """S(a, b) for |a|, |b| <= window as a (2 window + 1)^2 int array indexed [a + window, b + window]: the live cells (i, j) whose key cell (i + a, j + b) is set."""
    G, M = live.shape[0], int(window)
    pad = np.zeros((G + 2 * M, G + 2 * M), bool)
    pad[M:M + G, M:M + G] = key
    li, lj = np.nonzero(live)
    S = np.zeros((2 * M + 1, 2 * M + 1), np.int64)
    for a in range(-M, M + 1):
        for b in range(-M, M + 1):
            S[a + M, b + M] = int(pad[li + a + M, lj + b + M].sum())
    return S


def shift_key(score, a, b, h):
    """The order of the winners as one integer whose maximum wins: largest S; then smallest a a + b b; then smallest h, a, b."""
    return (int(score) << 32) | ((4095 - (a * a + b * b)) << 20) | ((63 - h) << 14) | ((MAX_WINDOW - a) << 7) | (MAX_WINDOW - b)


def best_shift(S, window, h):
    """The largest key of one hypothesis, and its (score, a, b)."""
    M = int(window)
    best = None
    top = S.max()
    for a, b in zip(*np.nonzero(S == top)):                            # (only a largest score can win)
        k = shift_key(top, int(a) - M, int(b) - M, h)
        if best is None or k > best[0]:
            best = (k, int(top), int(a) - M, int(b) - M)
    return best


def shift_code(a, b, h):
    return h | ((a + MAX_WINDOW) << 8) | ((b + MAX_WINDOW) << 16)


def start_pose(P, X0, Rh, a, b, y, f):
    """The start pose of the winner (a, b) of R_h: X_t = X0_t + R_h d, d = ((double)a cell, (double)b cell, 0); angles of R_h, -pi becoming pi; float32.
    Where nothing moves the value is X0's own: the translation when a = b = 0, the angles when y = 0 and f = 0."""
    X0 = np.asarray(X0, F)
    d = [D(a) * D(P.cell), D(b) * D(P.cell), D(0.0)]
    X = np.empty(6, F)
    for k in range(3):
        t = (Rh[k, 0] * d[0] + Rh[k, 1] * d[1]) + Rh[k, 2] * d[2]
        X[k] = X0[k] if (a == 0 and b == 0) else F(D(X0[k]) + t)
    ang = cm.euler_of(Rh)
    for k in range(3):
        v = ang[k]
        if v <= -PI:
            v = v + D(2.0) * PI
        X[3 + k] = X0[3 + k] if (y == 0 and f == 0) else F(v)
    return X


def search(P, pts, X0, key, window, Y, yaw_step, half_turn, min_score=1):
    """The whole search of one candidate.  key: the slot's (G, G) bool grid, or None when the slot has none.  Returns dict(score, a, b, h, live_bits, key_bits,
    found, x0): the match record and the start pose (X0 itself where found = 0)."""
    X0 = np.asarray(X0, F)
    if key is None:
        return dict(score=0, a=0, b=0, h=0, live_bits=0, key_bits=0, found=0, x0=X0.copy())
    st = structure(P, pts)
    best = None
    for h in range(n_hypotheses(Y, half_turn)):
        y, f = hypothesis_of(h, Y)
        live = live_grid(P, pts, X0, y, f, yaw_step, st)
        k, s, a, b = best_shift(scores(live, key, window), window, h)
        if best is None or k > best[0]:
            best = (k, s, a, b, h, int(live.sum()))
    _, s, a, b, h, lb = best
    found = int(s >= min_score)
    y, f = hypothesis_of(h, Y)
    x0 = start_pose(P, X0, hypothesis_rotation(X0, y, f, yaw_step), a, b, y, f) if found else X0.copy()
    return dict(score=s, a=a, b=b, h=h, live_bits=lb, key_bits=int(np.asarray(key).sum()), found=found, x0=x0)
