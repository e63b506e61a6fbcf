"""The neighbourhood rule of the registration against a shaped voxel map (include/icet_hip.h ICET_VOXEL_MAP_REG_NEIGHBOURS_*) in NumPy, on
top of tests/map_register_model.py and written from the rule, not from the header: a scored row looks at the cells of its neighbourhood in a fixed order -- N1 its
own cell; N7 own, -x, +x, -y, +y, -z, +z; N27 own, then the other 26 offsets with dx slowest, each over -1, 0, 1 -- skips the cells outside the grid and the cells
without a usable Gaussian, computes s = d . W d against each of the rest in the order of operations of a row's terms, and is scored against the cell with the
smallest s: ``best`` starts at +infinity and a cell wins iff s < best, so a tie stays with the earlier cell and a NaN or an infinite s never wins.  The terms of
the row are map_register_model's terms against the winner's Gaussian; a row without a winner is a miss.  The totals, the solve and the loop are the model's own."""
import numpy as np

import map_model as mm
import map_register_model as rm

FIELD = (1 << 21) - 1
N7 = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
N27 = [(0, 0, 0)] + [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
OFFSETS = {1: [(0, 0, 0)], 7: N7, 27: N27}
FLAGS = {1: 0, 7: 2, 27: 4}


class _Chosen:
    """The Gaussians of G with the look-up answered in advance: row i of a scan finds entry idx[i] if has[i]."""

    def __init__(self, G, idx, has):
        self.cell, self.key, self.mu, self.W = G.cell, G.key, G.mu, G.W
        self._idx, self._has = idx, has

    def find(self, key):
        return self._idx, self._has


def select(scan, R, t, G, neighbours, own):
    """Per row the place of the winning cell in the order of the neighbourhood (-1: none), the entry of G it is, and every candidate's s (N, K; NaN where the
    place holds no candidate).  ``own``: map_register_model.row_terms of the same rows (its classes and keys)."""
    p = np.asarray(scan, np.float32).reshape(-1, 3).astype(np.float64)
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    n = p.shape[0]
    offs = OFFSETS[neighbours]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    kept = own["cls"] == mm.KEPT
    key = np.where(kept, own["key"], np.uint64(0))
    f = [((key >> np.uint64(s)) & np.uint64(FIELD)).astype(np.int64) for s in (42, 21, 0)]
    place = np.full(n, -1, np.int64); entry = np.zeros(n, np.int64)
    best = np.full(n, np.inf)
    cand = np.full((n, len(offs)), np.nan)
    with np.errstate(all="ignore"):
        w = [((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + t[a] for a in range(3)]
        for j, d in enumerate(offs):
            g = [f[a] + d[a] for a in range(3)]
            inside = kept & np.logical_and.reduce([(g[a] >= 1) & (g[a] <= FIELD) for a in range(3)])
            gg = [np.where(inside, g[a], 0).astype(np.uint64) for a in range(3)]
            idx, found = G.find((gg[0] << np.uint64(42)) | (gg[1] << np.uint64(21)) | gg[2])
            usable = found & inside
            if G.key.shape[0] == 0:
                continue
            mu, W = G.mu[idx], G.W[idx]
            dd = [w[a] - mu[:, a] for a in range(3)]
            Wf = [[W[:, 0], W[:, 1], W[:, 2]], [W[:, 1], W[:, 3], W[:, 4]], [W[:, 2], W[:, 4], W[:, 5]]]
            a_ = [(Wf[i][0] * dd[0] + Wf[i][1] * dd[1]) + Wf[i][2] * dd[2] for i in range(3)]
            s = (dd[0] * a_[0] + dd[1] * a_[1]) + dd[2] * a_[2]
            cand[usable, j] = s[usable]
            win = usable & (s < best)
            best = np.where(win, s, best); place[win] = j; entry[win] = idx[win]
    return place, entry, cand


def row_terms(scan, R, t, G, neighbours=1, scale=11.3449, min_range=0.0, max_range=0.0):
    """map_register_model.row_terms under a neighbourhood of 1, 7 or 27 cells: the same dict (key is still the row's own cell), and ``place``: the winner's place
    in the order, -1 for a row without one; the record's ``matched`` word is place + 1."""
    own = rm.row_terms(scan, R, t, G, scale, min_range, max_range)
    place, entry, cand = select(scan, R, t, G, neighbours, own)
    tm = rm.row_terms(scan, R, t, _Chosen(G, entry, place >= 0), scale, min_range, max_range)
    assert np.array_equal(tm["cls"], own["cls"]) and np.array_equal(tm["key"], own["key"]) and np.array_equal(tm["matched"], place >= 0)
    tm["place"] = place; tm["cand"] = cand
    return tm


def register(scan, pose, G, neighbours=1, order="forward", **kw):
    """map_register_model.register with the rows scored under the neighbourhood."""
    P = rm.params(**kw)
    q = rm.Query(pose, P)
    ev = lambda R, t: rm.totals(row_terms(scan, R, t, G, neighbours, P["scale"], P["min_range"], P["max_range"]), order)
    q.step(0, ev(*rm.pose64(pose)))
    for k in range(1, P["max_iters"] + 1):
        if not q.running:
            break
        q.step(k, ev(*q.trial))
    return q.record()


def cost(scan, R, t, G, neighbours=1, **kw):
    P = rm.params(**kw)
    return rm.totals(row_terms(scan, R, t, G, neighbours, P["scale"], P["min_range"], P["max_range"]), "exact")[0][0]
