"""NumPy model of the appearance search's rule (include/icet_hip.h "loop closure by appearance"; icet_amd/csrc/icet_appearance.h), written from the
rule's text alone: the cell and height code of a point, the descriptor and its column weights, the distance at every column shift, the candidate
order and the start pose of a shift.  tests/test_appearance.py holds the header (on the host) and the kernels (on the GPU) to it."""
import numpy as np

TWO_PI = 2.0 * np.pi
F = np.float32


class Params:
    """The parameters enable fixes, and the three constants the host derives in double and rounds to float32 once."""

    def __init__(self, sectors=120, rings=20, rho_max=80.0, z_lo=-3.0, z_hi=12.0):
        self.A, self.Rn = int(sectors), int(rings)
        self.rho_max, self.z_lo, self.z_hi = F(rho_max), F(z_lo), F(z_hi)
        self.kr = F(np.float64(self.Rn) / np.float64(self.rho_max))
        self.ka = F(np.float64(self.A) / TWO_PI)
        self.kz = F(254.0 / (np.float64(self.z_hi) - np.float64(self.z_lo)))

    def args(self):
        return [str(self.A), str(self.Rn), repr(float(self.rho_max)), repr(float(self.z_lo)), repr(float(self.z_hi))]


def cells(P, pts):
    """(valid, ring, sector, q) of the points (n, 3) float32; the last three are zero where a point does not count."""
    p = np.asarray(pts, F).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        rho2 = (x * x) + (y * y)                                        # float32, one rounding per operation
        rho = np.sqrt(rho2)
        t = rho * P.kr
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (rho2 > 0) & (t < F(P.Rn))
        ring = np.where(ok, np.floor(t), 0).astype(np.int64)
        az = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(F)
        u = (az * P.ka) + F(P.A // 2)
        sec = np.where(ok, np.floor(u), 0).astype(np.int64)
        sec = np.where(sec >= P.A, sec - P.A, sec)
        sec = np.maximum(sec, 0)
        zc = np.minimum(np.maximum(z, P.z_lo), P.z_hi)
        q = 1 + np.where(ok, np.floor((zc - P.z_lo) * P.kz), 0).astype(np.int64)
        q = np.clip(q, 1, 255)
    z0 = np.zeros_like(ring)
    return ok, np.where(ok, ring, z0), np.where(ok, sec, z0), np.where(ok, q, z0)


def weights(D):
    """Column weights: (float)(1 / sqrt((double)sum_r D[r][j]^2)), 0 for an empty column."""
    n = (np.asarray(D).astype(np.int64) ** 2).sum(0)
    with np.errstate(divide="ignore"):
        w = (1.0 / np.sqrt(n.astype(np.float64))).astype(F)
    return np.where(n > 0, w, F(0)).astype(F)


def descriptor(P, pts):
    """D (rings, sectors) uint8 and the column weights (sectors) float32 of a scan (n, 3)."""
    ok, ring, sec, q = cells(P, pts)
    D = np.zeros((P.Rn, P.A), np.int64)
    np.maximum.at(D, (ring[ok], sec[ok]), q[ok])
    D = D.astype(np.uint8)
    return D, weights(D)


def shift_distances(Dq, wq, Dc, wc):
    """d_s for every shift s (float32, +inf where fewer than ceil(A / 4) columns are valid)."""
    Dq = np.asarray(Dq).astype(np.int64); Dc = np.asarray(Dc).astype(np.int64)
    wq = np.asarray(wq, F); wc = np.asarray(wc, F)
    A = Dq.shape[1]
    d = np.empty(A, F)
    need = (A + 3) // 4
    for s in range(A):
        Dcs, wcs = np.roll(Dc, -s, axis=1), np.roll(wc, -s)             # column j of the roll is column (j + s) mod A
        G = (Dq * Dcs).sum(0)
        assert G.max(initial=0) < (1 << 24)
        c = (G.astype(F) * wq) * wcs                                    # float32, two roundings
        valid = (wq > 0) & (wcs > 0)
        m = int(valid.sum())
        if m < need:
            d[s] = np.inf
            continue
        total = np.cumsum(c[valid].astype(np.float64))[-1]              # left to right, ascending j
        v = F(1.0 - total / np.float64(m))
        d[s] = v if v >= 0 else F(0)
    return d


def distance(Dq, wq, Dc, wc):
    """(d, s): the smallest d_s, ties to the lowest s."""
    d = shift_distances(Dq, wq, Dc, wc)
    s = int(np.argmin(d))
    return d[s], s


def shift_yaw(s, A):
    """The yaw of the start pose of shift s, float32: (double)s (2 pi / A), minus 2 pi when above pi."""
    a = np.float64(s) * (TWO_PI / np.float64(A))
    if a > np.pi:
        a = a - TWO_PI
    return F(a)


def candidates(Dq, wq, slots, sq, max_distance, k, min_stamp_gap=0):
    """slots: {slot: (D, w, stamp)} of the occupied slots that have a descriptor.  Returns (cand, dist, shift, x0_base): the first k eligible slots in
    ascending (d, slot), -1 behind the last; +inf, -1 and zeros for a missing candidate."""
    found = []
    for slot in sorted(slots):
        D, w, stamp = slots[slot]
        d, s = distance(Dq, wq, D, w)
        if not (d <= F(max_distance)):
            continue
        if min_stamp_gap > 0 and abs(int(sq) - int(stamp)) < int(min_stamp_gap):
            continue
        found.append((F(d).view(np.uint32).item(), slot, d, s))
    found.sort(key=lambda t: (t[0], t[1]))
    A = np.asarray(Dq).shape[1]
    cand = np.full(k, -1, np.int32); dist = np.full(k, np.inf, F); shift = np.full(k, -1, np.int32); x0 = np.zeros((k, 6), F)
    for i, (_, slot, d, s) in enumerate(found[:k]):
        cand[i], dist[i], shift[i] = slot, d, s
        x0[i, 5] = shift_yaw(s, A)
    return cand, dist, shift, x0
