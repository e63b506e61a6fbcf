"""Exact reference for the point pass of a Gauss-Newton iteration (icet_amd/csrc/icet_accumulate.hip): per voxel the counts n2 (scan-2 points in the
voxel's angular bin) and m (those inside the cluster bounds) and the nine sums  S = sum d, sum d d^T  of  d = float32(q) - float32(mu1)  rounded to
float32, summed in EXACT arithmetic (Python integers on the float bit patterns).  tests/test_point_pass.py holds the raw accumulator records of the
device (icet_debug_point_sums_device) to it, voxel by voxel and word by word.

MEMBERSHIP is the oracle's restated decisions: cartesianToSpherical (pyoracle.c2s), sortSphericalCoordinates' voxel (pyoracle.voxel_of) and the six
comparisons of filterPointsInsideCluster in float32 against the keyframe's cluster bounds; a voxel takes part when the keyframe made it active
(has_fit, n1_raw > n, outer bound > 1: the scan-1 half of the gate at src/icet.cpp:290).

POSE.  The sums are checked at X = 0 with scan 2 moved on the host beforehand: the device's transform (x + t) R is then the identity in float32 --
apart from  -0 + (+0) = +0  and  inf * 0 = NaN, which transform() reproduces -- so no transform arithmetic enters the reference.  transform() also
restates the general float32 transform (fused multiply-adds, emulated exactly) for the count checks at X != 0.

THE BOUND.  Per voxel and word, with u = 2^-24 and the sums over the voxel's m in-bounds points:
    |device - exact| <= 8 u sum |d_i d_j| + m 2^-37          (sum d d^T)
    |device - exact| <= 8 u sum |d_i|     + m 2^-37          (sum d)
Why 7 terms per float partial sum (icet_accumulate.hip, phase C):  a lane holds 4 consecutive points.  Its run A is the maximal run of one slot that
starts at its point 0: at most 4 own points (a1 / a2 / a3).  In front of them come the points the PREVIOUS lane hands over by DPP (g1, g2, g3): that
lane's suffix run Z, the run of its point 3 -- and Z exists only when that lane's four points are NOT one run (z3 = !a3), so it holds at most points
1..3: 3 points.  A lane that receives passes nothing of it on (what it hands over is its own Z, which again excludes its point 0's run when all four
are one run: then z3 is false and nothing is handed over), so chains do not grow: 3 + 4 = 7 terms at most, in stream order.  The Z run flushed on its
own has <= 3 terms, a middle run <= 2, a parked point is a run of one.  A sum of products starts with one rounded product and takes one fused
multiply-add per further term: 7 roundings for 7 terms (6 for sum d, whose terms are exact floats); each rounding is at most u times the partial
result, itself at most (1 + 7u) sum |terms|: 7 u (1 + 7 u) < 8 u.  Every flushed value is then rounded ONCE to the 2^-36 grid (to_fix*, nearest:
at most 2^-37), and a voxel's in-bounds points make at most m flushes that carry a value.  Integer addition is exact, so nothing else enters.
"""
from fractions import Fraction

import numpy as np

U = Fraction(1, 1 << 24)
FIX_BITS = 36
HALF_FIX = Fraction(1, 1 << 37)
FIX_BIAS = 0x40F8000000000000                     # kFixBias (icet_device_common.h): the bit pattern of 1.5 * 2^16


# ---- float32 arithmetic, exactly ------------------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """float32 fma(a, b, c) of float32 arrays with ONE rounding.  a * b is exact in float64; the float64 sum p + c is rounded once more when it is cast to
    float32, which differs from the single rounding only when the float64 sum lies exactly half-way between two float32 values while the true sum does
    not: TwoSum gives the true sum's side."""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32); c = np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)                         # exact: true sum = s + err
        r = s.astype(np.float32)
        up = np.nextafter(r, np.float32(np.inf)).astype(np.float64); dn = np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
        r64 = r.astype(np.float64)
        fin = np.isfinite(s) & np.isfinite(up) & np.isfinite(dn) & (err != 0)
        at_up = fin & (s == 0.5 * (r64 + up)); at_dn = fin & (s == 0.5 * (r64 + dn))
        r = np.where(at_up & (err > 0), up.astype(np.float32), r)
        r = np.where(at_dn & (err < 0), dn.astype(np.float32), r)
    return r.astype(np.float32)


def transform(scan, X=None):
    """transform_point (icet_device_common.h) on an N x 3 float32 scan: (x + t) R with the fused multiply-adds written out.  X None or zero: R = 1."""
    s = np.ascontiguousarray(scan, np.float32)
    X = np.zeros(6, np.float32) if X is None else np.asarray(X, np.float32)
    if X[3:].any():
        from oracle import pyoracle as po
        R = po.euler_R(X[3:])                                     # the solver's rotation in float32, as the oracle builds it
    else:
        R = np.eye(3, dtype=np.float32)
    with np.errstate(all="ignore"):
        a = s[:, 0] + X[0]; b = s[:, 1] + X[1]; c = s[:, 2] + X[2]
        q = [fma32(c, np.full_like(c, R[2, k]), fma32(b, np.full_like(b, R[1, k]), a * R[0, k])) for k in range(3)]
    return np.stack(q, 1).astype(np.float32)


def exact_sum(x):
    """The exact sum of a float64 array as a Fraction (Python integers on the bit patterns)."""
    x = np.asarray(x, np.float64).ravel()
    x = x[x != 0]
    if x.size == 0:
        return Fraction(0)
    assert np.isfinite(x).all()
    mant, e = np.frexp(x)
    mi = np.ldexp(mant, 53).astype(np.int64)                      # |mant| in [0.5, 1): an exact 53-bit integer
    sh = (e.astype(np.int64) - 53); emin = int(sh.min()); sh -= emin
    tot = 0
    for m_, s_ in zip(mi.tolist(), sh.tolist()):
        tot += m_ << s_
    return Fraction(tot) * (Fraction(2) ** emin)


def fix_of(v):
    """round-half-even(v * 2^36) of a finite float, exactly."""
    return round(Fraction(float(v)) * (1 << FIX_BITS))          # (Python rounds a Fraction half to even)


# ---- membership and the exact sums ------------------------------------------------------------------------------------------------------

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))        # words 3..8: xx, xy, xz, yy, yz, zz


def keyframe_tables(src, n=25):
    """The keyframe tables the model needs, from the device's aux output (Context.solve(aux=True)) or from an oracle trace: bounds (V, 6), mu1 (V, 3)
    and which voxels are active."""
    bounds = np.asarray(src["cluster_bounds"] if "cluster_bounds" in src else src["bounds"], np.float32)
    has_fit = np.asarray(src["has_fit"]) == 1
    active = has_fit & (np.asarray(src["n1_raw"]) > n) & (bounds[:, 5] > 1)
    return dict(bounds=bounds, mu1=np.asarray(src["mu1"], np.float32), active=active)


def membership(q, kf, bins_phi, bins_theta):
    """Per point of the transformed scan q: its voxel, and whether it passes the voxel's cluster bounds (float32 comparisons)."""
    from oracle import pyoracle as po
    sph = po.c2s(q)
    vox = po.voxel_of(sph, bins_phi, bins_theta)
    b = kf["bounds"][vox]
    r, az, el = sph[:, 0], sph[:, 1], sph[:, 2]
    inb = (az >= b[:, 0]) & (az <= b[:, 1]) & (el >= b[:, 2]) & (el <= b[:, 3]) & (r >= b[:, 4]) & (r <= b[:, 5])
    return vox, inb


class Reference:
    """n2, m (V,) -- zero for voxels that are not active -- and per active voxel with m > 0: d (m, 3) float32, S[9] and A[9] (sums of the terms and of
    their absolute values, Fractions)."""

    def __init__(self, V):
        self.V = V
        self.n2 = np.zeros(V, np.int64); self.m = np.zeros(V, np.int64)
        self.d = {}; self.S = {}; self.A = {}

    def bound(self, v, k):
        return 8 * U * self.A[v][k] + int(self.m[v]) * HALF_FIX


def terms_of(d):
    """(m, 9) float64: the nine terms per point, each EXACT (a float32, or the product of two)."""
    d64 = d.astype(np.float64)
    return np.concatenate([d64, np.stack([d64[:, i] * d64[:, j] for i, j in PAIRS], 1)], 1)


def reference(scan2, kf, bins_phi, bins_theta, X=None, sums=True):
    """The exact per-voxel record of scan 2 (N x 3, any order: the sums are permutation-invariant) at pose X (sums: X = 0 only)."""
    q = transform(scan2, X)
    V = bins_phi * bins_theta
    vox, inb = membership(q, kf, bins_phi, bins_theta)
    ref = Reference(V)
    act = kf["active"]
    ref.n2 = np.where(act, np.bincount(vox, minlength=V)[:V], 0).astype(np.int64)
    ref.m = np.where(act, np.bincount(vox[inb], minlength=V)[:V], 0).astype(np.int64)
    if not sums:
        return ref
    assert X is None or not np.asarray(X).any(), "the sums are defined at X = 0 (move scan 2 on the host)"
    order = np.argsort(vox, kind="stable")
    sel = order[inb[order] & act[vox[order]]]
    vs = vox[sel]
    cuts = np.nonzero(np.diff(vs))[0] + 1
    for idx in np.split(sel, cuts) if sel.size else []:
        v = int(vox[idx[0]])
        with np.errstate(all="ignore"):
            d = (q[idx] - kf["mu1"][v]).astype(np.float32)         # float32 - float32, rounded to float32
        t = terms_of(d)
        ref.d[v] = d
        ref.S[v] = [exact_sum(t[:, k]) for k in range(9)]
        ref.A[v] = [exact_sum(np.abs(t[:, k])) for k in range(9)]
    return ref


def compare(rec, ref, label=""):
    """Hold a registration's dumped records (POINT_SUMS_DTYPE, one per voxel) to the reference: counts exactly, every word within the bound.  Returns
    (list of failure strings, worst error / bound ratio)."""
    bad = []
    worst = 0.0
    n2 = rec["n2"].astype(np.int64); m = rec["m"].astype(np.int64)
    for v in np.nonzero((n2 != ref.n2) | (m != ref.m))[0]:
        bad.append("%s voxel %d: counts (n2, m) = (%d, %d), reference (%d, %d)" % (label, v, n2[v], m[v], ref.n2[v], ref.m[v]))
    for v in range(ref.V):
        words = [int(w) for w in rec["sums"][v]]
        if ref.m[v] == 0:
            if any(words):
                bad.append("%s voxel %d: m = 0 but the sums are %s" % (label, v, words))
            continue
        for k in range(9):
            err = abs(Fraction(words[k], 1 << FIX_BITS) - ref.S[v][k]); bnd = ref.bound(v, k)
            worst = max(worst, float(err / bnd))
            if err > bnd:
                bad.append("%s voxel %d word %d: device %.9g, exact %.9g, |error| %.3g > bound %.3g (m = %d)"
                           % (label, v, k, words[k] / 2.0 ** FIX_BITS, float(ref.S[v][k]), float(err), float(bnd), ref.m[v]))
    return bad, worst


def moments(S, m, mu1):
    """mu2 and cov2 (packed xx, xy, xz, yy, yz, zz) from a voxel's sums by the formulas of icet_solve_body.h -- db = sd / m, mu2 = mu1 + db,
    cov = (sdd - m db db^T) / (m - 1) -- in exact arithmetic, as Fractions."""
    db = [S[k] / m for k in range(3)]
    mu2 = [Fraction(float(mu1[k])) + db[k] for k in range(3)]
    cov = [(S[3 + q] - m * db[i] * db[j]) / (m - 1) for q, (i, j) in enumerate(PAIRS)]
    return mu2, cov


def sym3(c):
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]], np.float64)


# ---- the device's arithmetic, emulated: float32 partial sums of <= 7 terms, each rounded to the 2^-36 grid ----------------------------------

def emulate_words(d, rng, max_run=7):
    """A voxel's nine fixed-point words as the point pass would form them for ONE random grouping of its points: a random order cut into runs of 1 ..
    max_run points, each run summed in float32 in order (sum d: additions; sum d d^T: one product, then fused multiply-adds), each run's value rounded
    half-even to a multiple of 2^-36, the integers added.  Returns nine Python integers."""
    m = d.shape[0]
    d = d[rng.permutation(m)]
    lens = []
    left = m
    while left > 0:
        k = int(min(left, rng.integers(1, max_run + 1))); lens.append(k); left -= k
    lens = np.asarray(lens); start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    g = lens.shape[0]
    acc = np.zeros((g, 9), np.float32)
    for j in range(max_run):
        live = lens > j
        p = d[np.minimum(start + j, m - 1)]
        for k in range(3):
            nxt = p[:, k] if j == 0 else (acc[:, k] + p[:, k]).astype(np.float32)
            acc[:, k] = np.where(live, nxt, acc[:, k])
        for q, (a, b) in enumerate(PAIRS):
            nxt = (p[:, a] * p[:, b]).astype(np.float32) if j == 0 else fma32(p[:, a], p[:, b], acc[:, 3 + q])
            acc[:, 3 + q] = np.where(live, nxt, acc[:, 3 + q])
    return [sum(fix_of(x) for x in acc[:, k].tolist()) for k in range(9)]
