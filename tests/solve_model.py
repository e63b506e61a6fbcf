"""The per-voxel algebra of one Gauss-Newton iteration (gn_solve_body, icet_amd/csrc/icet_solve_body.h; its second copy in k_gn_score, icet_score.hip), restated
in NumPy in the device's own expression order.  It calls nothing in the library.  Fed with the device's OWN integer accumulator words and the device's OWN SlotFit
records (icet_debug_gn_terms_device), a voxel's 21 + 6 float32 terms are the device's bit for bit; the reduction over slots, waves and virtual blocks is held to a
rounding bound derived from the source (tests/test_voxel_algebra.py).

ARITHMETIC.  The 64-bit words become doubles with one rounding (int64 -> float64), times 2^-36 (exact).  rfm = 1.0 / m, den = 1.0 / (m - 1), db = sd rfm,
mu2 = mu1 + db and cov2 = (sdd - m db db^T) den are formed in float64, every operation rounded on its own, and rounded once to float32 -- lines 331-340 of the
source.  Everything behind them is float32 with every product and every sum rounded on its own (the source stands under `contract(off)`), sums of three taken left
to right.  NumPy's float32 array operations round each operation to float32, so the expressions below are written operation by operation over arrays of voxels.

THE WEIGHT.  By default W is the float CompleteOrthogonalDecomposition pseudo-inverse of the nine-entry Rp9 = (M Rn) M^T -- oracle.pyoracle.pinv, bit-identical to
the device's cod_pinv3_lane (tests/test_gpu_parity.py::test_pinv3_reference_bits) -- and W H uses all nine entries.  Under FLAG_DOUBLE_W it is pinv3_sym_fast of
the packed Rp, restated here in float64 operation by operation (that function stands outside contract(off): where the compiler fuses a product into a sum the
double intermediate moves by 2^-53 relative, which reaches the float32 result only when it lies that close to a rounding boundary).

THE REDUCTION BOUND.  A term is a float32; the device adds the terms of a registration in float32 in a fixed tree.  An addition whose partial sum is s is off by at
most u |s|, u = 2^-24, so a tree in which no term passes through more than D additions stays within ((1 + u)^D - 1) sum |term| of the exact sum.  D from the
source:
    256-thread form (kT = 256, grids of <= 4096 voxels):   slot s lives on thread s % 256, which adds it to its S in round s / 256: a term entering in round 0
        passes through all R = ceil(n_slots / 256) of the thread's additions.  Then wave_total: an inclusive scan of six DPP steps (row_shr 1, 2, 4, 8, row_bcast 15,
        31), one addition each.  Then lane < 27 adds the 4 wave totals to t = 0 in wave order: 4 additions.           D = R + 6 + 4
    canonical 512-slot form (kT = 512), the same tree in its three launch forms (stage 1 + 2 from partials; one block; stage 2 doing the whole solve behind a
        drain):  per virtual block the thread's S = 0 + term (1), six DPP steps, the 8 wave totals added to t = 0 in wave order (8), and the NVB =
        ceil(n_slots / 512) virtual blocks added to t = 0 in index order.                                               D = 1 + 6 + 8 + NVB
    In both forms at least two of the counted additions are exact (0 + x: the thread's first, and the first wave total's), so at most D - 2 round, and
    (1 + u)^(D - 2) - 1 < D u for every D < 2^22.  bound = D 2^-24 sum |term|, a condition derived from the source and not a measurement.

THE FLOAT64 COMPARISON.  From db, mu2, M, J and a fixed W the float32 terms differ from the same formulas in float64 by roundings only.  Count them on the deepest
path (every sum of three is product, +, +: a product on it meets at most 3 roundings):  Hj 3;  Hz (columns 3-5) 3 + 3 = 6, (columns 0-2) 0: -M is exact;  W H 3 more:
9, resp. 3;  a term of H^T W H  Hz[a] WH[b]:  6 + 9 + 3 = 18;  dz 3;  a term of H^T W dz  WH[a] dz:  9 + 3 + 3 = 15.  (1 + u)^18 - 1 < 19 u and (1 + u)^15 - 1 < 16 u:
    |term32 - term64| <= c u P,   c = 19 (H^T W H), 16 (H^T W dz),   P = the same formulas evaluated on absolute values ("sum |products|").
"""
import math
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24
FIX_INV = 2.0 ** -36
FLAG_REJECT_MOVING = 4
FLAG_DOUBLE_W = 32
REJECT_THRESH = np.float32(0.3)                   # kRejectMovingThresh
REJECT_START_ITER = 4                             # kRejectMovingStartIter
C_HTWH, C_HTWDZ = 19, 16

FIT_DTYPE = np.dtype([("mu", "<f4", (3,)), ("s1n", "<f4", (6,)), ("M", "<f4", (9,)), ("n1", "<i4"), ("v", "<i4")])      # SlotFit, 80 bytes
assert FIT_DTYPE.itemsize == 80
TRI = [(a, b) for a in range(6) for b in range(a, 6)]                 # the 21 packed entries of H^T W H, in the source's order
F32 = np.float32


# ---- records -------------------------------------------------------------------------------------------------------------------------------

def fit_from_words(words):
    """(n_slots, 20) uint32 words of SlotFit (KeyframeStore.debug_fetch(slot, "fit")) -> FIT_DTYPE records."""
    return np.frombuffer(np.ascontiguousarray(words, np.uint32).tobytes(), FIT_DTYPE).copy()


def fit_from_tables(mu1, sigma1, evecs1, l_diag, n1_raw, voxels):
    """SlotFit records rebuilt from a solve's aux outputs (or an oracle trace's keyframe tables) for the given voxels: s1n = sigma1 / float32(n1_raw - 1) (upper
    triangle xx xy xz yy yz zz), M = diag(l_diag) evecs1."""
    v = np.asarray(voxels, np.int64)
    f = np.zeros(v.shape[0], FIT_DTYPE)
    f["mu"] = np.asarray(mu1, F32)[v]
    s = np.asarray(sigma1, F32).reshape(-1, 9)[v]
    d1 = (np.asarray(n1_raw)[v] - 1).astype(F32)
    with np.errstate(all="ignore"):
        f["s1n"] = s[:, [0, 1, 2, 4, 5, 8]] / d1[:, None]
        f["M"] = (np.asarray(l_diag, F32)[v][:, :, None] * np.asarray(evecs1, F32).reshape(-1, 3, 3)[v]).reshape(-1, 9)
    f["n1"] = np.asarray(n1_raw)[v]; f["v"] = v
    return f


def xf_record(X):
    """write_xf's transform record (48 floats: t | R | angles | pad | J[27]) with every product and sum rounded on its own.  The device's record may differ in last
    bits where the compiler fuses (write_xf stands outside contract(off)): the GPU tests take J from the device and hold the record to its own bound."""
    X = np.asarray(X, F32)
    s = [F32(math.sin(float(a))) for a in X[3:]]; c = [F32(math.cos(float(a))) for a in X[3:]]
    sph, sth, sps = s; cph, cth, cps = c
    xf = np.zeros(48, F32)
    xf[0:3] = X[0:3]
    xf[3] = cth * cps; xf[4] = sps * cph + sph * sth * cps; xf[5] = sph * sps - sth * cph * cps
    xf[6] = -sps * cth; xf[7] = cph * cps - sph * sth * sps; xf[8] = sph * cps + sth * sps * cph
    xf[9] = sth; xf[10] = -sph * cth; xf[11] = cph * cth
    xf[12:15] = X[3:6]
    J = xf[16:]
    J[1] = -sps * sph + cph * sth * cps; J[2] = cph * sps + sth * sph * cps
    J[4] = -sph * cps - cph * sth * sps; J[5] = cph * cps - sth * sps * sph
    J[7] = -cph * cth; J[8] = -sph * cth
    J[9] = -sth * cps; J[10] = cth * sph * cps; J[11] = -cth * cph * cps
    J[12] = sps * sth; J[13] = -cth * sph * sps; J[14] = cth * sps * cph
    J[15] = cth; J[16] = sph * sth; J[17] = -sth * cph
    J[18] = -cth * sps; J[19] = cps * cph - sph * sth * sps; J[20] = cps * sph + sth * cph * sps
    J[21] = -cps * cth; J[22] = -sps * cph - sph * sth * cps; J[23] = -sph * sps + sth * cps * cph
    return xf


XF_ZERO = (15, 16, 19, 22, 40, 41, 42)            # the entries write_xf sets to zero: the pad, J[0], J[3], J[6], J[24..26]


def xf_reference(X):
    """For the transform-record test: the float32-rounded sines and cosines of the float32 angles (correctly rounded from double), and per R / J entry the float64
    value of write_xf's formula on them with the sum of the absolute products.  Returns (sincos[6] float32 = sph cph sth cth sps cps, value[48], absprod[48])."""
    X = np.asarray(X, F32)
    sc = []
    for a in X[3:]:
        sc += [F32(math.sin(float(a))), F32(math.cos(float(a)))]
    sph, cph, sth, cth, sps, cps = [float(x) for x in sc]
    P = {}                                          # index -> list of signed products
    P[3] = [cth * cps]; P[4] = [sps * cph, sph * sth * cps]; P[5] = [sph * sps, -sth * cph * cps]
    P[6] = [-sps * cth]; P[7] = [cph * cps, -sph * sth * sps]; P[8] = [sph * cps, sth * sps * cph]
    P[9] = [sth]; P[10] = [-sph * cth]; P[11] = [cph * cth]
    j = 16
    P[j + 1] = [-sps * sph, cph * sth * cps]; P[j + 2] = [cph * sps, sth * sph * cps]
    P[j + 4] = [-sph * cps, -cph * sth * sps]; P[j + 5] = [cph * cps, -sth * sps * sph]
    P[j + 7] = [-cph * cth]; P[j + 8] = [-sph * cth]
    P[j + 9] = [-sth * cps]; P[j + 10] = [cth * sph * cps]; P[j + 11] = [-cth * cph * cps]
    P[j + 12] = [sps * sth]; P[j + 13] = [-cth * sph * sps]; P[j + 14] = [cth * sps * cph]
    P[j + 15] = [cth]; P[j + 16] = [sph * sth]; P[j + 17] = [-sth * cph]
    P[j + 18] = [-cth * sps]; P[j + 19] = [cps * cph, -sph * sth * sps]; P[j + 20] = [cps * sph, sth * cph * sps]
    P[j + 21] = [-cps * cth]; P[j + 22] = [-sps * cph, -sph * sth * cps]; P[j + 23] = [-sph * sps, sth * cps * cph]
    val = np.zeros(48); ab = np.zeros(48)
    for k, pr in P.items():
        val[k] = sum(pr); ab[k] = sum(abs(x) for x in pr)
    return np.asarray(sc, F32), val, ab


# ---- the per-voxel weight ------------------------------------------------------------------------------------------------------------------

def _jacobi_pinv3(a, rel_tol):
    """pinv3_sym<double> (icet_device_math.h): cyclic Jacobi in float64 on one packed symmetric matrix."""
    A00, A01, A02, A11, A12, A22 = [float(x) for x in a]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    A = {(0, 0): A00, (0, 1): A01, (0, 2): A02, (1, 1): A11, (1, 2): A12, (2, 2): A22}

    def g(i, j):
        return A[(min(i, j), max(i, j))]

    def st(i, j, x):
        A[(min(i, j), max(i, j))] = x

    def rot(p, q, r):
        apq = g(p, q)
        if apq == 0.0:
            return
        theta = (g(q, q) - g(p, p)) / (2.0 * apq)
        t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
        c = 1.0 / math.sqrt(t * t + 1.0); s = t * c
        app = g(p, p) - t * apq; aqq = g(q, q) + t * apq
        apr = c * g(p, r) - s * g(q, r); aqr = s * g(p, r) + c * g(q, r)
        st(p, p, app); st(q, q, aqq); st(p, q, 0.0); st(p, r, apr); st(q, r, aqr)
        for k in range(3):
            v = c * V[k][p] - s * V[k][q]; V[k][q] = s * V[k][p] + c * V[k][q]; V[k][p] = v
    for _ in range(10):
        off = abs(g(0, 1)) + abs(g(0, 2)) + abs(g(1, 2)); dg = abs(g(0, 0)) + abs(g(1, 1)) + abs(g(2, 2))
        if off <= 1e-17 * dg:
            break
        rot(0, 1, 2); rot(0, 2, 1); rot(1, 2, 0)
    lmax = max(abs(g(0, 0)), abs(g(1, 1)), abs(g(2, 2)))
    thr = float(F32(rel_tol)) * lmax
    inv = [1.0 / g(k, k) if abs(g(k, k)) > thr else 0.0 for k in range(3)]
    w = []
    for (r, s_) in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        w.append(F32(inv[0] * V[r][0] * V[s_][0] + inv[1] * V[r][1] * V[s_][1] + inv[2] * V[r][2] * V[s_][2]))
    return np.asarray(w, F32)


def pinv3_sym_fast(a, rel_tol=3.0 * 2.0 ** -23):
    """pinv3_sym_fast (icet_device_math.h) on one packed symmetric float32 matrix (xx xy xz yy yz zz), in float64 operation by operation."""
    a = np.asarray(a, F32)
    if not np.isfinite(a).all():
        return _jacobi_pinv3(a, rel_tol)
    a00, a01, a02, a11, a12, a22 = [float(x) for x in a]
    z0, z1, z2 = a[0] == 0, a[3] == 0, a[5] == 0
    fill = max(max(a00, a11), a22)
    if z0:
        a00 = fill
    if z1:
        a11 = fill
    if z2:
        a22 = fill
    clean = (not z0 or (a[1] == 0 and a[2] == 0)) and (not z1 or (a[1] == 0 and a[4] == 0)) and (not z2 or (a[2] == 0 and a[4] == 0))
    c00 = a11 * a22 - a12 * a12; c01 = a02 * a12 - a01 * a22; c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02; c12 = a01 * a02 - a00 * a12; c22 = a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    if clean and fill > 0.0 and det > 0.0:
        rd = 1.0 / det
        i00, i01, i02, i11, i12, i22 = c00 * rd, c01 * rd, c02 * rd, c11 * rd, c12 * rd, c22 * rd
        fa = a00 * a00 + a11 * a11 + a22 * a22 + 2.0 * (a01 * a01 + a02 * a02 + a12 * a12)
        fi = i00 * i00 + i11 * i11 + i22 * i22 + 2.0 * (i01 * i01 + i02 * i02 + i12 * i12)
        if fa * fi <= 1e12:
            z = F32(0)
            return np.asarray([z if z0 else F32(i00), z if (z0 or z1) else F32(i01), z if (z0 or z2) else F32(i02),
                               z if z1 else F32(i11), z if (z1 or z2) else F32(i12), z if z2 else F32(i22)], F32)
    return _jacobi_pinv3(a, rel_tol)


def _cod_pinv(Rp9):
    from oracle import pyoracle as po
    return po.pinv(np.asarray(Rp9, F32).reshape(3, 3))[0].reshape(9)


# ---- the per-voxel terms -------------------------------------------------------------------------------------------------------------------

def _dot3(a0, b0, a1, b1, a2, b2):
    """a0 b0 + a1 b1 + a2 b2 in float32, every operation rounded, left to right."""
    return (a0 * b0 + a1 * b1) + a2 * b2


def voxel_terms(words, n2, m, fit, J, flags=0, n=25, iter=0, W9=None, _fault=None):
    """N voxels at once.  words (N, 9) int64, n2 / m (N,), fit (N,) FIT_DTYPE, J (27,) float32.  Returns a dict: terms (N, 27) float32 = the 21 packed entries of
    H^T W H and the 6 of H^T W dz (zero rows for voxels that do not contribute), dz (N, 3), W9 (N, 9), q (N,) float64 = dz^T W dz, used (N,) bool, and the
    intermediates db, mu2, Rp (packed), Rp9.  W9: a fixed weight to use instead of computing one.  _fault (the checker's own test): ("swap_counts", i) evaluates
    voxel i with n2 and m exchanged, ("transpose_hz", i) reads Hz[6 r + c] of voxel i's rotational block as Hz[6 (c - 3) + r + 3]."""
    words = np.asarray(words, np.int64).reshape(-1, 9); N = words.shape[0]
    n2 = np.asarray(n2, np.int64).copy(); m = np.asarray(m, np.int64).copy()
    if _fault and _fault[0] == "swap_counts":
        i = _fault[1]; n2[i], m[i] = m[i], n2[i]
    J = np.asarray(J, F32).reshape(27)
    gate = (n2 > n) & (m > n)
    ms = np.where(gate, m, 2).astype(np.float64)                    # (a harmless divisor where the voxel is gated off)
    with np.errstate(all="ignore"):
        sD = words.astype(np.float64) * FIX_INV
        rfm = 1.0 / ms
        dbD = sD[:, :3] * rfm[:, None]
        db = dbD.astype(F32)
        mu = fit["mu"].astype(F32)
        mu2 = (mu.astype(np.float64) + dbD).astype(F32)
        den = 1.0 / (ms - 1.0)
        d2 = np.where(gate, n2 - 1, 1).astype(F32)
        prs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        cov2 = np.stack([((sD[:, 3 + k] - ms * dbD[:, i] * dbD[:, j]) * den).astype(F32) for k, (i, j) in enumerate(prs)], 1)
        Rn = fit["s1n"].astype(F32) + cov2 / d2[:, None]
        M = fit["M"].astype(F32)
        dz = np.stack([_dot3(M[:, 3 * i], db[:, 0], M[:, 3 * i + 1], db[:, 1], M[:, 3 * i + 2], db[:, 2]) for i in range(3)], 1)
        used = gate.copy()
        if (flags & FLAG_REJECT_MOVING) and iter >= REJECT_START_ITER:
            used &= ~(np.abs(dz) > REJECT_THRESH).any(1)
        MR = np.zeros((N, 9), F32)
        for i in range(3):
            a, b, c = M[:, 3 * i], M[:, 3 * i + 1], M[:, 3 * i + 2]
            MR[:, 3 * i + 0] = _dot3(a, Rn[:, 0], b, Rn[:, 1], c, Rn[:, 2])
            MR[:, 3 * i + 1] = _dot3(a, Rn[:, 1], b, Rn[:, 3], c, Rn[:, 4])
            MR[:, 3 * i + 2] = _dot3(a, Rn[:, 2], b, Rn[:, 4], c, Rn[:, 5])
        Rp9 = np.zeros((N, 9), F32)
        for i in range(3):
            for j in range(3):
                Rp9[:, 3 * i + j] = _dot3(MR[:, 3 * i], M[:, 3 * j], MR[:, 3 * i + 1], M[:, 3 * j + 1], MR[:, 3 * i + 2], M[:, 3 * j + 2])
        Rp = Rp9[:, [0, 1, 2, 4, 5, 8]]
        if W9 is None:
            W9 = np.zeros((N, 9), F32)
            for k in np.nonzero(used)[0]:
                if flags & FLAG_DOUBLE_W:
                    w = pinv3_sym_fast(Rp[k])
                    W9[k] = w[[0, 1, 2, 1, 3, 4, 2, 4, 5]]
                else:
                    W9[k] = _cod_pinv(Rp9[k])
        else:
            W9 = np.asarray(W9, F32).reshape(N, 9)
        Hj = np.zeros((N, 9), F32)
        for i in range(3):
            for c in range(3):
                o = 9 * c + 3 * i
                Hj[:, 3 * i + c] = _dot3(J[o], mu2[:, 0], J[o + 1], mu2[:, 1], J[o + 2], mu2[:, 2])
        Hz = np.zeros((N, 18), F32)
        for i in range(3):
            Hz[:, 6 * i + 0] = -M[:, 3 * i]; Hz[:, 6 * i + 1] = -M[:, 3 * i + 1]; Hz[:, 6 * i + 2] = -M[:, 3 * i + 2]
            for j in range(3):
                Hz[:, 6 * i + 3 + j] = _dot3(M[:, 3 * i], Hj[:, j], M[:, 3 * i + 1], Hj[:, 3 + j], M[:, 3 * i + 2], Hj[:, 6 + j])
        if _fault and _fault[0] == "transpose_hz":
            i = _fault[1]
            blk = Hz[i].reshape(3, 6)[:, 3:].copy()
            Hz[i].reshape(3, 6)[:, 3:] = blk.T
        WH = np.zeros((N, 18), F32)
        for j in range(6):
            for r in range(3):
                WH[:, 6 * r + j] = _dot3(W9[:, 3 * r], Hz[:, j], W9[:, 3 * r + 1], Hz[:, 6 + j], W9[:, 3 * r + 2], Hz[:, 12 + j])
        T = np.zeros((N, 27), F32)
        for q, (a, b) in enumerate(TRI):
            T[:, q] = _dot3(Hz[:, a], WH[:, b], Hz[:, 6 + a], WH[:, 6 + b], Hz[:, 12 + a], WH[:, 12 + b])
        for a in range(6):
            T[:, 21 + a] = _dot3(WH[:, a], dz[:, 0], WH[:, 6 + a], dz[:, 1], WH[:, 12 + a], dz[:, 2])
        qq = np.zeros(N, np.float64)
        dzD = dz.astype(np.float64); WD = W9.astype(np.float64)
        for i in range(3):
            for j in range(3):
                qq = qq + dzD[:, i] * WD[:, 3 * i + j] * dzD[:, j]
    T[~used] = 0; qq = np.where(used, qq, 0.0)
    return dict(terms=T, dz=dz, W9=W9, q=qq, used=used, db=db, mu2=mu2, Rp=Rp, Rp9=Rp9, M=M, Hz=Hz)


def terms_float64(db, mu2, M, W9, J):
    """The same formulas in float64 from float32 db, mu2, M, J and a fixed W9: (value (N, 27), P (N, 27)) with P the formulas on absolute values."""
    db = np.asarray(db, np.float64); mu2 = np.asarray(mu2, np.float64); M = np.asarray(M, np.float64).reshape(-1, 3, 3)
    W = np.asarray(W9, np.float64).reshape(-1, 3, 3); J = np.asarray(J, np.float64).reshape(3, 3, 3)       # J[c][i][k]
    N = db.shape[0]

    def ev(ab):
        f = np.abs if ab else (lambda x: x)
        Hj = np.einsum("cik,nk->nic", f(J), f(mu2))                         # (N, 3, 3): row i, column c
        Hz = np.concatenate([f(-M), np.einsum("nik,nkc->nic", f(M), Hj)], 2)   # (N, 3, 6)
        WH = np.einsum("nrk,nkj->nrj", f(W), Hz)
        dz = np.einsum("nik,nk->ni", f(M), f(db))
        out = np.zeros((N, 27))
        for q, (a, b) in enumerate(TRI):
            out[:, q] = (Hz[:, :, a] * WH[:, :, b]).sum(1)
        for a in range(6):
            out[:, 21 + a] = (WH[:, :, a] * dz).sum(1)
        return out
    return ev(False), ev(True)


# ---- the reduction ------------------------------------------------------------------------------------------------------------------------

def mirror(t27):
    """27 sums -> (H^T W H (6, 6) with the upper triangle mirrored, H^T W dz (6,))."""
    H = np.zeros((6, 6), F32)
    for q, (a, b) in enumerate(TRI):
        H[a, b] = t27[q]; H[b, a] = t27[q]
    return H, np.asarray(t27[21:27], F32)


def pack(htwh, htwdz):
    """(6, 6), (6,) -> the 27 packed sums."""
    H = np.asarray(htwh, F32).reshape(6, 6)
    return np.concatenate([np.asarray([H[a, b] for a, b in TRI], F32), np.asarray(htwdz, F32).reshape(6)])


def form_of(V):
    return "512" if V > 4096 else "256"


def depth(n_slots, form):
    """D: the largest number of float additions any one term passes through (derivation in the module docstring)."""
    if form == "256":
        return max(1, -(-n_slots // 256)) + 6 + 4
    return 1 + 6 + 8 + max(1, -(-n_slots // 512))


def exact_total(terms):
    """Per entry the exact sum of the float32 terms and the sum of their absolute values, as Fractions: (S[27], A[27])."""
    t = np.asarray(terms, np.float64).reshape(-1, 27)
    S = [Fraction(0)] * 27; A = [Fraction(0)] * 27
    for k in range(27):
        col = t[:, k][t[:, k] != 0]
        S[k] = sum((Fraction(x) for x in col.tolist()), Fraction(0)); A[k] = sum((abs(Fraction(x)) for x in col.tolist()), Fraction(0))
    return S, A


def bound(A, n_slots, form):
    """Per entry D 2^-24 sum |term|."""
    D = depth(n_slots, form)
    return [D * Fraction(1, 1 << 24) * a for a in A]


def compare_total(got27, terms, n_slots, form, exact=None):
    """(worst |got - exact| / bound over the entries with a non-zero bound, list of failing entries).  An entry whose terms are all zero must be zero.
    exact: exact_total(terms), when the caller has it already."""
    S, A = exact if exact is not None else exact_total(terms)
    B = bound(A, n_slots, form)
    worst, bad = 0.0, []
    for k in range(27):
        g = float(got27[k])
        if not np.isfinite(g):
            bad.append(k); worst = float("inf"); continue
        err = abs(Fraction(g) - S[k])
        if B[k] == 0:
            if err != 0:
                bad.append(k)
            continue
        worst = max(worst, float(err / B[k]))
        if err > B[k]:
            bad.append(k)
    return worst, bad


def _wave_total(v):
    """wave_total (icet_device_common.h) on (..., 64) float32: the inclusive DPP scan, lane 63."""
    v = np.asarray(v, F32).copy()
    lane = np.arange(64)
    for sh in (1, 2, 4, 8):
        src = np.zeros_like(v)
        ok = (lane % 16) >= sh
        src[..., ok] = v[..., lane[ok] - sh]
        v = v + src
    add = np.zeros_like(v); add[..., 16:32] = v[..., 15:16]; add[..., 48:64] = v[..., 47:48]
    v = v + add
    add = np.zeros_like(v); add[..., 32:64] = v[..., 31:32]
    v = v + add
    return v[..., 63]


def emulate_total(terms, form):
    """The device's reduction of (n_slots, 27) float32 terms in slot order (zero rows for slots that do not contribute), in float32: the 256-thread form or the
    canonical 512-slot form.  Returns 27 float32."""
    t = np.asarray(terms, F32).reshape(-1, 27)
    ns = t.shape[0]
    kT = 256 if form == "256" else 512
    rounds = max(1, -(-ns // kT))
    pad = np.zeros((rounds * kT, 27), F32); pad[:ns] = t
    pad = pad.reshape(rounds, kT, 27)
    if form == "256":
        S = np.zeros((kT, 27), F32)
        for r in range(rounds):
            S = S + pad[r]
        wt = _wave_total(S.reshape(4, 64, 27).transpose(0, 2, 1))            # (4 waves, 27)
        tot = np.zeros(27, F32)
        for w in range(4):
            tot = tot + wt[w]
        return tot
    tot = np.zeros(27, F32)
    for r in range(rounds):
        S = np.zeros((kT, 27), F32) + pad[r]
        wt = _wave_total(S.reshape(8, 64, 27).transpose(0, 2, 1))
        vb = np.zeros(27, F32)
        for w in range(8):
            vb = vb + wt[w]
        tot = tot + vb
    return tot
