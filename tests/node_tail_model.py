"""What a node hands to its caller AFTER the solve (icet_amd/csrc/icet_nodes.hip: ring_add_scan_row, align_row, frame_tail; icet_node_tail.h), as a function of the
node's OWN X per frame, its stored scan and the down-sample draw -- so nothing here carries a solve tolerance.  NumPy only; calls nothing in the library and reads no
file.  Two models (tests/test_node_tail.py holds the oracle's node, the hook icet_debug_node_tail and the device to them):

FLOAT32 RESTATEMENT (F32Tail, inverse3_lu, pose_chain, quat_of, ring_row, cloud_row).  The source's operation order, every operation a float32 NumPy operation of
its own (NumPy does not fuse): the LU inverse with its pivot choice (first largest |entry| of the column, strict >), the `== 0` skip and the two triangular solves
against the permuted identity; the pose product `acc = 0; acc += pose[r][k] * Hi[k][c]` for k = 0 .. 3; Shoemake's four branches; the ring row `a -= tx`, then
`(a*i00 + b*i10) + c*i20`; the cloud and snail row `((a*i00 + b*i10) + c*i20) - tx`; the ring's write window [pos, pos + m) modulo cap, `filled` once
pos + m >= cap and getQueue's order (pos + i) % cap.  R is NOT restated: std::cos / std::sin in float are the C library's, so the restatement takes R as an input
(the hook's) and R is held to a bound only.

EXACT MODEL (ExactTail), np.longdouble on the float32 inputs: the Euler R in the layout of euler_R_host, R^-1 = R^T, a ring row as the composition of
v -> (v - t_j) R_j^-1 over the frames since its insertion (that frame included), the cloud v R^-1 - t, the snail trail, the pose product, and a quaternion as the
dominant eigenvector of the 4 x 4 K matrix of the pose (no branches; compared up to sign).

BOUNDS, u = 2^-24, from the source's operation counts -- conditions, not measurements:
  R entry, C_R = 16.  The C library's float cos / sin are within 1 ulp: |d| <= 2u absolute.  A product of two of them: 2 * 2u + u = 5u (R[0], R[3], R[7], R[8];
      R[6] = sin: 2u).  `x*y + p*q*r`: 5u + (3 * 2u + 2u) + u for the sum = 14u.  With the second-order terms: 16u for every entry, and the Frobenius norm of
      R_hat - R is within sqrt(3^2 + 4 * 6^2 + 4 * 16^2) u < 35u.
  R^-1 entry against R^T, C_RI = 104.  (a) inv(R_hat) - R^T = -R^T E R^T + O(E^2), entry (i, j) <= 16u * |column i of R|_1 * |row j of R|_1 <= 48u (Frobenius: that
      of E, 35u).  (b) the LU inverse of A = R_hat: every column solves (A + dA) x = e with |dA| <= gamma_9 |L||U| (Higham, Accuracy and Stability, theorem 9.4,
      n = 3), so |X_hat - A^-1| <= 9u |A^-1||L||U||X_hat| entrywise.  A is orthonormal to first order, so row k of U = (row k of L^-1) * (orthonormal) has 2-norm
      <= 1, sqrt 2, sqrt 6 (|l| <= 1 under partial pivoting), a column of X_hat has 2-norm 1, sum over p >= k of |A^-1|[i][p] <= sqrt(4 - k):
      sqrt 3 * 1 + sqrt 2 * sqrt 2 + 1 * sqrt 6 < 6.2, times 9u: 56u.  C_RI = 48 + 56.  The Frobenius norm of R^-1_hat - R^T is within 35u + 3 * 56u = 203u.
  A row, per application, in the 2-NORM of the row (a rigid motion keeps the 2-norm of an older error, not its largest entry):
      |row_hat - row|_2 <= C_ROW u (|v|_2 + |t|_2),  C_ROW = 216 -- above 64, and the term that carries it is (b): the worst-case backward error of a pivoted LU (gamma_9
      times the growth of |L||U|), three times over to turn an entrywise bound into a norm; then (a), R's own entries.  The arithmetic of the row -- one difference, three
      products, two sums, each within u of a value <= |v| + |t| -- adds sqrt 3 * 5u < 9u; 203 + 9 < 216.  For the ring v - t is formed first (|v - t| <= |v| + |t|), for
      the cloud and the trail the difference comes last; the same constant covers both.  A ring or trail row that has been through several frames accumulates
      sum_j C_ROW u (|v_j| + |t_j|), v_j the exact row in front of application j.  The measured errors are a few u (prototype: 0.3 of a bound with C_ROW = 16), so the bound
      is loose by the factor the worst cases demand; the BIT comparison with the restatement is the sharp check, the bound the one that needs no restatement.
  Pose entry.  P_hat = fl(P_hat' H_hat), H_hat = [R_hat t; 0 1]: four products and four sums, so entrywise
      |P_hat - P| <= B' |H| + (|P'| + B') (E_H + 4u |H|) (1 + 2^-20),  B' the bound of the pose before the frame (0 for an exact pose_in), E_H = 16u on the 3 x 3 block.
  Quaternion, against the exact quaternion of an exact rotation from which the float32 3 x 3 block differs entrywise by at most eps.  The branch taken has
      s = 4 q_i^2 >= 1 for its largest component: s carries 3 eps + 12u, t = sqrt s half of that relatively plus u, q_i = t / 2; another component is
      (m_ab +- m_ba) (0.5 / t): eps + u from the numerator (<= 2 in size, halved) and |q| (1.5 eps + 6u + 3u) from the factor:
      |q_hat -+ q| <= 3 eps + 12u = E_Q(eps) per component, and the norm of q_hat is held to the same figure.

NAMED FAULTS (`_fault=` of ExactTail): transposed_inverse (R in place of R^-1), euler_reversed (the angles taken as psi, theta, phi), subtract_then_rotate (cloud and
trail as (v - t) R^-1), rotate_then_subtract (ring as v R^-1 - t), pose_reversed (H * pose), window_off_by_one (the write window starts at pos + 1), no_wrap (the
window is cut off at cap).  tests/test_node_tail.py shows that each one leaves its bound by more than a factor of ten on the suite's drive.
"""
import numpy as np

F32 = np.float32
LD = np.longdouble
U = 2.0 ** -24
C_R, C_RI, C_ROW = 16, 104, 216
FAULTS = ("transposed_inverse", "euler_reversed", "subtract_then_rotate", "rotate_then_subtract", "pose_reversed", "window_off_by_one", "no_wrap")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the float32 restatement ------------------------------------------------------------------------------------------------------------------

def inverse3_lu(A):
    """icet_node_tail::inverse3_lu: (3, 3) float32 -> (3, 3) float32, operation for operation."""
    lu = np.array(A, F32).reshape(3, 3).copy()
    perm = [0, 1, 2]
    inv = np.zeros((3, 3), F32)
    with np.errstate(all="ignore"):
        for k in range(3):
            piv, best = k, np.abs(lu[k, k])
            for r in range(k + 1, 3):
                if np.abs(lu[r, k]) > best:
                    best, piv = np.abs(lu[r, k]), r
            if piv != k:
                lu[[k, piv]] = lu[[piv, k]]
                perm[k], perm[piv] = perm[piv], perm[k]
            if lu[k, k] == 0:
                continue
            for r in range(k + 1, 3):
                lu[r, k] = lu[r, k] / lu[k, k]
                for c in range(k + 1, 3):
                    lu[r, c] = lu[r, c] - lu[r, k] * lu[k, c]
        for col in range(3):
            b = [F32(1.0) if perm[r] == col else F32(0.0) for r in range(3)]
            for r in range(1, 3):
                for c in range(r):
                    b[r] = b[r] - lu[r, c] * b[c]
            for r in (2, 1, 0):
                for c in range(r + 1, 3):
                    b[r] = b[r] - lu[r, c] * b[c]
                b[r] = b[r] / lu[r, r]
            for r in range(3):
                inv[r, col] = b[r]
    return inv


def pose_chain(pose, R, t):
    """icet_node_tail::pose_chain: pose * [R t; 0 1], (4, 4) float32."""
    pose = np.array(pose, F32).reshape(4, 4)
    Hi = np.zeros((4, 4), F32); Hi[:3, :3] = np.array(R, F32).reshape(3, 3); Hi[:3, 3] = np.array(t, F32).reshape(3); Hi[3, 3] = 1
    P = np.zeros((4, 4), F32)
    with np.errstate(all="ignore"):
        for r in range(4):
            for c in range(4):
                acc = F32(0.0)
                for k in range(4):
                    acc = acc + pose[r, k] * Hi[k, c]
                P[r, c] = acc
    return P


def quat_branch(P):
    """The branch quat_of takes on this float32 pose: 3 for `t > 0`, otherwise i = 0, 1, 2."""
    m = np.array(P, F32).reshape(4, 4)
    with np.errstate(all="ignore"):
        t = (m[0, 0] + m[1, 1]) + m[2, 2]
    if t > 0:
        return 3
    i = 0
    if m[1, 1] > m[0, 0]: i = 1
    if m[2, 2] > m[i, i]: i = 2
    return i


def quat_of(P):
    """icet_node_tail::quat_of: x, y, z, w of the pose's 3 x 3 block, float32."""
    m = np.array(P, F32).reshape(4, 4)
    q = np.zeros(4, F32)
    half, one = F32(0.5), F32(1.0)
    with np.errstate(all="ignore"):
        i = quat_branch(m)
        if i == 3:
            t = np.sqrt(((m[0, 0] + m[1, 1]) + m[2, 2]) + one)
            q[3] = half * t; t = half / t
            q[0] = (m[2, 1] - m[1, 2]) * t; q[1] = (m[0, 2] - m[2, 0]) * t; q[2] = (m[1, 0] - m[0, 1]) * t
        else:
            j = (i + 1) % 3; k = (j + 1) % 3
            t = np.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + one)
            q[i] = half * t; t = half / t
            q[3] = (m[k, j] - m[j, k]) * t; q[j] = (m[j, i] + m[i, j]) * t; q[k] = (m[k, i] + m[i, k]) * t
    return q


def ring_row(v, t, Ri):
    """ring_add_scan_row on rows v (n, 3): a -= tx, then (a*i00 + b*i10) + c*i20."""
    v = np.asarray(v, F32); t = np.asarray(t, F32); Ri = np.asarray(Ri, F32).reshape(3, 3)
    with np.errstate(all="ignore"):
        a, b, c = v[:, 0] - t[0], v[:, 1] - t[1], v[:, 2] - t[2]
        return np.stack([(a * Ri[0, k] + b * Ri[1, k]) + c * Ri[2, k] for k in range(3)], axis=1)


def cloud_row(v, t, Ri):
    """align_row and the snail trail's row: ((a*i00 + b*i10) + c*i20) - tx."""
    v = np.asarray(v, F32).reshape(-1, 3); t = np.asarray(t, F32); Ri = np.asarray(Ri, F32).reshape(3, 3)
    with np.errstate(all="ignore"):
        a, b, c = v[:, 0], v[:, 1], v[:, 2]
        return np.stack([((a * Ri[0, k] + b * Ri[1, k]) + c * Ri[2, k]) - t[k] for k in range(3)], axis=1)


class _Ring:
    """EigenQueue's bookkeeping (simpleMapMaker.cpp:18-59) over rows of any dtype; `aux` rides along (the exact model's accumulated bounds)."""

    def __init__(self, cap, dtype, fault=None):
        self.cap, self.fault = int(cap), fault
        self.q = np.zeros((self.cap, 3), dtype); self.aux = np.zeros(self.cap, dtype)
        self.pos, self.filled = 0, False
        self.last_window = np.zeros(0, np.int64)

    def write(self, rows):
        m = len(rows)
        start = self.pos + (1 if self.fault == "window_off_by_one" else 0)
        idx = start + np.arange(m)
        keep = idx < self.cap if self.fault == "no_wrap" else np.ones(m, bool)
        idx = idx % self.cap
        self.q[idx[keep]] = rows[keep]; self.aux[idx[keep]] = 0
        self.last_window = idx[keep]
        if self.pos + m >= self.cap: self.filled = True
        self.pos = (self.pos + m) % self.cap

    def order(self):
        return (self.pos + np.arange(self.cap)) % self.cap if self.filled else np.arange(self.pos)


class F32Tail:
    """The tail in float32, frame by frame.  frame(X, R, raw, scan): X the node's solution, R the frame's rotation (the hook's: not restated), raw the rows drawn for
    the ring (m, 3), scan the stored scan (n, 3) -> the aligned cloud (or None).  map(), snail, pose, quat are what the accessors and the result return."""

    def __init__(self, cap=0, aligned=False, snail=False):
        self.ring = _Ring(cap, F32) if cap > 0 else None
        self.want_aligned = aligned
        self.snail = np.zeros((1, 3), F32) if snail else None
        self.pose = np.eye(4, dtype=F32); self.quat = quat_of(self.pose)
        self.Ri = None

    def frame(self, X, R, raw=None, scan=None):
        X = np.asarray(X, F32); t = X[:3]
        Ri = self.Ri = inverse3_lu(R)
        if self.ring is not None:
            self.ring.write(np.asarray(raw, F32).reshape(-1, 3))
            self.ring.q = ring_row(self.ring.q, t, Ri)
        out = cloud_row(scan, t, Ri) if self.want_aligned else None
        if self.snail is not None:
            self.snail = np.concatenate([cloud_row(self.snail, t, Ri), np.zeros((1, 3), F32)])
        self.pose = pose_chain(self.pose, R, t); self.quat = quat_of(self.pose)
        return out

    def map(self):
        return self.ring.q[self.ring.order()]


# ---- the exact model --------------------------------------------------------------------------------------------------------------------------

def exact_R(angles, _fault=None):
    """euler_R_host's layout in longdouble on the float32 angles (phi, theta, psi)."""
    a = np.asarray(angles, F32).astype(LD)
    if _fault == "euler_reversed": a = a[::-1]
    (cph, cth, cps), (sph, sth, sps) = np.cos(a), np.sin(a)
    return np.array([[cth * cps, sps * cph + sph * sth * cps, sph * sps - sth * cph * cps],
                     [-sps * cth, cph * cps - sph * sth * sps, sph * cps + sth * sps * cph],
                     [sth, -sph * cth, cph * cth]], LD)


def norm2(v):
    v = np.asarray(v, LD)
    return np.sqrt((v * v).sum(axis=-1))


def row_bound(v, t):
    """One application of a frame to exact rows v (n, 3): C_ROW u (|v|_2 + |t|_2), the bound on the 2-norm of the row's error."""
    return C_ROW * U * (norm2(v) + norm2(t))


def pose_bound(P_prev, B_prev, H):
    """Entrywise bound of the chained pose behind one frame (module docstring): P_prev exact (4, 4), B_prev its bound, H = [R t; 0 1] exact."""
    E = np.zeros((4, 4), LD); E[:3, :3] = C_R * U
    aH = np.abs(H)
    return B_prev @ aH + (np.abs(P_prev) + B_prev) @ (E + 4 * U * aH) * (1 + 2.0 ** -20)


def quat_bound(eps):
    return 3 * eps + 12 * U


def exact_quat(P):
    """x, y, z, w of the rotation nearest the 3 x 3 block: the dominant eigenvector of K (Bar-Itzhack); float64 eigh of longdouble entries (2^-53 against bounds of 2^-21)."""
    m = np.asarray(P, LD)[:3, :3].astype(np.float64)
    K = np.array([[m[0, 0] - m[1, 1] - m[2, 2], m[1, 0] + m[0, 1], m[2, 0] + m[0, 2], m[2, 1] - m[1, 2]],
                  [m[1, 0] + m[0, 1], m[1, 1] - m[0, 0] - m[2, 2], m[2, 1] + m[1, 2], m[0, 2] - m[2, 0]],
                  [m[2, 0] + m[0, 2], m[2, 1] + m[1, 2], m[2, 2] - m[0, 0] - m[1, 1], m[1, 0] - m[0, 1]],
                  [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], m[0, 0] + m[1, 1] + m[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K)
    return v[:, -1]


def quat_error(q, q_exact):
    """max |q -+ q_exact| over the components, the better of the two signs."""
    q = np.asarray(q, np.float64); e = np.asarray(q_exact, np.float64)
    return float(min(np.abs(q - e).max(), np.abs(q + e).max()))


class ExactTail:
    """The tail in longdouble with its derived bounds, frame by frame; the arguments of F32Tail.frame without R.  After a frame: map() / map_bound() (rows in
    getQueue's order, bound on each row's 2-norm error), aligned / aligned_bound, snail / snail_bound, pose / pose_B (entrywise), quat / quat_E."""

    def __init__(self, cap=0, aligned=False, snail=False, _fault=None):
        assert _fault is None or _fault in FAULTS
        self.fault = _fault
        self.ring = _Ring(cap, LD, _fault) if cap > 0 else None
        self.want_aligned = aligned
        self.snail = np.zeros((1, 3), LD) if snail else None
        self.snail_bound = np.zeros(1, LD)
        self.pose = np.eye(4, dtype=LD); self.pose_B = np.zeros((4, 4), LD)
        self.aligned = self.aligned_bound = None
        self.quat, self.quat_E = exact_quat(self.pose), quat_bound(0.0)

    def _cloud(self, v, t, Ri):
        return (v - t) @ Ri if self.fault == "subtract_then_rotate" else v @ Ri - t

    def frame(self, X, raw=None, scan=None):
        X = np.asarray(X, F32).astype(LD); t = X[:3]
        R = exact_R(np.asarray(X[3:], F32), self.fault)
        Ri = R if self.fault == "transposed_inverse" else R.T
        if self.ring is not None:
            g = self.ring
            g.write(np.asarray(raw, F32).reshape(-1, 3).astype(LD))
            g.aux = g.aux + row_bound(g.q, t)
            g.q = g.q @ Ri - t if self.fault == "rotate_then_subtract" else (g.q - t) @ Ri
        if self.want_aligned:
            v = np.asarray(scan, F32).astype(LD)
            self.aligned, self.aligned_bound = self._cloud(v, t, Ri), row_bound(v, t)
        if self.snail is not None:
            self.snail_bound = np.concatenate([self.snail_bound + row_bound(self.snail, t), np.zeros(1, LD)])
            self.snail = np.concatenate([self._cloud(self.snail, t, Ri), np.zeros((1, 3), LD)])
        H = np.eye(4, dtype=LD); H[:3, :3] = R; H[:3, 3] = t
        self.pose_B = pose_bound(self.pose, self.pose_B, H)
        self.pose = H @ self.pose if self.fault == "pose_reversed" else self.pose @ H
        self.quat, self.quat_E = exact_quat(self.pose), quat_bound(float(self.pose_B[:3, :3].max()))

    def map(self):
        return self.ring.q[self.ring.order()]

    def map_bound(self):
        return self.ring.aux[self.ring.order()]


def row_ratio(got, exact, bound):
    """Worst |got - exact|_2 / bound over the rows with finite `exact` (0 for no rows); rows whose exact value is not finite must not be finite in `got` either."""
    got = np.asarray(got, F32).astype(LD).reshape(-1, 3); exact = np.asarray(exact, LD).reshape(-1, 3); bound = np.asarray(bound, LD).reshape(-1)
    assert got.shape == exact.shape and len(bound) == len(got)
    fin = np.isfinite(exact).all(axis=1)
    assert not np.isfinite(got[~fin]).all(axis=1).any()
    if not fin.any(): return 0.0
    err = norm2(got[fin] - exact[fin]); b = bound[fin]
    if (err[b == 0] > 0).any(): return float("inf")               # (a bound of 0 -- a fresh trail origin, a row under X = 0 at the origin -- asks for the exact value)
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
