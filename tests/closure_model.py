"""NumPy model of the loop-closure query's rule (include/icet_hip.h "loop closure against the store"; icet_amd/csrc/icet_closure.h), written
from the rule's text alone: the float32 candidate distance and order, and the double-precision start pose.  tests/test_loop_closure.py holds the
header (on the host) and the kernels (on the GPU) to it."""
import numpy as np


def euler_R(phi, theta, psi):
    """The rotation of (phi, theta, psi) as the solver writes it, float64 3 x 3 (row-major as printed)."""
    c, s = np.cos, np.sin
    return np.array([[c(theta) * c(psi), s(psi) * c(phi) + s(phi) * s(theta) * c(psi), s(phi) * s(psi) - s(theta) * c(phi) * c(psi)],
                     [-s(psi) * c(theta), c(phi) * c(psi) - s(phi) * s(theta) * s(psi), s(phi) * c(psi) + s(theta) * s(psi) * c(phi)],
                     [s(theta), -s(phi) * c(theta), c(phi) * c(theta)]], np.float64)


def euler_of(R):
    """(phi, theta, psi) of a rotation written as euler_R writes it."""
    return np.array([np.arctan2(-R[2, 1], R[2, 2]), np.arcsin(np.clip(R[2, 0], -1.0, 1.0)), np.arctan2(-R[1, 0], R[0, 0])], np.float64)


def pose(t, R):
    """4 x 4 float32 pose [R | t; 0 0 0 1]."""
    T = np.eye(4, dtype=np.float64); T[:3, :3] = R; T[:3, 3] = t
    return T.astype(np.float32)


def pose_yaw(t, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return pose(t, np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]))


def start_pose64(Tq, Tj):
    """The six values of the start pose in double, from float32 poses, sums left to right: R_X = R_q^T R_j, X_t = R_q^T (t_q - t_j)."""
    Tq = np.asarray(Tq, np.float32).reshape(4, 4).astype(np.float64); Tj = np.asarray(Tj, np.float32).reshape(4, 4).astype(np.float64)
    Rq, Rj = Tq[:3, :3], Tj[:3, :3]
    d = Tq[:3, 3] - Tj[:3, 3]
    RX = np.empty((3, 3), np.float64); t = np.empty(3, np.float64)
    for a in range(3):
        for b in range(3):
            RX[a, b] = (Rq[0, a] * Rj[0, b] + Rq[1, a] * Rj[1, b]) + Rq[2, a] * Rj[2, b]
        t[a] = (Rq[0, a] * d[0] + Rq[1, a] * d[1]) + Rq[2, a] * d[2]
    return np.concatenate([t, euler_of(RX)])


def start_pose(Tq, Tj):
    return start_pose64(Tq, Tj).astype(np.float32)


def pose_step64(X):
    """[R(X)^T | R(X)^T X_t] in double from the float32 X."""
    X = np.asarray(X, np.float32).astype(np.float64)
    R = euler_R(X[3], X[4], X[5])
    T = np.eye(4, dtype=np.float64); T[:3, :3] = R.T; T[:3, 3] = R.T @ X[:3]
    return T


def dist2(tq, ts):
    """float32, one rounding per operation: fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)); ts: (n, 3)."""
    tq = np.asarray(tq, np.float32); ts = np.asarray(ts, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = tq[0] - ts[:, 0]; dy = tq[1] - ts[:, 1]; dz = tq[2] - ts[:, 2]
        return ((dx * dx) + (dy * dy)) + (dz * dz)


def candidates(tq, sq, t_slots, stamps, has_pose, radius, k, min_stamp_gap=0):
    """The first k eligible slots in ascending (d2, slot) order, -1 behind the last; also their d2.  t_slots (n, 3) float32, stamps (n) int64, has_pose (n) bool
    (occupied and posed)."""
    d2 = dist2(tq, t_slots)
    r2 = np.float32(radius) * np.float32(radius)
    with np.errstate(invalid="ignore"):
        ok = np.asarray(has_pose, bool) & (d2 <= r2)
    if min_stamp_gap > 0:
        gap = np.array([abs(int(sq) - int(s)) for s in np.asarray(stamps).tolist()], dtype=object)
        ok &= np.array([g >= int(min_stamp_gap) for g in gap], bool)
    idx = np.nonzero(ok)[0]
    order = idx[np.lexsort((idx, d2[idx]))][:k]
    out = np.full(k, -1, np.int32); out[:order.size] = order
    dd = np.zeros(k, np.float32); dd[:order.size] = d2[order]
    return out, dd
