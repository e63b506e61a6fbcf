"""A NumPy restatement of the deskew rule (include/icet_hip.h icet_deskew_*; the device compiles icet_amd/csrc/icet_deskew.h).
float64 element-wise, one rounding per operation, in the order of the header, so the outputs agree with it bit for bit; the two pose <-> twist maps use
np.sin / np.cos / np.arctan2 and agree to the last bits of the math library."""
import math

import numpy as np

MOVED, ZERO, NONFINITE, BAD_TIME, OUT_OF_RANGE = 0, 1, 2, 3, 4
CLASS_NAMES = ("moved", "zero", "nonfinite", "bad_time", "out_of_range")
TIME_ARRAY, TIME_COLUMN_FAST, TIME_COLUMN_SLOW = 0, 1, 2

# the doubles nearest to (-1)^k / (2k + 1)!, / (2k + 2)!, / (2k + 3)! (every factorial up to 21! is a double: one rounding each)
FA = [(-1.0) ** k / float(math.factorial(2 * k + 1)) for k in range(10)]
FB = [(-1.0) ** k / float(math.factorial(2 * k + 2)) for k in range(10)]
FC = [(-1.0) ** k / float(math.factorial(2 * k + 3)) for k in range(10)]


def horner(c, u):
    u = np.asarray(u, np.float64)
    r = np.full_like(u, c[9])
    for k in range(8, -1, -1):
        r = r * u + c[k]
    return r


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def row_times(n, time=None, mode=TIME_ARRAY, period=0):
    """tau per row (float64) and the rows whose time is unusable."""
    if mode == TIME_ARRAY:
        tau = np.asarray(time, np.float32).reshape(-1).astype(np.float64)
        assert tau.shape[0] == n
        return tau, ~np.isfinite(tau)
    i = np.arange(n, dtype=np.int64)
    c = i % period if mode == TIME_COLUMN_FAST else i // period
    return c.astype(np.float64) + 0.5, np.zeros(n, bool)


def deskew(rows, twist, time=None, mode=TIME_ARRAY, period=0, t0=0.0, inv_span=1.0, ref=1.0):
    """rows N x 3 float32 -> (N x 3 float32, classes).  A row that is not moved keeps its bits."""
    rows = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 3))
    n = rows.shape[0]
    xi = np.asarray(twist, np.float64).reshape(6)
    out = rows.copy()
    cls = np.full(n, MOVED, np.int64)
    if n == 0:
        return out, cls
    tau, bad = row_times(n, time, mode, period)
    with np.errstate(all="ignore"):
        p = rows.astype(np.float64)
        d = (tau - float(t0)) * float(inv_span) - float(ref)
        th = d[:, None] * xi[None, 3:]
        u = (th[:, 0] * th[:, 0] + th[:, 1] * th[:, 1]) + th[:, 2] * th[:, 2]
        A, B, Cc = horner(FA, u), horner(FB, u), horner(FC, u)
        sg = d[:, None] * xi[None, :3]
        c1 = cross(th, p); c2 = cross(th, c1); r1 = cross(th, sg); r2 = cross(th, r1)
        o = ((p + A[:, None] * c1) + B[:, None] * c2) + ((sg + B[:, None] * r1) + Cc[:, None] * r2)
        o32 = o.astype(np.float32)
        cls[~(u <= 1.0)] = OUT_OF_RANGE                               # (the order of the rule: non-finite, zero, time, range)
        cls[bad] = BAD_TIME
        cls[(rows == 0).all(1)] = ZERO
        cls[~np.isfinite(rows).all(1)] = NONFINITE
    moved = cls == MOVED
    out[moved] = o32[moved]
    return out, cls


def counts(cls):
    return {name: int((np.asarray(cls) == k).sum()) for k, name in enumerate(CLASS_NAMES)}


# ---- pose <-> twist: float64, the order of the header ------------------------------------------------------------------------------------------------------------

def _abc(u):
    if u <= 1.0:
        return float(horner(FA, u)), float(horner(FB, u)), float(horner(FC, u))
    t = math.sqrt(u)
    return math.sin(t) / t, (1.0 - math.cos(t)) / u, (t - math.sin(t)) / (u * t)


def _hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def pose_from_twist(xi, s=1.0):
    xi = np.asarray(xi, np.float64).reshape(6)
    sg, th = s * xi[:3], s * xi[3:]
    u = float((th[0] * th[0] + th[1] * th[1]) + th[2] * th[2])
    A, B, C = _abc(u)
    K = _hat(th)
    T = np.eye(4)
    T[:3, :3] = (np.eye(3) + A * K) + B * (K @ K)
    T[:3, 3] = (sg + B * (K @ sg)) + C * (K @ (K @ sg))
    return T


def twist_from_pose(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    w = 0.5 * np.array([T[2, 1] - T[1, 2], T[0, 2] - T[2, 0], T[1, 0] - T[0, 1]])
    sn = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    cs = 0.5 * (((T[0, 0] + T[1, 1]) + T[2, 2]) - 1.0)
    t = math.atan2(sn, cs)
    f = t / sn if sn > 1e-5 else 1.0 + t * t * (1.0 / 6.0 + t * t * (7.0 / 360.0))
    th = f * w
    u = float((th[0] * th[0] + th[1] * th[1]) + th[2] * th[2])
    _, B, C = _abc(u)
    K = _hat(th)
    V = (np.eye(3) + B * K) + C * (K @ K)
    return np.concatenate([np.linalg.solve(V, T[:3, 3]), th])


def twist_between(T0, T1, scale=1.0):
    """scale log(T0^-1 T1) from two float32 poses, the inverse of a pose taken as the transpose of its rotation."""
    T0 = np.asarray(T0, np.float32).reshape(4, 4).astype(np.float64); T1 = np.asarray(T1, np.float32).reshape(4, 4).astype(np.float64)
    D = np.eye(4)
    D[:3, :3] = T0[:3, :3].T @ T1[:3, :3]
    D[:3, 3] = T0[:3, :3].T @ (T1[:3, 3] - T0[:3, 3])
    return scale * twist_from_pose(D)


def exp_closed(xi, s):
    """exp(s xi) per entry of s from np.sin / np.cos (Rodrigues, no series): R (N x 3 x 3), t (N x 3).  The reference the polynomials are judged by."""
    xi = np.asarray(xi, np.float64).reshape(6); s = np.asarray(s, np.float64).reshape(-1)
    R = np.zeros((s.shape[0], 3, 3)); t = np.zeros((s.shape[0], 3))
    for k, sk in enumerate(s):
        th = sk * xi[3:]; sg = sk * xi[:3]
        a = float(np.linalg.norm(th)); K = _hat(th)
        if a < 1e-7:
            A, B, C = 1.0 - a * a / 6.0, 0.5 - a * a / 24.0, 1.0 / 6.0 - a * a / 120.0
        else:
            A, B, C = np.sin(a) / a, (1.0 - np.cos(a)) / (a * a), (a - np.sin(a)) / (a ** 3)
        R[k] = np.eye(3) + A * K + B * (K @ K)
        t[k] = (np.eye(3) + B * K + C * (K @ K)) @ sg
    return R, t


# ---- the tables the CPU and the GPU tests share -------------------------------------------------------------------------------------------------------------------

TWIST = np.array([1.0, 0.05, 0.0, 0.002, -0.001, 0.08])              # per sweep: 10 m/s and 0.8 rad/s at 10 Hz


def class_table():
    """(rows, time, twist, kwargs, expected classes): the edge table of the rule, one call each."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    cases = []
    # zeros with both signs, NaN and inf coordinates, a NaN time, ordinary rows, denormals, 1e18 magnitudes, s < 0 and s > 1
    rows = np.array([[0, 0, 0], [-0.0, 0.0, -0.0], [-0.0, -0.0, -0.0], [nan, 1, 1], [1, inf, 1], [1, 1, -inf], [nan, 0, 0], [1, 2, 3], [4, 5, 6],
                     [1e-45, 0, 0], [1e-40, -1e-42, 1e-39], [1e18, -1e18, 1e18], [3e38, 3e38, 3e38], [10, 20, 1], [10, 20, 1], [0, 0, 1e-45]], np.float32)
    time = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, nan, nan, inf, 0.25, 0.75, 0.5, 0.3, -0.7, 1.9, 0.1], np.float32)
    exp = [ZERO, ZERO, ZERO, NONFINITE, NONFINITE, NONFINITE, NONFINITE, BAD_TIME, BAD_TIME, MOVED, MOVED, MOVED, MOVED, MOVED, MOVED, MOVED]
    cases.append((rows, time, TWIST, dict(ref=1.0), exp))
    # u just below, at and just above 1: |phi| = 1 along z, d = s - 0
    one = np.array([[1, 2, 3]] * 5, np.float32)
    t1 = np.array([np.nextafter(np.float32(1), np.float32(0)), 1.0, np.nextafter(np.float32(1), np.float32(2)), -1.0, -1.0000001], np.float32)
    cases.append((one, t1, np.array([0.1, 0.2, 0.3, 0.0, 0.0, 1.0]), dict(ref=0.0), [MOVED, MOVED, OUT_OF_RANGE, MOVED, OUT_OF_RANGE]))
    # a NaN twist, a NaN parameter: every finite non-zero row with a time is out of range
    two = np.array([[1, 2, 3], [0, 0, 0], [nan, 1, 1], [4, 5, 6]], np.float32); t2 = np.array([0.5, 0.5, 0.5, nan], np.float32)
    tw_nan = TWIST.copy(); tw_nan[4] = np.nan
    cases.append((two, t2, tw_nan, dict(ref=1.0), [OUT_OF_RANGE, ZERO, NONFINITE, BAD_TIME]))
    cases.append((two, t2, TWIST, dict(ref=np.nan), [OUT_OF_RANGE, ZERO, NONFINITE, BAD_TIME]))
    cases.append((two, t2, TWIST, dict(ref=1.0, inv_span=np.inf), [OUT_OF_RANGE, ZERO, NONFINITE, BAD_TIME]))
    # a NaN in rho alone: the rotation is in range, the row is moved to NaN (the rule does not look at rho)
    tw_rho = TWIST.copy(); tw_rho[0] = np.nan
    cases.append((two[:1], t2[:1], tw_rho, dict(ref=1.0), [MOVED]))
    return cases


def sharpness_inputs(n_frames=8, rings=16, steps=256, sigma=0.02):
    """Sweeps of rings x steps from make_scene(2000) at TWIST with their true start poses: (raw rows, row times, model-deskewed rows to ref 0, float32 poses)."""
    from icet_amd import lidar_sim as ls
    sweeps, poses = ls.make_sweep_sequence(n_frames, TWIST, 2000, 2001, rings, steps, sigma)
    raw = [sc.numpy().T.copy() for sc, _ in sweeps]
    times = [s.numpy() for _, s in sweeps]
    fixed = [deskew(r, TWIST, t, ref=0.0)[0] for r, t in zip(raw, times)]
    return raw, times, fixed, poses.astype(np.float32)


def sharpness_counts(cell=0.5):
    """Occupied cells of the map model fused from the raw sweeps and from the deskewed ones, at the same poses."""
    import map_model as mm
    raw, _, fixed, poses = sharpness_inputs()
    return mm.Map(cell).add(raw, poses).stats()["cells_occupied"], mm.Map(cell).add(fixed, poses).stats()["cells_occupied"]
