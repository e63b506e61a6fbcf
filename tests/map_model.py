"""A NumPy restatement of the voxel map's rule (include/icet_hip.h icet_voxel_map_*; the device compiles icet_amd/csrc/icet_map.h).
float64 element-wise for what the rule does in double, keys by np.unique, sums and counts in Python integers, centroids with Python float(int)."""
import numpy as np

LIMIT = 1 << 20
TWO32 = float(1 << 32)
KEPT, NONFINITE, RANGE, OUTSIDE = 0, 1, 2, 3
OK, TABLE_FULL, NEGATIVE, TRUNCATED = 0, 1, 2, 4


def classify(scan, pose, cell, min_range=0.0, max_range=0.0):
    """Per row of ``scan`` (N x 3 float32) at ``pose`` (4 x 4 float32): class (KEPT / NONFINITE / RANGE / OUTSIDE), key (uint64), q (N x 3 uint64),
    cells (N x 3 int64).  key, q and cells only mean something where the class is KEPT."""
    p = np.asarray(scan, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(pose, np.float32).reshape(4, 4).astype(np.float64)
    cell32 = np.float32(cell)
    inv = 1.0 / float(cell32)
    mn, mx = float(np.float32(min_range)), float(np.float32(max_range))
    n = p.shape[0]
    cls = np.full(n, KEPT, np.int64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        d2 = (x * x + y * y) + z * z
        in_range = (d2 > mn * mn) & ((mx <= 0) | (d2 <= mx * mx))
        c = np.zeros((n, 3), np.float64); q = np.zeros((n, 3), np.uint64)
        inside = np.ones(n, bool)
        for a in range(3):
            w = ((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]
            s = w * inv
            ca = np.floor(s)
            ok = np.abs(ca) < LIMIT                                   # (a NaN compares false)
            u = s - ca
            f = np.floor(u * TWO32)
            f = np.where(ok & finite, np.minimum(f, TWO32 - 1.0), 0.0)
            q[:, a] = f.astype(np.uint64)
            c[:, a] = np.where(ok & finite, ca, 0.0)
            inside &= ok
    cls[~inside] = OUTSIDE
    cls[~in_range] = RANGE                                            # (the order of the rule: non-finite, range, outside)
    cls[~finite] = NONFINITE
    cells = c.astype(np.int64)
    cc = (cells + LIMIT).astype(np.uint64)
    key = (cc[:, 0] << np.uint64(42)) | (cc[:, 1] << np.uint64(21)) | cc[:, 2]
    return cls, key, q, cells


def key_cells(key):
    k = np.asarray(key, np.uint64)
    m = np.uint64(0x1FFFFF)
    return np.stack([((k >> np.uint64(42)) & m).astype(np.int64), ((k >> np.uint64(21)) & m).astype(np.int64), (k & m).astype(np.int64)], axis=-1) - LIMIT


def centroid(c, total, n, cell):
    """(float32)(((double)c + (double)total / ((double)n 2^32)) (double)cell), total and n Python integers."""
    return np.float32((float(int(c)) + float(int(total)) / (float(int(n)) * TWO32)) * float(np.float32(cell)))


class Map:
    """The map as a dict key -> [count, sum_x, sum_y, sum_z] of Python integers, and the running totals."""

    def __init__(self, cell=0.1, min_range=0.0, max_range=0.0):
        self.cell, self.min_range, self.max_range = cell, min_range, max_range
        self.clear()

    def clear(self):
        self.cells = {}
        self.totals = dict(points_in=0, points_kept=0, points_nonfinite=0, points_outside=0, points_dropped=0)

    def add(self, scans, poses, sign=1):
        poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
        assert len(scans) == poses.shape[0] and sign in (1, -1)
        for scan, T in zip(scans, poses):
            cls, key, q, _ = classify(scan, T, self.cell, self.min_range, self.max_range)
            t = self.totals
            t["points_in"] += int(cls.shape[0]); t["points_nonfinite"] += int((cls == NONFINITE).sum()); t["points_outside"] += int((cls == OUTSIDE).sum())
            keep = cls == KEPT
            t["points_kept"] += sign * int(keep.sum())
            if not keep.any():
                continue
            uk, inv, cnt = np.unique(key[keep], return_inverse=True, return_counts=True)
            qk = q[keep]
            hi = np.zeros((uk.shape[0], 3), np.uint64); lo = np.zeros((uk.shape[0], 3), np.uint64)
            np.add.at(hi, inv, qk >> np.uint64(16)); np.add.at(lo, inv, qk & np.uint64(0xFFFF))     # (uint64 sums of 32-bit values: exact)
            for i, k in enumerate(uk):
                e = self.cells.setdefault(int(k), [0, 0, 0, 0])
                e[0] += sign * int(cnt[i])
                for a in range(3):
                    e[1 + a] += sign * ((int(hi[i, a]) << 16) + int(lo[i, a]))
        return self

    def remove(self, scans, poses):
        return self.add(scans, poses, -1)

    def stats(self, min_points=1):
        mp = max(1, int(min_points))
        s = dict(self.totals)
        s["cells_occupied"] = sum(1 for e in self.cells.values() if e[0] > 0)
        s["cells_out"] = sum(1 for e in self.cells.values() if e[0] >= mp)
        s["cells_negative"] = sum(1 for e in self.cells.values() if e[0] < 0)
        s["status"] = (TABLE_FULL if s["points_dropped"] else 0) | (NEGATIVE if s["cells_negative"] else 0)
        return s

    def extract(self, min_points=1, cap_rows=None):
        mp = max(1, int(min_points))
        keys = sorted(k for k, e in self.cells.items() if e[0] >= mp)
        st = self.stats(min_points)
        if cap_rows is not None and len(keys) > cap_rows:
            keys = keys[:cap_rows]; st["status"] |= TRUNCATED
        xyz = np.zeros((len(keys), 3), np.float32); cnt = np.zeros(len(keys), np.int64)
        kc = key_cells(np.array(keys, np.uint64)).reshape(-1, 3)
        for i, k in enumerate(keys):
            e = self.cells[k]
            cnt[i] = e[0]
            for a in range(3):
                xyz[i, a] = centroid(kc[i, a], e[1 + a], e[0], self.cell)
        return dict(xyz=xyz, count=cnt, key=np.array(keys, np.uint64), stats=st)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(t=(0, 0, 0), r=(0, 0, 0)):
    T = np.eye(4)
    T[:3, :3] = rot(*r); T[:3, 3] = t
    return T.astype(np.float32)


def edge_rows(cell):
    """The edge table of the rule for one cell size, as (scan, pose, expected) triples: rows that the pose carries to the listed world coordinates.  The poses
    are pure translations or the identity, so w = x + t exactly where the text says so.  expected: a list of per-row dicts with the fields that are pinned
    (cls; cells / q where the text names them)."""
    I = pose()
    cases = []
    c32 = float(np.float32(cell))
    # w = k cell on x: u = 0 where k cell inv_cell is exactly k (cell 0.125; at 0.1 the model is the judge)
    rows = np.array([[k * c32, 1.0, 1.0] for k in (-3, 0, 5)], np.float32)
    exp = [dict(cls=KEPT, cx=k, qx=0) if cell == 0.125 else dict(cls=KEPT) for k in (-3, 0, 5)]
    cases.append((rows, I, exp))
    # -1e-29: cell -1, u rounds to 1.0, q clamps to 2^32 - 1
    cases.append((np.array([[-1e-29, 1.0, 1.0], [1.0, -1e-29, 1.0], [1.0, 1.0, -1e-29]], np.float32), I,
                  [dict(cls=KEPT, cx=-1, qx=(1 << 32) - 1), dict(cls=KEPT, cy=-1, qy=(1 << 32) - 1), dict(cls=KEPT, cz=-1, qz=(1 << 32) - 1)]))
    # +0.0 and -0.0: cell 0, q 0
    cases.append((np.array([[0.0, 1.0, 1.0], [-0.0, 1.0, 1.0]], np.float32), I, [dict(cls=KEPT, cx=0, qx=0), dict(cls=KEPT, cx=0, qx=0)]))
    # -0.3 and 0.3
    cases.append((np.array([[-0.3, 0.3, 1.0], [0.3, -0.3, 1.0]], np.float32), I, [dict(cls=KEPT), dict(cls=KEPT)]))
    # |c| = 2^20 - 1 (kept) and 2^20 (outside), each axis, both signs: a point 1 m from the sensor, the pose's translation carries it there
    for a in range(3):
        for c, cls in ((LIMIT - 1, KEPT), (LIMIT, OUTSIDE), (-(LIMIT - 1), KEPT), (-LIMIT, OUTSIDE)):
            t = [0.0, 0.0, 0.0]; t[a] = (c + 0.5) * c32               # the middle of cell c (float32 spacing there is 1 / 128 m)
            p = np.zeros((1, 3), np.float32); p[0, (a + 1) % 3] = 1.0  # 1 m from the sensor on another axis: w_a = t_a exactly
            e = dict(cls=cls)
            if cls == KEPT:
                e["c%s" % "xyz"[a]] = c
            cases.append((p, pose(t=t), [e]))
    # NaN, +inf, -inf in a row
    cases.append((np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf]], np.float32), I, [dict(cls=NONFINITE)] * 3))
    # NaN in the pose
    Tn = pose(); Tn[1, 3] = np.nan
    cases.append((np.array([[1, 2, 3]], np.float32), Tn, [dict(cls=OUTSIDE)]))
    Ti = pose(); Ti[0, 0] = np.inf
    cases.append((np.array([[1, 2, 3]], np.float32), Ti, [dict(cls=OUTSIDE)]))
    # an exact-zero row at min_range = 0
    cases.append((np.array([[0, 0, 0], [0, 0, 1e-20]], np.float32), I, [dict(cls=RANGE), dict(cls=KEPT)]))
    return cases


def range_rows():
    """Rows for min_range = 5, max_range = 13: d2 exactly min^2 (dropped), just above (kept), exactly max^2 (kept), just above (dropped)."""
    rows = np.array([[3, 4, 0], [3, 4, 0.01], [5, 12, 0], [5, 12, 0.01], [0, 0, 0]], np.float32)
    return rows, [RANGE, KEPT, KEPT, RANGE, RANGE]
