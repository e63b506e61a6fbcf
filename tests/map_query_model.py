"""A NumPy restatement of the rule of a voxel map's query (include/icet_hip.h icet_voxel_map_query_*; the device compiles
icet_amd/csrc/icet_map_query.h), on top of the extract of tests/map_model.py: float64 element-wise for what the rule does in double, with the float32 casts
where the rule has them."""
import numpy as np

TRUNCATED, BAD_POSE = 4, 8


def pose_ok(pose):
    return bool(np.isfinite(np.asarray(pose, np.float32).reshape(-1)[:12]).all())


def query_extract(ext, pose, min_range=0.0, max_range=0.0, min_points=1, world=False, cap_rows=None):
    """The sub-map of an extract at min_points 1 (dict xyz, count, key: tests/map_model.py Map.extract()) around ``pose`` (4 x 4 float32):
    dict(xyz (n, 3) float32, count, key, total, status)."""
    T = np.asarray(pose, np.float32).reshape(4, 4)
    if not pose_ok(T):
        return dict(xyz=np.zeros((0, 3), np.float32), count=np.zeros(0, np.int64), key=np.zeros(0, np.uint64), total=0, status=BAD_POSE)
    m = np.asarray(ext["xyz"], np.float32).reshape(-1, 3)
    R = T[:3, :3].astype(np.float64); t = T[:3, 3].astype(np.float64)
    mn, mx = float(np.float32(min_range)), float(np.float32(max_range))
    with np.errstate(all="ignore"):
        d = m.astype(np.float64) - t[None, :]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = (np.asarray(ext["count"]) >= max(1, int(min_points))) & (d2 > mn * mn) & ((mx <= 0) | (d2 <= mx * mx))
        if world:
            rows = m.copy()
        else:
            rows = np.stack([((R[0, a] * d[:, 0] + R[1, a] * d[:, 1]) + R[2, a] * d[:, 2]).astype(np.float32) for a in range(3)], axis=1)
    sel = np.flatnonzero(keep)                                        # the extract is in ascending key order: so is this
    total = int(sel.shape[0])
    status = 0
    if cap_rows is not None and total > cap_rows:
        sel = sel[:int(cap_rows)]; status |= TRUNCATED
    return dict(xyz=np.ascontiguousarray(rows[sel], np.float32).reshape(-1, 3), count=np.asarray(ext["count"], np.int64)[sel],
                key=np.asarray(ext["key"], np.uint64)[sel], total=total, status=status)


def query(model, poses, **kw):
    """One query_extract per pose of ``poses`` on a map_model.Map."""
    ext = model.extract(1)
    return [query_extract(ext, T, **kw) for T in np.asarray(poses, np.float32).reshape(-1, 4, 4)]


def x_interval(pose, cell, max_range, prune=True):
    """The run of x cells a query can reach (the pruning of the kernels): (lo, hi); empty (lo > hi) for an unusable pose."""
    lim = 1 << 20
    T = np.asarray(pose, np.float32).reshape(4, 4)
    if not pose_ok(T):
        return lim, -lim
    mx = np.float32(max_range)
    if not prune or not mx > 0:
        return -lim, lim
    inv = 1.0 / float(np.float32(cell))
    a = np.floor((float(T[0, 3]) - float(mx)) * inv) - 1.0
    b = np.floor((float(T[0, 3]) + float(mx)) * inv) + 1.0
    lo = -lim if not a > -lim else (int(a) if a < lim else lim)
    hi = lim if not b < lim else (int(b) if b > -lim else -lim)
    return lo, hi


def next_f32(v, up=True):
    """The float32 one ulp above (below) v."""
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)).astype(np.float32)
