"""Properties of the query's NumPy model (tests/map_query_model.py; the rule: include/icet_hip.h icet_voxel_map_query_*) that the GPU
tests rely on: the world-frame query of everything is the extract, the identity pose changes no row, disjoint shells partition the map, and the boundary
table has the classes the other tests take for granted."""
import numpy as np

import map_model as mm
import map_query_model as qm


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cloud_map(seed=11, n=3000, cell=0.1):
    rs = np.random.RandomState(seed)
    scans = [(rs.randn(n, 3) * [8, 8, 1.5]).astype(np.float32) for _ in range(3)]
    poses = np.stack([mm.pose(t=(k, -0.5 * k, 0.1), r=(0.01, -0.02, 0.4 * k)) for k in range(3)])
    return mm.Map(cell).add(scans, poses)


def boundary_map():
    """Single-point cells at exact multiples of 0.125 (cell 0.125: the centroids are the points), and the points one float32 ulp further out."""
    pts = np.array([[3, 4, 0], [5, 12, 0], [qm.next_f32(4), 3, 0], [qm.next_f32(12), 5, 0], [0, 0, 0], [0.125, 0, 0]], np.float32)      # (each in a cell of its own)
    # min_range 0: the map keeps every row but the all-zero one, which no scan can add
    return mm.Map(0.125).add([pts], mm.pose()[None]), pts


def test_world_query_of_everything_is_the_extract():
    model = _cloud_map()
    ext = model.extract(1)
    T = mm.pose(t=(0.123, 4.5, -0.7), r=(0.3, 0.2, 0.1))             # t is no centroid
    got = qm.query(model, T[None], world=True)[0]
    assert got["total"] == ext["key"].shape[0] > 2000 and got["status"] == 0
    assert np.array_equal(got["key"], ext["key"]) and np.array_equal(got["count"], ext["count"]) and np.array_equal(_bits(got["xyz"]), _bits(ext["xyz"]))
    for mp in (2, 3):
        e = model.extract(mp)
        g = qm.query(model, T[None], world=True, min_points=mp)[0]
        assert np.array_equal(g["key"], e["key"]) and np.array_equal(_bits(g["xyz"]), _bits(e["xyz"]))
    assert np.all(got["key"][1:] > got["key"][:-1])                   # ascending keys


def test_identity_pose_gives_the_world_rows():
    model = _cloud_map(12)
    I = mm.pose()[None]
    a, b = qm.query(model, I, max_range=6.0)[0], qm.query(model, I, max_range=6.0, world=True)[0]
    assert a["total"] == b["total"] > 100 and np.array_equal(a["key"], b["key"])
    assert np.array_equal(_bits(a["xyz"]), _bits(b["xyz"]))


def test_disjoint_shells_partition_the_map():
    model = _cloud_map(13)
    ext = model.extract(1)
    T = mm.pose(t=(1.0, -2.0, 0.3), r=(0, 0, 1.0))[None]
    for r in (0.5, 3.0, 7.5, 40.0):
        inner, outer = qm.query(model, T, max_range=r)[0], qm.query(model, T, min_range=r)[0]
        assert inner["total"] + outer["total"] == ext["key"].shape[0]
        assert not set(inner["key"].tolist()) & set(outer["key"].tolist())
        assert np.array_equal(np.sort(np.concatenate([inner["key"], outer["key"]])), ext["key"])


def test_boundary_table_has_the_classes_it_is_used_for():
    model, pts = boundary_map()
    ext = model.extract(1)
    assert ext["key"].shape[0] == 5 and (ext["count"] == 1).all()     # the all-zero row never entered the map
    assert set(map(tuple, _bits(ext["xyz"]).tolist())) == set(map(tuple, _bits(pts[[0, 1, 2, 3, 5]]).tolist()))      # the centroids are the points, exactly
    I = mm.pose()[None]

    def kept(**kw):
        return set(map(tuple, qm.query(model, I, world=True, **kw)[0]["xyz"].tolist()))
    p = [tuple(float(v) for v in r) for r in pts]
    assert p[0] in kept(max_range=5.0) and p[0] not in kept(min_range=5.0)
    assert p[2] not in kept(max_range=5.0) and p[2] in kept(min_range=5.0)        # one ulp further out flips both
    assert p[1] in kept(max_range=13.0) and p[1] not in kept(min_range=13.0)
    assert p[3] not in kept(max_range=13.0) and p[3] in kept(min_range=13.0)
    # a centroid exactly at the query's origin is dropped at min_range 0, as all-zero rows are
    T = mm.pose(t=(0.125, 0, 0))[None]
    assert qm.query(model, T)[0]["total"] == 4 and qm.query(model, I)[0]["total"] == 5


def test_truncation_bad_poses_and_the_run_of_x_cells():
    model = _cloud_map(14)
    T = mm.pose(t=(0.5, 0.5, 0), r=(0, 0, 0.3))
    full = qm.query(model, T[None], max_range=5.0)[0]
    cut = qm.query(model, T[None], max_range=5.0, cap_rows=full["total"] - 1)[0]
    assert cut["status"] == qm.TRUNCATED and cut["total"] == full["total"] and np.array_equal(cut["key"], full["key"][:-1])
    assert qm.query(model, T[None], max_range=5.0, cap_rows=full["total"])[0]["status"] == 0
    for j in range(12):
        for v in (np.nan, np.inf, -np.inf):
            B = T.copy(); B.reshape(-1)[j] = v
            r = qm.query(model, B[None], max_range=5.0)[0]
            assert r["total"] == 0 and r["status"] == qm.BAD_POSE and r["xyz"].shape == (0, 3)
            assert qm.x_interval(B, 0.1, 5.0)[0] > qm.x_interval(B, 0.1, 5.0)[1]
    B = T.copy(); B[3, 1] = np.nan                                    # the last row is never read
    assert qm.query(model, B[None], max_range=5.0)[0]["total"] == full["total"]
    # every kept cell lies in the run of x cells the kernels prune to
    lo, hi = qm.x_interval(T, 0.1, 5.0)
    cx = mm.key_cells(full["key"])[:, 0]
    assert lo <= cx.min() and cx.max() <= hi and hi - lo <= 2 * 50 + 4
    assert qm.x_interval(T, 0.1, 0.0) == (-(1 << 20), 1 << 20) and qm.x_interval(T, 0.1, 5.0, prune=False) == (-(1 << 20), 1 << 20)
