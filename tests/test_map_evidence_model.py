"""Properties of the NumPy model of a voxel map's visibility evidence (tests/map_evidence_model.py): the sums are sums, order is free, the
thresholds tie the way the rule says, the octahedral pixel of the directions where it can go wrong, the windows at the image corners, and the drive with a car."""
import numpy as np

import map_evidence_cases as cases
import map_evidence_model as em
import map_model as mm

KW = dict(max_range=30.0, margin=0.3, min_range=0.5, image_log2=6, window=1, min_miss=2, agree_factor=1)


def _cloud(seed=5, n=4, rows=700):
    rs = np.random.RandomState(seed)
    scans = [(rs.randn(rows, 3) * [7, 7, 1.0]).astype(np.float32) for _ in range(n)]
    poses = np.stack([mm.pose(t=(k, -0.5 * k, 0.1), r=(0.01, -0.02, 0.4 * k)) for k in range(n)])
    return scans, poses, mm.Map(0.1).add(scans, poses)


def test_n_scans_in_one_call_are_the_sum_of_n_calls_and_order_is_free():
    scans, poses, model = _cloud()
    ext = model.extract(1)
    one = em.evidence_extract(ext, scans, poses, **KW)
    assert one["miss"].sum() > 50 and one["agree"].sum() > 500 and 0 < one["stats"]["cells_transient"] < ext["key"].shape[0]
    parts = [em.evidence_extract(ext, [s], T[None], **KW) for s, T in zip(scans, poses)]
    assert np.array_equal(one["miss"], sum(p["miss"] for p in parts)) and np.array_equal(one["agree"], sum(p["agree"] for p in parts))
    assert one["stats"]["rows_imaged"] == sum(p["stats"]["rows_imaged"] for p in parts)
    perm = [2, 0, 3, 1]
    other = em.evidence_extract(ext, [scans[k] for k in perm], poses[perm], **KW)
    for k in ("miss", "agree", "transient", "key"):
        assert np.array_equal(one[k], other[k])
    assert one["stats"] == other["stats"]
    assert np.array_equal(one["transient"], em.decide(one["miss"], one["agree"], 2, 1).astype(np.uint8))


def test_the_scan_that_built_the_map_agrees_with_its_own_cells():
    """A scan of the inside of a sphere (radius 10 +- 0.01 m): nothing stands in front of anything, so every pixel of every window holds the sphere, and a
    cell's centroid lies within a cell diagonal of the rows that made it."""
    rs = np.random.RandomState(8)
    dirs = rs.randn(6000, 3)
    scan = (dirs / np.linalg.norm(dirs, axis=1)[:, None] * (10.0 + rs.uniform(-0.01, 0.01, (6000, 1)))).astype(np.float32)
    model = mm.Map(0.1).add([scan], mm.pose()[None])
    ext = model.extract(1)
    diag = float(np.float32(0.1)) * np.sqrt(3.0)
    for window in (0, 1, 2):
        for mx, want in ((20.0, ext["key"].shape[0]), (9.0, 0)):      # inside the range: every cell; outside: none
            ev = em.evidence_extract(ext, [scan], mm.pose()[None], max_range=mx, margin=diag, min_range=0.0, image_log2=4, window=window)
            assert want == 0 or want > 5000
            assert int((ev["agree"] >= 1).sum()) == want and (ev["miss"] == 0).all() and not ev["transient"].any()


def test_an_empty_scan_and_no_scan_give_zeros():
    scans, poses, model = _cloud()
    ext = model.extract(1)
    for sc, T in (([np.zeros((0, 3), np.float32)], poses[:1]), ([], poses[:0]), ([np.full((5, 3), np.nan, np.float32)], poses[:1])):
        ev = em.evidence_extract(ext, sc, T, **KW)
        assert not ev["miss"].any() and not ev["agree"].any() and not ev["transient"].any()
        assert ev["stats"] == dict(rows_imaged=0, cells=ext["key"].shape[0], cells_transient=0, scans_used=len(sc), scans_bad_pose=0)


def test_a_non_finite_value_in_each_of_the_12_pose_entries():
    scans, poses, model = _cloud()
    ext = model.extract(1)
    good = em.evidence_extract(ext, scans[1:], poses[1:], **KW)
    for j in range(16):
        for v in (np.nan, np.inf, -np.inf):
            T = poses.copy(); T[0].reshape(-1)[j] = v
            ev = em.evidence_extract(ext, scans, T, **KW)
            if j < 12:
                assert ev["stats"]["scans_bad_pose"] == 1 and ev["stats"]["scans_used"] == 3
                assert np.array_equal(ev["miss"], good["miss"]) and np.array_equal(ev["agree"], good["agree"])
                assert ev["stats"]["rows_imaged"] == good["stats"]["rows_imaged"] + em.range_image(scans[0], KW["min_range"], 6)[1]
            else:                                                     # the last row of T is never read
                assert ev["stats"]["scans_bad_pose"] == 0 and ev["miss"].sum() > good["miss"].sum()


def test_the_tie_table():
    pt, table = cases.tie_cases()
    model = mm.Map(0.125).add([pt], mm.pose()[None])
    ext = model.extract(1)
    assert ext["xyz"].view(np.uint32).tolist() == pt.view(np.uint32).tolist()      # the centroid is the point
    seen = set()
    for c in table:
        row = np.array([c["scan_row"]], np.float32)
        ev = em.evidence_extract(ext, [row], mm.pose()[None], max_range=c["mx"], margin=c["mg"], min_range=c["mn"], image_log2=8, window=0, min_miss=1, agree_factor=0)
        got = "miss" if ev["miss"][0] else ("agree" if ev["agree"][0] else "none")
        assert got == c["want"] and ev["miss"][0] + ev["agree"][0] <= 1, c
        assert ev["transient"][0] == (got == "miss")
        seen.add(got)
    assert seen == {"miss", "agree", "none"}
    # the classes themselves: rn == rc + mg is agree, one ulp above is miss, rn == rc - mg is agree, one ulp below is occluded
    w = lambda v: np.array([v], np.float32).view(np.uint32)
    for rn, want in ((5.5, em.AGREE), (cases.nf(5.5), em.MISS), (4.5, em.AGREE), (cases.nf(4.5, False), em.OCCLUDED), (np.inf, em.MISS)):
        assert em.classes([25.0], w(rn), 0.5)[0] == want, rn
    assert em.classes([25.0], [em.EMPTY], 0.5)[0] == em.NONE
    # a scan row against min_range^2: (3, 4, 0) has d2 == 25
    rows = np.array([[3, 4, 0], [3, 4, 0.01], [0, 0, 0], [np.nan, 1, 1], [1, np.inf, 1], [0, 0, 1e-30]], np.float32)
    assert em.scan_rows(rows, 5.0, 8)[0].tolist() == [False, True, False, False, False, False]
    assert em.scan_rows(rows, cases.nf(5.0, False), 8)[0].tolist() == [True, True, False, False, False, False]
    assert em.scan_rows(rows, 0.0, 8)[0].tolist() == [True, True, False, False, False, True]
    # max_range does not apply to a scan's rows
    assert em.range_image(np.array([[3e38, 0, 0]], np.float32), 0.0, 4)[1] == 1


def test_the_decision_table():
    d = lambda m, a, mm_, f: bool(em.decide([m], [a], mm_, f)[0])
    assert not d(0, 0, 0, 0) and d(1, 0, 0, 0) and d(1, 5, 0, 0) and not d(1, 0, 2, 0) and d(2, 1, 2, 1) and not d(2, 2, 2, 1) and d(3, 2, 2, 1)
    assert not d(2 ** 31 - 1, 2, 1, 2 ** 30) and d(2 ** 31 - 1, 1, 1, 2 ** 30) and not d(2 ** 31 - 1, 2 ** 31 - 1, 1, 2 ** 31 - 1)      # products beyond 2^31


def test_the_direction_table():
    rows = cases.direction_rows()
    part, pix, word = em.scan_rows(rows, 0.0, 4)
    assert part.all()
    u, v = pix & 15, pix >> 4
    assert list(zip(u[:6].tolist(), v[:6].tolist())) == cases.AXIS_PIXELS_W16
    assert [(int(a), int(b)) for a, b in zip(u[6:9], v[6:9])] == [(15, 15), (15, 15), (8, 8)]      # -0.0 and +0.0 both fold to +1
    by = {tuple(r.view(np.uint32).tolist()): (int(a), int(b)) for r, a, b in zip(rows, u, v)}
    k = lambda *r: tuple(np.array(r, np.float32).view(np.uint32).tolist())
    assert by[k(1, 2, 0.0)] == by[k(1, 2, -0.0)] and by[k(-3, 1, 0.0)] == by[k(-3, 1, -0.0)]      # -0.0 is not below the horizon
    assert by[k(0.0, 1, -1)] == by[k(-0.0, 1, -1)] == (12, 15)        # px = +-0 -> sgn +1: (1 - 1/2, 1 - 0)
    assert by[k(1, 0.0, -1)] == by[k(1, -0.0, -1)] == (15, 12)
    assert by[k(0.0, -1, -1)] == (12, 0)
    assert by[k(1, 1, 0.0)] == by[k(1, 1, -0.0)] == (12, 12) and by[k(1, 1, -1.0)] == (13, 13) and by[k(-1, -1, 0.0)] == (4, 4) and by[k(-1, -1, -2.0)] == (2, 2)      # the fold keeps the diagonal
    assert by[k(0.25, 0.125, 0.625)] == (10, 9) and by[k(-1.0, 0.0, 0.0)] == (0, 8) and by[k(1.0, 0.0, 0.0)] == (15, 8)      # on a border: the upper pixel, clamped
    # a direction's pixel does not depend on its magnitude
    base = np.array([(1, 2, -1), (-3, 1, 2), (0.5, -0.25, -4), (1, 1, 1), (0, 0, -1), (-1, 0, 0)], np.float32)
    want = em.scan_rows(base, 0.0, 8)[1]
    for s in (1e-30, 3e38 / 4):
        rows_s = (base * np.float32(s)).astype(np.float32)
        part, pix, word = em.scan_rows(rows_s, 0.0, 8)
        assert part.all() and np.array_equal(pix, want)
    assert em.scan_rows(np.array([[3e38, 3e38, 3e38]], np.float32), 0.0, 8)[2][0] == 0x7F800000      # the range overflows float32: +inf, below the empty word


def test_windows_at_the_image_corners():
    W = 16
    img = np.full((W, W), em.EMPTY, np.uint32)
    f = lambda v: int(np.float32(v).view(np.uint32))
    img[0, 0] = f(3.0); img[0, W - 1] = f(4.0); img[W - 1, 0] = f(5.0); img[W - 1, W - 1] = f(6.0); img[7, 7] = f(1.0)
    for w in (0, 1, 2):
        near = em.near_image(img, w)
        cnt = lambda val: int((near == f(val)).sum())
        assert cnt(3.0) == cnt(4.0) == cnt(5.0) == cnt(6.0) == (w + 1) ** 2      # clipped: no wrap across the fold
        assert cnt(1.0) == (2 * w + 1) ** 2
        assert int((near == em.EMPTY).sum()) == W * W - 4 * (w + 1) ** 2 - (2 * w + 1) ** 2
        assert near[0, w] == f(3.0) and (w == W - 1 or near[0, w + 1] == em.EMPTY) and near[w, W - 1 - w] == f(4.0)
    img[1, 1] = f(2.0)
    assert em.near_image(img, 1)[0, 0] == f(2.0) and em.near_image(img, 0)[0, 0] == f(3.0) and em.near_image(img, 2)[3, 3] == f(2.0)


def test_the_drive_with_a_car():
    """rings 64, steps 1024: the movers leave, the rest stays."""
    d = cases.car_drive(64, 1024)
    ev = em.evidence_extract(d["ext"], d["scans"], d["poses"], max_range=40.0, margin=0.3, image_log2=8, window=1, min_miss=2, agree_factor=1)
    movers = cases.mover_cells(d["ext"]["xyz"], d["boxes"], d["ground"])
    tr = ev["transient"].astype(bool)
    n, nm = tr.shape[0], int(movers.sum())
    hit, false = int((tr & movers).sum()), int((tr & ~movers).sum())
    print("cells %d, movers %d, movers transient %d (%.1f %%), others transient %d (%.3f %%)" % (n, nm, hit, 100.0 * hit / nm, false, 100.0 * false / (n - nm)))
    assert nm > 1000
    assert hit >= 0.5 * nm
    assert false <= 0.002 * (n - nm)
