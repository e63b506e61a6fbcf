"""CPU tests of the voxel map's shape MODEL (tests/map_shape_model.py): the properties the integer moments promise, the covariance against a
float64 covariance of the rows, the accuracy of the normals on a noisy plane, and the sweep count of the Jacobi.  These measure the model, never the device code;
the device is held to the model bit for bit in tests/test_map_shape.py."""
import numpy as np
import pytest

import map_model as mm
import map_shape_model as sm

CELL = 0.5


@pytest.fixture(scope="module")
def plane():
    rows = sm.plane_rows()
    T = mm.pose()
    ex = sm.ShapeMap(CELL).add([rows], [T]).extract_shape()
    _, key, _, _ = mm.classify(rows, T, CELL)
    W = sm.world_rows(rows, T)
    order = np.argsort(key, kind="stable")
    uk, start = np.unique(key[order], return_index=True)
    end = np.append(start[1:], order.shape[0])
    assert np.array_equal(uk, ex["key"])
    return dict(ex=ex, cells=[W[order[s:e]] for s, e in zip(start, end)])


def _scans():
    rs = np.random.RandomState(11)
    scans = [(rs.randn(700, 3) * [2, 2, 0.5]).astype(np.float32) for _ in range(3)]
    poses = np.stack([mm.pose(t=(0.3 * k, -0.2 * k, 0.1), r=(0.01, 0.02, 0.3 * k)) for k in range(3)])
    return scans, poses


def test_moments_do_not_depend_on_order_or_on_how_a_scan_is_split():
    scans, poses = _scans()
    want = sm.ShapeMap(0.5).add(scans, poses)
    rs = np.random.RandomState(12)
    perm = [s[rs.permutation(s.shape[0])] for s in scans]
    split = [p for s in scans for p in (s[:123], s[123:])]
    for got in (sm.ShapeMap(0.5).add(perm[::-1], poses[::-1]), sm.ShapeMap(0.5).add(split, np.repeat(poses, 2, axis=0))):
        assert got.cells == want.cells and got.mom == want.mom
    assert len(want.mom) == len(want.cells) > 100 and max(e[0] for e in want.cells.values()) > 5


def test_add_then_remove_leaves_all_zero_words():
    scans, poses = _scans()
    m = sm.ShapeMap(0.5).add(scans, poses).remove(scans[1:], poses[1:]).remove(scans[:1], poses[:1])
    assert all(e == [0] * sm.WORDS for e in m.mom.values()) and all(e == [0, 0, 0, 0] for e in m.cells.values())
    # a remove alone: the words are the two's complement of the add's
    a = sm.ShapeMap(0.5).add(scans[:1], poses[:1]); r = sm.ShapeMap(0.5).remove(scans[:1], poses[:1])
    for k in a.mom:
        assert [(x + y) & sm.MASK for x, y in zip(a.words(k), r.words(k))] == [0] * sm.WORDS


def test_a_cell_of_one_row_has_exactly_zero_covariance_and_the_normal_x():
    rs = np.random.RandomState(13)
    rows = (rs.rand(200, 3) * 400 - 200).astype(np.float32)           # 200 rows over 400 m: one row per cell
    for cell in (0.1, 0.5):
        ex = sm.ShapeMap(cell).add([rows], [mm.pose()]).extract_shape()
        assert (ex["count"] == 1).all() and ex["key"].shape[0] == 200
        assert not ex["cov64"].any() and not ex["evals"].any()
        assert np.array_equal(ex["normal"], np.tile(np.array([1, 0, 0], np.float32), (200, 1)))
    # offsets 0 and 65535, alone: h^2 is exact on both sides
    for h in (0, 65535):
        assert not sm.cov(1, [h, h, h] + [h * h] * 6, 0.1).any()


def test_covariance_against_a_float64_covariance_of_the_rows(plane):
    """The rule differs from np.cov(rows, bias=True) in float64 by the truncation of the offsets to 16 bits only.  Measured on the 520 cells of count >= 10 of the
    noisy plane at a 0.5 m cell: max |C - C_ref| / max |C_ref| = 1.70e-5 (median 3.2e-6); asserted at twice the measured maximum."""
    ex = plane["ex"]
    rel = []
    for i, P in enumerate(plane["cells"]):
        assert P.shape[0] == ex["count"][i]
        if P.shape[0] < 10:
            continue
        ref = np.cov(P.T, bias=True)
        rel.append(np.abs(sm.cov_matrix(ex["cov64"][i]) - ref).max() / np.abs(ref).max())
    rel = np.array(rel)
    print("cells %d  max relative difference %.3e  median %.3e" % (rel.shape[0], rel.max(), np.median(rel)))
    assert rel.shape[0] == 520
    assert rel.max() <= 2 * 1.70e-5


def test_normals_of_a_noisy_plane(plane):
    """Cells of count >= 10 of the plane z = 0.3 x + 0.1 y + 2 (sigma 0.02 along the normal, 0.5 m cell): measured median angle to the true normal 1.43 degrees,
    95th percentile 9.8 degrees (the tail: slivers a cell boundary cuts off).  The median is asserted at 1.5 times the measured value."""
    ex = plane["ex"]
    big = ex["count"] >= 10
    n = ex["normal"][big].astype(np.float64)
    ang = np.degrees(np.arcsin(np.clip(np.linalg.norm(np.cross(n, sm.PLANE_NORMAL), axis=1), 0, 1)))
    print("cells %d  median %.3f deg  95th percentile %.3f deg" % (big.sum(), np.median(ang), np.percentile(ang, 95)))
    assert big.sum() == 520
    assert np.median(ang) <= 1.5 * 1.43
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
    f = _features(ex["evals"][big])
    assert np.median(f["planarity"]) > 0.5 and np.median(f["sphericity"]) < 0.05


def _features(evals):
    from icet_amd import api
    return api.shape_features(evals)


def test_six_sweeps_suffice_and_the_jacobi_agrees_with_eigh(plane):
    """After SWEEPS sweeps the off-diagonal is below 4e-16 of the largest eigenvalue on every cell of the plane (measured: 7.1e-16 after 3 sweeps, 3.2e-64 after 4,
    exactly 0 after 6); the eigenvalues are eigh's within 1e-6 of the largest, and the smallest stays above -1e-13 of it (measured -2.3e-14)."""
    ex = plane["ex"]
    assert sm.SWEEPS == 6
    worst, lowest = 0.0, 0.0
    for C in ex["cov64"]:
        A, _ = sm.jacobi(C)
        d = [A[0][0], A[1][1], A[2][2]]
        lam = max(abs(v) for v in d)
        if lam == 0:
            continue
        worst = max(worst, max(abs(A[0][1]), abs(A[0][2]), abs(A[1][2])) / lam)
        lowest = min(lowest, min(d) / lam)
    print("off-diagonal / largest %.3e  lowest eigenvalue / largest %.3e" % (worst, lowest))
    assert worst <= 4e-16 and lowest >= -1e-13
    ref = np.linalg.eigvalsh(sm.cov_matrix(ex["cov64"]))
    assert (np.abs(ex["evals"].astype(np.float64) - ref) <= 1e-6 * ref[:, 2:3] + 1e-300).all()
    assert (np.diff(ex["evals"].astype(np.float64), axis=1) >= 0).all()


def test_theta_may_overflow_and_ties_go_to_the_lowest_column():
    ev, n = sm.eigen([1.0, 1e-300, 0.0, 3.0, 0.0, 2.0])              # theta = 2 / 2e-300 overflows nothing; (1e300)^2 does: t = 0
    assert list(ev) == [1.0, 2.0, 3.0] and list(n) == [1.0, 0.0, 0.0]
    ev, n = sm.eigen([2.0, 0.0, 0.0, 1.0, 0.0, 1.0])                 # a tie between columns 1 and 2
    assert list(ev) == [1.0, 1.0, 2.0] and list(n) == [0.0, 1.0, 0.0]
    ev, n = sm.eigen([1.0, -1.0, 0.0, 1.0, 0.0, 5.0])                # eigenvector (1, 1, 0) / sqrt 2 up to sign: equal magnitudes, the lowest axis is made positive
    assert list(ev[:2]) == [0.0, 2.0] and n[0] > 0 and abs(abs(n[0]) - abs(n[1])) < 1e-7


def test_cov_matrix_and_shape_features():
    from icet_amd import api
    c = np.arange(12, dtype=np.float32).reshape(2, 6)
    m = api.cov_matrix(c)
    assert m.shape == (2, 3, 3) and m.dtype == np.float32 and np.array_equal(m, np.transpose(m, (0, 2, 1)))
    assert np.array_equal(m[1], [[6, 7, 8], [7, 9, 10], [8, 10, 11]]) and np.array_equal(m, sm.cov_matrix(c))
    f = api.shape_features(np.array([[0, 0, 0], [0, 0, 2], [0, 2, 2], [2, 2, 2], [-1e-9, 1, 4]], np.float32))
    assert np.array_equal(f["linearity"][:4], [0, 1, 0, 0]) and np.array_equal(f["planarity"][:4], [0, 0, 1, 0]) and np.array_equal(f["sphericity"][:4], [0, 0, 0, 1])
    assert abs(f["linearity"][4] - 0.75) < 1e-6 and abs(f["planarity"][4] - 0.25) < 1e-6
