"""The voxel map's model (tests/map_model.py) held to its own properties: the contents depend on the multiset of (row, pose, sign)
only, remove + add at new poses is a fresh build, and the edge table of the rule."""
import numpy as np
import pytest

import map_model as mm


def _scans(seed=3, n_scans=4, n=300):
    r = np.random.RandomState(seed)
    scans = [(r.randn(n + 7 * k, 3) * [6, 6, 1.5]).astype(np.float32) for k in range(n_scans)]
    for s in scans:
        s[::17] = 0.0                                                # the exact-zero rows of real scans
    poses = np.stack([mm.pose(t=(0.4 * k, -0.3 * k, 0.02 * k), r=(0.01 * k, -0.02 * k, 0.15 * k)) for k in range(n_scans)])
    return scans, poses


def _same(a, b):
    assert np.array_equal(a["key"], b["key"]) and np.array_equal(a["count"], b["count"])
    assert np.array_equal(a["xyz"].view(np.uint32), b["xyz"].view(np.uint32))
    assert a["stats"] == b["stats"]


def test_order_and_call_splitting_do_not_matter():
    scans, poses = _scans()
    one = mm.Map(0.1).add(scans, poses).extract()
    split = mm.Map(0.1)
    for k in (2, 0, 3, 1):
        half = scans[k].shape[0] // 2
        split.add([scans[k][half:]], poses[k:k + 1]); split.add([scans[k][:half]], poses[k:k + 1])
    _same(one, split.extract())
    assert one["stats"]["points_kept"] == int(one["count"].sum()) and one["stats"]["status"] == mm.OK


def test_remove_then_add_at_new_poses_equals_a_fresh_build():
    scans, poses = _scans()
    drift = np.stack([mm.pose(t=(0.4 * k + 0.05 * k, -0.3 * k, 0.02 * k), r=(0.01 * k, -0.02 * k, 0.15 * k + 0.01 * k)) for k in range(4)])
    m = mm.Map(0.1).add(scans, drift)
    m.remove(scans[1:], drift[1:]).add(scans[1:], poses[1:])
    fresh = mm.Map(0.1).add(scans, poses).extract()
    got = m.extract()
    assert np.array_equal(got["key"], fresh["key"]) and np.array_equal(got["count"], fresh["count"])
    assert np.array_equal(got["xyz"].view(np.uint32), fresh["xyz"].view(np.uint32))
    assert got["stats"]["cells_negative"] == 0 and got["stats"]["points_kept"] == fresh["stats"]["points_kept"]
    assert all(e[0] >= 0 for e in m.cells.values()) and any(e[0] == 0 for e in m.cells.values())      # emptied cells stay in the dict, never in the extract
    assert all(e[1:] == [0, 0, 0] for e in m.cells.values() if e[0] == 0)
    # a remove of a scan never added
    neg = mm.Map(0.1).remove(scans[:1], poses[:1]).stats()
    assert neg["cells_negative"] > 0 and neg["status"] & mm.NEGATIVE


@pytest.mark.parametrize("cell", [0.125, 0.1])
def test_edge_table(cell):
    for rows, T, exp in mm.edge_rows(cell):
        cls, key, q, cells = mm.classify(rows, T, cell)
        for i, e in enumerate(exp):
            assert cls[i] == e["cls"], (rows[i], T, e)
            for a, ax in enumerate("xyz"):
                if "c" + ax in e:
                    assert cells[i, a] == e["c" + ax] and mm.key_cells(key[i])[a] == e["c" + ax]
                if "q" + ax in e:
                    assert int(q[i, a]) == e["q" + ax]
            if cls[i] == mm.KEPT:
                assert int(key[i]) < (1 << 63) and (q[i] < (1 << 32)).all()


def test_range_limits_are_exact():
    rows, exp = mm.range_rows()
    cls = mm.classify(rows, mm.pose(), 0.1, 5.0, 13.0)[0]
    assert list(cls) == exp
    assert list(mm.classify(rows, mm.pose(), 0.1, 0.0, 0.0)[0]) == [mm.KEPT] * 4 + [mm.RANGE]


def test_centroid_is_inside_its_cell_and_exact_for_one_point():
    T = mm.pose()
    p = np.array([[0.3125, -0.4375, 2.0625]], np.float32)              # multiples of 1 / 16: exact at cell 0.125
    got = mm.Map(0.125).add([p], T[None]).extract()
    assert np.array_equal(got["xyz"], p) and list(got["count"]) == [1]
    assert list(mm.key_cells(got["key"][0])) == [2, -4, 16]
