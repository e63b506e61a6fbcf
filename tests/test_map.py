"""The voxel map on the GPU (include/icet_hip.h icet_voxel_map_*) against the NumPy model of tests/map_model.py, BIT FOR BIT: the keys,
the counts and the three float32 coordinates of an extract, and the totals.  Every sum the kernels form is an integer, so nothing here has a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import map_model as mm
import map_query_model as qm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
LOG2 = 16                                                            # 65 536 entries: every map below fits with room, and a pass over the table is short


def _upload(scan, pad=3):
    """An N x 3 scan as a device buffer with leading dimension n + pad and NaN in the padding: (buffer, (ptr, n, ld))."""
    s = np.asarray(scan, np.float32).reshape(-1, 3)
    n = s.shape[0]; ld = n + pad
    h = np.full((3, max(ld, 1)), np.nan, np.float32)
    h[:, :n] = s.T
    b = torch.from_numpy(h).to(DEV)
    return b, (b.data_ptr(), n, ld)


def _descs(scans, pad=3):
    bufs = [_upload(s, pad) for s in scans]
    torch.cuda.synchronize(DEV)
    return [b for b, _ in bufs], [d for _, d in bufs]


def _same(got, want, what=""):
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert np.array_equal(got["key"], want["key"]), what
    assert np.array_equal(got["count"], want["count"]), what
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), what


def _both_paths(ctx):
    """The two forms of k_map_add (option "map_lds"); the default is restored by the caller's finally."""
    for lds in (1, 0):
        ctx.set_option("map_lds", lds)
        yield lds


def _check(ctx, scans, poses, cell=0.125, log2=LOG2, pad=3, **kw):
    """One add of all scans with either form of the kernel: extract and stats equal the model's."""
    from icet_amd import api
    want = mm.Map(cell, **kw).add(scans, poses).extract()
    keep, descs = _descs(scans, pad)
    try:
        for lds in _both_paths(ctx):
            m = api.VoxelMap(ctx, cell=cell, table_log2=log2, **kw)
            m.add_device(descs, np.asarray(poses, np.float32))
            _same(m.extract(), want, "map_lds %d" % lds)
            m.close()
    finally:
        ctx.set_option("map_lds", 1)
    return want


# ---- 0. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_change_nothing(gpu_ctx):
    from icet_amd import api
    lib = api.load_library()
    for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(table_log2=9), dict(table_log2=31), dict(min_range=float("nan"))):
        with pytest.raises(api.IcetError) as e:
            api.VoxelMap(gpu_ctx, **bad)
        assert e.value.status == api.ICET_ERR_BAD_ARG
    h = C.c_void_p()
    p = api.MapParams(0.1, 0.0, 0.0, 12, 1)
    assert lib.icet_voxel_map_create(gpu_ctx._h, C.byref(p), C.byref(h)) == api.ICET_ERR_BAD_ARG and not h.value
    m = api.VoxelMap(gpu_ctx, cell=0.125, table_log2=12)
    scan = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    keep, descs = _descs([scan])
    T = mm.pose()[None]
    m.add_device(descs, T)
    before = m.extract()
    ptr, n, ld = descs[0]
    A = api._dev_scans(descs)
    for args in ((-1, A, T.ctypes.data, 1), (1, A, T.ctypes.data, 0), (1, A, T.ctypes.data, 2), (1, None, T.ctypes.data, 1), (1, A, None, 1),
                 (1, api._dev_scans([(ptr, n, n - 1)]), T.ctypes.data, 1), (1, api._dev_scans([(ptr, -1, ld)]), T.ctypes.data, 1), (1, api._dev_scans([(0, n, ld)]), T.ctypes.data, 1)):
        assert lib.icet_voxel_map_add_device(m._h, *args) == api.ICET_ERR_BAD_ARG
        assert lib.icet_voxel_map_last_error(m._h)
    assert lib.icet_voxel_map_add_posed_device(m._h, 1, A, None, 1) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_stats(m._h, 1, None) == api.ICET_ERR_BAD_ARG
    s = api.MapStats()
    xyz = np.zeros((3, 4), np.float32)
    assert lib.icet_voxel_map_extract(m._h, 1, xyz.ctypes.data, 4, -1, None, None, C.byref(s)) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_extract(m._h, 1, xyz.ctypes.data, 1, 2, None, None, C.byref(s)) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_extract(m._h, 1, None, 4, 2, None, None, C.byref(s)) == api.ICET_ERR_BAD_ARG
    with pytest.raises(api.IcetError):
        gpu_ctx.set_option("map_lds_", 1)
    _same(m.extract(), before)
    m.add_device([], np.zeros((0, 4, 4), np.float32))                 # n = 0: nothing
    _same(m.extract(), before)
    m.clear()
    st = m.stats()
    assert st == dict.fromkeys(st, 0)
    m.close()


# ---- 1. the edge table, and the sizes at which the kernel takes another path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [0.125, 0.1])
def test_edge_table_and_sizes(gpu_ctx, cell):
    rs = np.random.RandomState(1)
    scans, poses = [], []
    for rows, T, _ in mm.edge_rows(cell):
        scans.append(rows); poses.append(T)
    r, _ = mm.range_rows()
    scans.append(r); poses.append(mm.pose())
    for k, n in enumerate((0, 1, 3, 4, 5, 255, 256, 257, 1025, 2047, 2048, 2049, 4100)):      # lane groups of 4, wave, trip and block boundaries
        s = (rs.randn(n, 3) * [3, 3, 1]).astype(np.float32)
        s[::7] = 0.0
        if n > 5:
            s[5, 1] = np.nan; s[3, 0] = np.inf
        scans.append(s); poses.append(mm.pose(t=(0.3 * k, -0.2 * k, 0.1), r=(0.01, 0.02, 0.3 * k)))
    for pad in (3, 4, 0):                                             # columns off and on 16-byte boundaries; ld = n
        want = _check(gpu_ctx, scans, np.stack(poses), cell=cell, pad=pad)
    st = want["stats"]
    assert st["points_nonfinite"] >= 3 + 2 * 8 and st["points_outside"] >= 8 and st["status"] == 0
    # with a range gate
    _check(gpu_ctx, scans, np.stack(poses), cell=cell, min_range=2.0, max_range=5.0)


# ---- 2. one cell: every lane of every wave on one LDS and one global address ----------------------------------------------------------------------------------
def test_one_cell(gpu_ctx):
    one = np.tile(np.array([[1.03, -2.01, 0.52]], np.float32), (4096, 1))
    want = _check(gpu_ctx, [one], mm.pose()[None])
    assert list(want["count"]) == [4096]
    rs = np.random.RandomState(2)
    inside = (np.array([1.0, -2.0, 0.5]) + rs.rand(4096, 3) * 0.1249).astype(np.float32)
    want = _check(gpu_ctx, [inside], mm.pose()[None])
    assert list(want["count"]) == [4096]


# ---- 3. distinct cells: the block's LDS table overflows into the direct path ----------------------------------------------------------------------------------
def test_distinct_cells(gpu_ctx):
    i = np.arange(4096)
    rows = np.stack([(i - 2048 + 0.5) * 0.125, np.full(4096, 1.0), np.full(4096, 1.0)], axis=1).astype(np.float32)
    want = _check(gpu_ctx, [rows], mm.pose()[None])
    assert want["key"].shape[0] == 4096 and (want["count"] == 1).all()
    twice = rows.copy(); twice[1::2] = twice[0::2]                    # every second row repeats
    want = _check(gpu_ctx, [twice], mm.pose()[None])
    assert want["key"].shape[0] == 2048 and (want["count"] == 2).all()
    # scattered over three axes, at a rotated pose
    rs = np.random.RandomState(3)
    cloud = (rs.rand(4096, 3) * [40, 40, 6] - [20, 20, 3]).astype(np.float32)
    _check(gpu_ctx, [cloud], mm.pose(t=(3, -2, 1), r=(0.02, -0.03, 0.7))[None])


# ---- 4. a table near full, and a full one ----------------------------------------------------------------------------------------------------------------------
def _line(n):
    i = np.arange(n)
    return np.stack([(i + 0.5) * 0.125, np.full(n, 1.0), (i % 7 + 0.5) * 0.125], axis=1).astype(np.float32)


def test_table_near_full_and_full(gpu_ctx):
    from icet_amd import api
    want = _check(gpu_ctx, [_line(1000)], mm.pose()[None], log2=10)
    assert want["key"].shape[0] == 1000 and want["stats"]["status"] == 0
    rows = _line(1500)
    model = mm.Map(0.125).add([rows], mm.pose()[None])
    kept_model = model.totals["points_kept"]
    keep, descs = _descs([rows])
    try:
        for lds in _both_paths(gpu_ctx):
            m = api.VoxelMap(gpu_ctx, cell=0.125, table_log2=10)
            m.add_device(descs, mm.pose()[None])
            got = m.extract()
            st = got["stats"]
            print("map_lds", lds, st)
            assert st["status"] & api.VOXEL_MAP_TABLE_FULL and st["points_dropped"] > 0
            assert st["points_kept"] + st["points_dropped"] == kept_model == 1500
            assert st["cells_out"] == got["key"].shape[0] <= 1024
            for k, c in zip(got["key"], got["count"]):
                assert 1 <= c <= model.cells[int(k)][0]
            m.close()
    finally:
        gpu_ctx.set_option("map_lds", 1)


# ---- 4b. the sorted cells of one map shrink and grow from extract to extract --------------------------------------------------------------------------------------
def _extract_device(m, cap, min_points):
    """extract_device into pre-filled buffers of `cap` rows (leading dimension cap + 5), as the dict of extract(); nothing beyond the rows is written."""
    dx = torch.full((3, cap + 5), -1.0, dtype=torch.float32, device=DEV)
    dc = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=DEV); dk = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize(DEV)
    st = m.extract_device(dx.data_ptr(), cap + 5, cap, min_points, dc.data_ptr(), dk.data_ptr())
    n = min(cap, st["cells_out"])
    assert (dx[:, n:] == -1.0).all() and (dc[n:] == -1).all() and (dk[n:] == -1).all()
    return dict(xyz=np.ascontiguousarray(dx[:, :n].cpu().numpy().T), count=dc[:n].cpu().numpy(), key=dk[:n].cpu().numpy().view(np.uint64), stats=st)


def test_sorted_cells_of_changing_size_one_map(gpu_ctx):
    """cells_out 3000, 17, 3000, 3500, 1, 0 on ONE map, extract and extract_device in turn: the select-and-sort buffers serve a smaller sort after a larger one and
    grow again, and between the steps a world-frame query that takes every cell (the index's buffers) equals the extract."""
    from icet_amd import api
    first = _line(3000)
    twice = first[np.arange(17) * 173 + 5] + np.float32(0.03)         # a second point in 17 of the cells ...
    second = np.concatenate([twice, twice[3:4]])                      # ... and a third in one of them
    more = _line(3500)[3000:]
    T = mm.pose()[None]
    far = mm.pose(t=(-1000.0, 0.0, 0.0))                              # every cell lies beyond min_range 0 of it
    model = mm.Map(0.125)
    m = api.VoxelMap(gpu_ctx, cell=0.125, table_log2=12)
    keep, descs = _descs([first, second, more])

    def step(what, min_points, cells, device):
        want = model.extract(min_points)
        assert want["key"].shape[0] == cells, what
        got = _extract_device(m, cells, min_points) if device else m.extract(min_points)
        _same(got, want, what)
        assert m.stats(min_points) == want["stats"], what
        q = m.query(far, min_points=min_points, world=True)[0]
        w = qm.query_extract(model.extract(1), far, min_points=min_points, world=True)
        assert (q["total"], q["status"]) == (w["total"], w["status"]) == (cells, 0), what
        for g in (w, want):                                           # the model's query, and the extract itself
            assert np.array_equal(q["key"], g["key"]) and np.array_equal(q["count"], g["count"]), what
            assert np.array_equal(q["xyz"].view(np.uint32), g["xyz"].view(np.uint32)), what

    m.add_device(descs[:1], T); model.add([first], T)
    step("3000 cells", 1, 3000, False)
    m.add_device(descs[1:2], T); model.add([second], T)
    step("17 cells of two points", 2, 17, True)
    step("3000 cells again", 1, 3000, False)
    m.add_device(descs[2:], T); model.add([more], T)
    step("3500 cells", 1, 3500, True)
    step("1 cell of three points", 3, 1, False)
    m.clear(); model.clear()
    step("cleared", 1, 0, True)
    m.close()


# ---- 5, 6, 9. several lidar scans ------------------------------------------------------------------------------------------------------------------------------
_DRIVE = {}


def _drive():
    """8 scans of scene 2000 (rings 16, steps 256, noise seeds 50 + k) along a line, their true poses, and poses with 0.01 rad and 5 cm of drift per frame."""
    if not _DRIVE:
        from icet_amd import lidar_sim
        scene = lidar_sim.make_scene(2000)
        true, drifted, scans = [], [], []
        for k in range(8):
            t = (-5.0 + 1.5 * k, -1.0 + 0.1 * k, 0.0); yaw = 0.05 * k
            T = mm.pose(t=t, r=(0, 0, yaw))
            true.append(T)
            drifted.append(mm.pose(t=(t[0] + 0.05 * k, t[1], t[2]), r=(0, 0, yaw + 0.01 * k)))
            s = lidar_sim.make_scan(scene, (np.array(t), T[:3, :3].astype(np.float64)), 50 + k, rings=16, steps=256)
            scans.append(np.ascontiguousarray(s.cpu().numpy().T))
        _DRIVE.update(scans=scans, true=np.stack(true), drifted=np.stack(drifted))
        _DRIVE["model_true"] = mm.Map(0.1).add(scans, _DRIVE["true"]).extract()
        _DRIVE["model_drifted"] = mm.Map(0.1).add(scans, _DRIVE["drifted"]).extract()
    return _DRIVE


def test_several_scans_any_order_any_split_either_path(gpu_ctx):
    from icet_amd import api
    d = _drive()
    scans, poses, want = d["scans"], d["true"], d["model_true"]
    assert all(3000 < s.shape[0] <= 4096 for s in scans)
    keep, descs = _descs(scans)
    try:
        for lds in _both_paths(gpu_ctx):
            m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2)
            m.add_device(descs, poses)
            _same(m.extract(), want, "one call")
            m.clear()
            for k in range(8):
                m.add_device(descs[k:k + 1], poses[k:k + 1])
            _same(m.extract(), want, "eight calls")
            m.clear()
            m.add_device(descs[::-1], poses[::-1])
            _same(m.extract(), want, "reversed")
            m.close()
        m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2)
        m.add(scans, poses)                                          # the host form
        _same(m.extract(), want, "host arrays")
        m.close()
    finally:
        gpu_ctx.set_option("map_lds", 1)


def test_repose_equals_rebuild(gpu_ctx):
    from icet_amd import api
    d = _drive()
    scans, true, drifted = d["scans"], d["true"], d["drifted"]
    final = np.concatenate([drifted[:3], true[3:]])
    want = mm.Map(0.1).add(scans, drifted).remove(scans[3:], drifted[3:]).add(scans[3:], true[3:]).extract()
    fresh_model = mm.Map(0.1).add(scans, final).extract()
    assert np.array_equal(want["key"], fresh_model["key"]) and np.array_equal(want["xyz"].view(np.uint32), fresh_model["xyz"].view(np.uint32))
    keep, descs = _descs(scans)
    try:
        for lds in _both_paths(gpu_ctx):
            m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2)
            m.add_device(descs, drifted)
            _same(m.extract(), d["model_drifted"], "drifted")
            m.remove_device(descs[3:], drifted[3:])
            m.add_device(descs[3:], true[3:])
            got = m.extract()
            _same(got, want, "re-posed")
            fresh = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2)
            fresh.add_device(descs, final)
            f = fresh.extract()
            for k in ("key", "count"):
                assert np.array_equal(got[k], f[k])
            assert np.array_equal(got["xyz"].view(np.uint32), f["xyz"].view(np.uint32))
            assert got["stats"]["cells_negative"] == 0 and got["stats"]["cells_out"] == f["stats"]["cells_out"] == got["stats"]["cells_occupied"]
            gone = set(int(k) for k in d["model_drifted"]["key"]) - set(int(k) for k in f["key"])
            assert gone and not gone & set(int(k) for k in got["key"])      # cells the remove emptied do not appear
            fresh.close()
            # a remove of a scan never added
            m.clear()
            m.remove_device(descs[:1], true[:1])
            st = m.stats()
            assert st["status"] & api.VOXEL_MAP_NEGATIVE and st["cells_negative"] > 0 and st["cells_out"] == 0
            assert st == mm.Map(0.1).remove(scans[:1], true[:1]).stats()
            assert m.extract()["key"].shape[0] == 0
            m.close()
    finally:
        gpu_ctx.set_option("map_lds", 1)


def test_true_poses_give_fewer_cells_than_drifted_ones(gpu_ctx):
    from icet_amd import api
    d = _drive()
    keep, descs = _descs(d["scans"])
    cells = {}
    for name in ("true", "drifted"):
        model = mm.Map(0.25).add(d["scans"], d[name]).stats()
        m = api.VoxelMap(gpu_ctx, cell=0.25, table_log2=LOG2)
        m.add_device(descs, d[name])
        cells[name] = m.stats()["cells_out"]
        assert cells[name] == model["cells_out"]
        m.close()
    print("cells at cell 0.25: true poses %d, drifted poses %d" % (cells["true"], cells["drifted"]))
    assert cells["true"] < cells["drifted"]


# ---- 7. poses in HBM -------------------------------------------------------------------------------------------------------------------------------------------
def test_poses_on_the_device_from_the_optimiser(gpu_ctx):
    from icet_amd import api
    import pose_graph_cases as pc
    g = pc.graph(6, pc.CASES[3][1], pc.CASES[3][2], True)
    t = [torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(DEV) for k in ("poses", "odo_X", "odo_info")]
    res = gpu_ctx.optimize_pose_graph_device(t[0], t[1], t[2], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL)
    d_poses = res["poses"]
    assert d_poses.is_cuda and tuple(d_poses.shape) == (6, 4, 4)
    h_poses = d_poses.cpu().numpy()
    scans = _drive()["scans"][:6]
    keep, descs = _descs(scans)
    want = mm.Map(0.1).add(scans, h_poses).extract()
    a = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2); b = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2)
    a.add_device(descs, d_poses)
    b.add_device(descs, h_poses)
    ea, eb = a.extract(), b.extract()
    _same(ea, eb); _same(ea, want)
    a.remove_device(descs, d_poses)
    assert a.stats()["cells_occupied"] == 0 and a.stats()["cells_negative"] == 0 and a.stats()["points_kept"] == 0
    a.close(); b.close()


# ---- 8. real scans ---------------------------------------------------------------------------------------------------------------------------------------------
def test_real_scans_min_points_and_truncation(gpu_ctx, frames, frames_golden):
    from icet_amd import api
    a, b = frames
    poses = np.stack([np.eye(4, dtype=np.float32), api.pose_step_from_X(frames_golden["X"])])
    model = mm.Map(0.1).add([a, b], poses)
    keep, descs = _descs([a, b], pad=1)
    m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=20)
    m.add_device(descs, poses)
    for mp in (1, 2, 5):
        want = model.extract(mp)
        _same(m.extract(mp), want, "min_points %d" % mp)
        assert m.stats(mp) == want["stats"]
    zeros = int((np.abs(a).max(axis=1) == 0).sum() + (np.abs(b).max(axis=1) == 0).sum())
    st = m.stats()
    assert st["points_kept"] == a.shape[0] + b.shape[0] - zeros and st["points_in"] == a.shape[0] + b.shape[0]
    cap = model.stats(2)["cells_out"] // 3
    got, want = m.extract(2, cap_rows=cap), model.extract(2, cap_rows=cap)
    assert got["stats"]["status"] & api.VOXEL_MAP_TRUNCATED and got["key"].shape[0] == cap
    _same(got, want, "truncated")
    # the device form: the same rows into a caller's buffers, leading dimension above the rows
    n = model.stats(1)["cells_out"]
    dx = torch.full((3, n + 5), -1.0, dtype=torch.float32, device=DEV); dc = torch.zeros(n, dtype=torch.int64, device=DEV); dk = torch.zeros(n, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize(DEV)
    st = m.extract_device(dx.data_ptr(), n + 5, n, 1, dc.data_ptr(), dk.data_ptr())
    want = model.extract(1)
    assert st == want["stats"]
    assert np.array_equal(dx[:, :n].cpu().numpy().T.view(np.uint32), want["xyz"].view(np.uint32)) and (dx[:, n:] == -1.0).all()
    assert np.array_equal(dc.cpu().numpy(), want["count"]) and np.array_equal(dk.cpu().numpy().view(np.uint64), want["key"])
    m.close()


# ---- 10, 11. the output is a scan; nothing else is disturbed ---------------------------------------------------------------------------------------------------
def test_extract_is_a_scan_a_store_accepts_and_nothing_else_is_disturbed(gpu_ctx, frames, frames_golden):
    import icet_amd
    from icet_amd import api
    a, b = frames
    before = gpu_ctx.solve(a, b, 7, np.zeros(6, np.float32), 24, 75)
    assert np.abs(before["X"] - frames_golden["X"]).max() < 3e-4
    store = icet_amd.KeyframeStore(gpu_ctx, 4)
    store.put([2], [a])
    slot_before = {k: np.array(store.debug_fetch(2, k)) for k in ("hot", "fit", "slot_of_voxel")}
    # a fused sub-map of three neighbouring scans, in the frame of the middle one
    from icet_amd import lidar_sim
    scene = lidar_sim.make_scene(2000)
    poses, scans = [], []
    for k in range(4):
        t = (-5.0 + 0.4 * k, -1.0, 0.0)
        T = mm.pose(t=t, r=(0, 0, 0.02 * k))
        poses.append(T)
        scans.append(np.ascontiguousarray(lidar_sim.make_scan(scene, (np.array(t), T[:3, :3].astype(np.float64)), 70 + k, rings=64, steps=1024).cpu().numpy().T))
    inv_mid = np.linalg.inv(poses[1].astype(np.float64))
    rel = np.stack([(inv_mid @ poses[k].astype(np.float64)).astype(np.float32) for k in range(3)])
    m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=20)
    m.add(scans[:3], rel)
    n = m.stats()["cells_out"]
    fused = torch.zeros((3, n), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    st = m.extract_device(fused.data_ptr(), n, n)
    assert st["cells_out"] == n > 10000 and st["status"] == 0
    store.put_device([0], [(fused.data_ptr(), n, n)])                 # the layout of a scan: straight into a store
    live, ld = _descs([scans[3]], pad=0)
    out = torch.zeros((1, 48), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    store.register_device([0], ld, api.Params(7, 24, 75, 25, 0.1, 0.1, 0), out.data_ptr())
    gpu_ctx.sync()
    X = out.cpu().numpy()[0, :6]
    print("a live scan against the fused map: X =", X)
    assert np.isfinite(X).all()
    m.close()
    # interference: the golden pair still solves to the same bits, and the store's other slot is unchanged
    after = gpu_ctx.solve(a, b, 7, np.zeros(6, np.float32), 24, 75)
    for k in ("X", "pred_stds", "cov"):
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32))
    for k, v in slot_before.items():
        assert np.array_equal(v, np.array(store.debug_fetch(2, k)))
    store.close()
