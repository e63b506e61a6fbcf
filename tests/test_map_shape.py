"""The voxel map's shape on the GPU (include/icet_hip.h icet_voxel_map_enable_shape / extract_shape) against the NumPy model of
tests/map_shape_model.py, BIT FOR BIT: the nine moment words, the six float32 covariance values, and the keys, counts and coordinates of the extract.  Every sum the
kernels form is an integer and the covariance is a fixed sequence of double operations, so nothing but the eigen-decomposition (test 10) has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_model as mm
import map_shape_model as sm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LOG2 = 16


def _upload(scan, pad=3, off=1):
    """An N x 3 scan as a device buffer with leading dimension n + pad, NaN in the padding, and the first row `off` floats into the allocation (off 1: every column
    is aligned to 4 bytes and to nothing more, whatever n): (buffer, (ptr, n, ld))."""
    s = np.asarray(scan, np.float32).reshape(-1, 3)
    n = s.shape[0]; ld = n + pad
    h = np.full(off + 3 * max(ld, 1), np.nan, np.float32)
    h[off:off + 3 * ld].reshape(3, ld)[:, :n] = s.T
    b = torch.from_numpy(h).to(DEV)
    return b, (b.data_ptr() + 4 * off, n, ld)


def _descs(scans, pad=3, off=1):
    bufs = [_upload(s, pad, off) for s in scans]
    torch.cuda.synchronize(DEV)
    return [b for b, _ in bufs], [d for _, d in bufs]


def _same(got, want, what=""):
    """Bit for bit: stats, key, count, xyz, and the moment words and float32 covariances where both sides carry them."""
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert np.array_equal(got["key"], want["key"]), what
    assert np.array_equal(got["count"], want["count"]), what
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), what
    for k in ("moments", "cov"):
        if k in got and k in want:
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
            assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
            bad = np.nonzero((a.view(np.uint8) != b.view(np.uint8)).reshape(a.shape[0], -1).any(axis=1))[0]
            assert bad.size == 0, (what, k, bad[:5], a[bad[:2]], b[bad[:2]])


def _both_paths(ctx):
    """The two forms of k_map_add (option "map_lds"); the default is restored by the caller's finally."""
    for lds in (1, 0):
        ctx.set_option("map_lds", lds)
        yield lds


def _check(ctx, scans, poses, cell=0.125, log2=LOG2, pad=3, off=1):
    """One add of all scans into a shaped map with either form of the kernel: extract_shape equals the model's."""
    from icet_amd import api
    want = sm.ShapeMap(cell).add(scans, poses).extract_shape(eig=False)
    keep, descs = _descs(scans, pad, off)
    try:
        for lds in _both_paths(ctx):
            m = api.VoxelMap(ctx, cell=cell, table_log2=log2, shape=True)
            m.add_device(descs, np.asarray(poses, np.float32))
            _same(m.extract_shape(moments=True), want, "map_lds %d" % lds)
            m.close()
    finally:
        ctx.set_option("map_lds", 1)
    return want


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
        _DRIVE["model_true"] = sm.ShapeMap(0.1).add(scans, _DRIVE["true"]).extract_shape(eig=False)
    return _DRIVE


# ---- 1. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu_ctx):
    from icet_amd import api
    lib = api.load_library()
    scan = np.array([[1, 2, 3], [4, 5, 6], [1.01, 2.01, 3.01]], np.float32)
    keep, descs = _descs([scan])
    T = mm.pose()[None]
    m = api.VoxelMap(gpu_ctx, cell=0.125, table_log2=12)
    m.add_device(descs, T)
    before = m.extract()
    with pytest.raises(api.IcetError) as e:                           # a plain map has no shape to extract
        m.extract_shape()
    assert e.value.status == api.ICET_ERR_BAD_ARG and "shape" in str(e.value)
    _same(m.extract(), before)
    with pytest.raises(api.IcetError) as e:                           # nor can it get one with rows in it
        m.enable_shape()
    assert e.value.status == api.ICET_ERR_BAD_ARG and not m.shape
    _same(m.extract(), before)
    m.clear()
    m.enable_shape(); m.enable_shape()                                # accepted on the cleared map, and again
    assert m.shape
    m.add_device(descs, T)
    want = sm.ShapeMap(0.125).add([scan], T).extract_shape(eig=False)
    before = m.extract_shape(moments=True)
    _same(before, want)
    n = before["key"].shape[0]
    assert n == 2
    xyz = np.zeros((3, 4), np.float32); cov = np.zeros((6, 4), np.float32); s = api.MapStats()
    ok = api.MapShape(cov.ctypes.data, None, None, None, 4, 0, 0)
    assert lib.icet_voxel_map_extract_shape(m._h, 1, xyz.ctypes.data, 4, 4, None, None, C.byref(ok), C.byref(s)) == api.ICET_OK
    cov[:] = 0; xyz[:] = 0
    for sh in (None, api.MapShape(cov.ctypes.data, None, None, None, 3, 0, 0), api.MapShape(cov.ctypes.data, None, None, None, 4, 1, 0),
               api.MapShape(cov.ctypes.data, None, None, None, 4, 0, 1)):
        st = lib.icet_voxel_map_extract_shape(m._h, 1, xyz.ctypes.data, 4, 4, None, None, C.byref(sh) if sh is not None else None, C.byref(s))
        assert st == api.ICET_ERR_BAD_ARG and lib.icet_voxel_map_last_error(m._h)
        assert not cov.any() and not xyz.any()
        _same(m.extract_shape(moments=True), before)
    for args in ((4, -1), (1, 2)):                                    # extract's own refusals hold for the shaped call
        assert lib.icet_voxel_map_extract_shape(m._h, 1, xyz.ctypes.data, args[0], args[1], None, None, C.byref(ok), C.byref(s)) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_extract_shape(m._h, 1, None, 4, 2, None, None, C.byref(ok), C.byref(s)) == api.ICET_ERR_BAD_ARG
    dx = torch.zeros((3, 4), dtype=torch.float32, device=DEV); dc = torch.zeros(8, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    odd = api.MapShape(None, None, None, dc.data_ptr() + 4, 4, 0, 0)  # uint64 words at an address that is 4 modulo 8
    assert lib.icet_voxel_map_extract_shape_device(m._h, 1, dx.data_ptr(), 4, 0, None, None, C.byref(odd), C.byref(s)) == api.ICET_ERR_BAD_ARG
    _same(m.extract_shape(moments=True), before)
    m.close()
    m = api.VoxelMap(gpu_ctx, cell=0.125, table_log2=12, shape=True)  # the constructor's form
    assert m.shape and m.extract_shape()["key"].shape[0] == 0
    m.close()


# ---- 2. the edge table, and the sizes at which the kernel takes another path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [0.1, 0.5])
def test_edge_table_and_sizes(gpu_ctx, cell):
    rs = np.random.RandomState(1)
    scans, poses = [], []
    for rows, T, _ in mm.edge_rows(cell):
        scans.append(rows); poses.append(T)
    r, _ = mm.range_rows()
    scans.append(r); poses.append(mm.pose())
    for k, n in enumerate((1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)):
        s = (rs.randn(n, 3) * [3, 3, 1]).astype(np.float32)
        s[::7] = 0.0
        if n > 5:
            s[5, 1] = np.nan; s[3, 0] = np.inf
        scans.append(s); poses.append(mm.pose(t=(0.3 * k, -0.2 * k, 0.1), r=(0.01, 0.02, 0.3 * k)))
    want = _check(gpu_ctx, scans, np.stack(poses), cell=cell, pad=3, off=1)      # columns at 4-byte-only alignment: the scalar loads
    _check(gpu_ctx, scans, np.stack(poses), cell=cell, pad=4, off=0)             # 16-byte loads where n allows
    st = want["stats"]
    assert st["points_nonfinite"] >= 3 + 2 * 8 and st["points_outside"] >= 8 and st["status"] == 0
    assert want["count"].max() >= 2 and want["cov"].any()


# ---- 3. one cell: every lane of every wave on one LDS slot and one table entry ---------------------------------------------------------------------------------
def test_one_cell(gpu_ctx):
    rs = np.random.RandomState(2)
    # cell (-1, 8, 4) at 0.125 m: x in [-0.125, 0), y in [1, 1.125), z in [0.5, 0.625)
    a = (np.array([-0.125, 1.0, 0.5]) + rs.rand(2049, 3) * 0.1249).astype(np.float32)
    a[:1100, 0] = -1e-29                                              # q_x = 2^32 - 1, h_x = 65535: more than half of each block
    a[7] = [-0.125, 1.0, 0.5]                                         # every offset 0
    a[2048] = [-1e-29, 1.0, 0.5]
    b = a.copy()
    b[:, 0] = -1e-29; b[:, 1] = np.nextafter(np.float32(1.125), np.float32(0)); b[:, 2] = np.nextafter(np.float32(0.625), np.float32(0))
    for scan in (a, b):                                               # b: every row at the top of the cell -- the largest sums a block's 32-bit S and 64-bit M see
        want = _check(gpu_ctx, [scan], mm.pose()[None])
        assert list(want["count"]) == [2049]
    assert int(want["moments"][0, 0]) == 2049 * 65535 and int(want["moments"][0, 3]) == 2049 * 65535 * 65535
    for scan in (a, b):                                               # the same scan 64 times in one call: 131 136 rows in one cell, 128 blocks on one entry
        want = _check(gpu_ctx, [scan] * 64, np.tile(mm.pose()[None], (64, 1, 1)))
        assert list(want["count"]) == [64 * 2049]
    assert int(want["moments"][0, 3]) == 64 * 2049 * 65535 * 65535 > 1 << 48


# ---- 4. 4096 distinct cells: the block's LDS table overflows into the direct path -------------------------------------------------------------------------------
def test_distinct_cells(gpu_ctx):
    rs = np.random.RandomState(3)
    i = np.arange(4096)
    rows = np.stack([(i - 2048) * 0.125 + rs.rand(4096) * 0.12, 1.0 + rs.rand(4096) * 0.12, 1.0 + rs.rand(4096) * 0.12], axis=1).astype(np.float32)
    want = _check(gpu_ctx, [rows], mm.pose()[None])
    assert want["key"].shape[0] == 4096 and (want["count"] == 1).all() and not want["cov"].any()
    twice = rows.copy(); twice[1::2, 0] = twice[0::2, 0]              # every second row falls into the cell before it
    want = _check(gpu_ctx, [twice], mm.pose()[None])
    assert want["key"].shape[0] == 2048 and (want["count"] == 2).all() and want["cov"][:, 3].all()
    cloud = (rs.rand(4096, 3) * [40, 40, 6] - [20, 20, 3]).astype(np.float32)
    _check(gpu_ctx, [cloud], mm.pose(t=(3, -2, 1), r=(0.02, -0.03, 0.7))[None])


# ---- 5. any order, any split, either form ------------------------------------------------------------------------------------------------------------------
def test_several_scans_any_order_any_split_either_form(gpu_ctx):
    from icet_amd import api
    d = _drive()
    scans, poses, want = d["scans"], d["true"], d["model_true"]
    assert all(3000 < s.shape[0] <= 4096 for s in scans) and want["count"].max() >= 5
    keep, descs = _descs(scans)
    got = []
    try:
        for lds in _both_paths(gpu_ctx):
            m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2, shape=True)
            m.add_device(descs, poses)
            got.append(m.extract_shape(moments=True)); _same(got[-1], want, "one call")
            m.clear()
            for k in range(8):
                m.add_device(descs[k:k + 1], poses[k:k + 1])
            got.append(m.extract_shape(moments=True)); _same(got[-1], want, "eight calls")
            m.clear()
            m.add_device(descs[::-1], poses[::-1])
            got.append(m.extract_shape(moments=True)); _same(got[-1], want, "reversed")
            m.close()
    finally:
        gpu_ctx.set_option("map_lds", 1)
    for g in got[1:]:                                                 # identical among themselves, eigenvalues and normals included
        for k in ("moments", "cov", "evals", "normal"):
            assert np.array_equal(g[k].view(np.uint8), got[0][k].view(np.uint8)), k


# ---- 6. re-pose equals rebuild, moments included ------------------------------------------------------------------------------------------------------------
def test_repose_equals_rebuild(gpu_ctx):
    from icet_amd import api
    d = _drive()
    scans, true, drifted = d["scans"], d["true"], d["drifted"]
    final = np.concatenate([drifted[:5], true[5:]])
    want = sm.ShapeMap(0.1).add(scans, drifted).remove(scans[5:], drifted[5:]).add(scans[5:], true[5:]).extract_shape(eig=False)
    fresh_model = sm.ShapeMap(0.1).add(scans, final).extract_shape(eig=False)
    for k in ("key", "count", "moments"):
        assert np.array_equal(want[k], fresh_model[k])
    keep, descs = _descs(scans)
    try:
        for lds in _both_paths(gpu_ctx):
            m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2, shape=True)
            m.add_device(descs, drifted)
            m.remove_device(descs[5:], drifted[5:])
            m.add_device(descs[5:], true[5:])
            got = m.extract_shape(moments=True)
            _same(got, want, "re-posed")
            fresh = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2, shape=True)
            fresh.add_device(descs, final)
            f = fresh.extract_shape(moments=True)
            for k in ("key", "count", "xyz", "moments", "cov", "evals", "normal"):
                assert np.array_equal(got[k].view(np.uint8), f[k].view(np.uint8)), k
            fresh.close()
            m.remove_device(descs, final)                             # everything: no rows, and the totals of kept rows return to zero
            e = m.extract_shape(moments=True)
            assert e["key"].shape[0] == 0 and e["stats"]["cells_negative"] == 0 and e["stats"]["points_kept"] == 0
            m.add_device(descs, final)                                # ... and every word did: the same map again
            again = m.extract_shape(moments=True)
            for k in ("key", "count", "xyz", "moments", "cov", "evals", "normal"):
                assert np.array_equal(again[k].view(np.uint8), f[k].view(np.uint8)), k
            m.close()
    finally:
        gpu_ctx.set_option("map_lds", 1)


# ---- 7. a plain map is untouched -----------------------------------------------------------------------------------------------------------------------------
def test_a_plain_map_and_a_shaped_map_read_alike(gpu_ctx):
    from icet_amd import api
    d = _drive()
    scans, true, drifted = d["scans"], d["true"], d["drifted"]
    keep, descs = _descs(scans)
    plain = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2); shaped = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2, shape=True)
    for m in (plain, shaped):
        m.add_device(descs, drifted)
        m.remove_device(descs[6:], drifted[6:])
        m.add_device(descs[6:], true[6:])
    for mp in (1, 3):
        ep, es = plain.extract(mp), shaped.extract(mp)
        _same(es, ep, "extract, min_points %d" % mp)
        assert plain.stats(mp) == shaped.stats(mp) == ep["stats"]
        _same(shaped.extract_shape(mp), ep, "extract_shape rows, min_points %d" % mp)
    assert plain.index() == shaped.index()
    far = mm.pose(t=(-1000.0, 0.0, 0.0))[None]                        # every cell lies beyond min_range 0 of it
    q = shaped.query(far, world=True)[0]
    e = shaped.extract()
    assert q["total"] == e["key"].shape[0] and q["status"] == 0
    assert np.array_equal(q["key"], e["key"]) and np.array_equal(q["count"], e["count"]) and np.array_equal(q["xyz"].view(np.uint32), e["xyz"].view(np.uint32))
    qp = plain.query(far, world=True)[0]
    assert np.array_equal(qp["key"], q["key"]) and np.array_equal(qp["xyz"].view(np.uint32), q["xyz"].view(np.uint32))
    plain.close(); shaped.close()


# ---- 8. poses in HBM -----------------------------------------------------------------------------------------------------------------------------------------
def test_poses_on_the_device(gpu_ctx):
    from icet_amd import api
    d = _drive()
    scans, poses = d["scans"], d["drifted"]
    keep, descs = _descs(scans)
    d_poses = torch.from_numpy(np.ascontiguousarray(poses, np.float32)).to(DEV)
    torch.cuda.synchronize(DEV)
    a = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2, shape=True); b = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2, shape=True)
    a.add_device(descs, d_poses)
    b.add_device(descs, poses)
    ea, eb = a.extract_shape(moments=True), b.extract_shape(moments=True)
    _same(ea, eb)
    _same(ea, sm.ShapeMap(0.1).add(scans, poses).extract_shape(eig=False))
    a.remove_device(descs, d_poses)
    assert a.stats()["cells_occupied"] == 0 and a.stats()["cells_negative"] == 0
    a.close(); b.close()


# ---- 9. cap_rows below cells_out ------------------------------------------------------------------------------------------------------------------------------
def test_truncation_writes_the_lowest_keys_and_nothing_beyond(gpu_ctx):
    from icet_amd import api
    d = _drive()
    keep, descs = _descs(d["scans"])
    m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2, shape=True)
    m.add_device(descs, d["true"])
    full = d["model_true"]
    total = full["key"].shape[0]
    cap, ld, sld = total // 3, total // 3 + 5, total // 3 + 9
    f = lambda cols, n: torch.full((cols, n), -7.0, dtype=torch.float32, device=DEV)
    dx, dcov, dn, de = f(3, ld), f(6, sld), f(3, sld), f(3, sld)
    dc = torch.full((ld,), -7, dtype=torch.int64, device=DEV); dk = torch.full((ld,), -7, dtype=torch.int64, device=DEV)
    dm = torch.full((9, sld), -7, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize(DEV)
    st = m.extract_shape_device(dx.data_ptr(), ld, cap, 1, dc.data_ptr(), dk.data_ptr(), dcov.data_ptr(), dn.data_ptr(), de.data_ptr(), dm.data_ptr(), shape_ld=sld)
    assert st["status"] & api.VOXEL_MAP_TRUNCATED and st["cells_out"] == total > cap
    for t in (dx, dcov, dn, de, dm):
        assert (t[:, cap:] == -7).all()
    assert (dc[cap:] == -7).all() and (dk[cap:] == -7).all()
    assert np.array_equal(dk[:cap].cpu().numpy().view(np.uint64), full["key"][:cap]) and np.array_equal(dc[:cap].cpu().numpy(), full["count"][:cap])
    assert np.array_equal(dx[:, :cap].cpu().numpy().T.view(np.uint32), full["xyz"][:cap].view(np.uint32))
    assert np.array_equal(dm[:, :cap].cpu().numpy().T.view(np.uint64), full["moments"][:cap])
    assert np.array_equal(dcov[:, :cap].cpu().numpy().T.view(np.uint32), full["cov"][:cap].view(np.uint32))
    whole = m.extract_shape(moments=True)
    assert np.array_equal(dn[:, :cap].cpu().numpy().T.view(np.uint32), whole["normal"][:cap].view(np.uint32))
    assert np.array_equal(de[:, :cap].cpu().numpy().T.view(np.uint32), whole["evals"][:cap].view(np.uint32))
    got = m.extract_shape(cap_rows=cap, moments=True)                 # the host form, truncated
    want = dict(full, stats=dict(full["stats"], status=full["stats"]["status"] | mm.TRUNCATED))
    for k in ("key", "count", "xyz", "moments", "cov"):
        want[k] = full[k][:cap]
    _same(got, want, "host form, truncated")
    only = m.extract_shape_device(dx.data_ptr(), ld, cap, 1, d_moments_ptr=dm.data_ptr(), shape_ld=sld)      # three of the four columns left out
    assert only == st
    m.close()


# ---- 10. eigenvalues and normals against numpy.linalg.eigh ------------------------------------------------------------------------------------------------------
def test_eigenvalues_and_normals_against_eigh(gpu_ctx):
    """|normal x n_ref| <= 1e-6 where count >= 3 and the gap l1 - l0 >= 1e-3 l2 (float32 rounding of three components sqrt(3) 2^-24 = 1e-7, perturbation
    eps64 l2 / gap <= 2.2e-13; ten times their sum); |evals - l_ref| <= 1e-6 l2 everywhere.  The gap condition may leave out 5 % of the count >= 3 cells at most."""
    from icet_amd import api
    d = _drive()
    scans, poses = d["scans"], d["true"]
    want = sm.ShapeMap(0.5).add(scans, poses).extract_shape(eig=False)
    keep, descs = _descs(scans)
    m = api.VoxelMap(gpu_ctx, cell=0.5, table_log2=LOG2, shape=True)
    m.add_device(descs, poses)
    got = m.extract_shape(moments=True)
    m.close()
    _same(got, want)
    lam, vec = np.linalg.eigh(sm.cov_matrix(want["cov64"]))
    l2 = lam[:, 2]
    ev, nm = got["evals"].astype(np.float64), got["normal"].astype(np.float64)
    assert (np.abs(ev - lam) <= 1e-6 * l2[:, None]).all()
    assert (np.diff(got["evals"], axis=1) >= 0).all()
    assert (np.abs(np.linalg.norm(nm, axis=1) - 1) <= 1e-6).all()
    a = np.abs(got["normal"])
    lead = np.argmax(a, axis=1)                                       # (argmax takes the lowest axis among equals)
    assert (got["normal"][np.arange(a.shape[0]), lead] > 0).all()
    three = want["count"] >= 3
    judged = three & (lam[:, 1] - lam[:, 0] >= 1e-3 * l2)
    print("cells %d, count >= 3: %d, with a gap: %d" % (three.shape[0], three.sum(), judged.sum()))
    assert three.sum() > 500 and judged.sum() >= 0.95 * three.sum()
    cross = np.linalg.norm(np.cross(nm[judged], vec[judged, :, 0]), axis=1)
    print("max |normal x n_ref| %.3e, max |evals - ref| / l2 %.3e" % (cross.max(), (np.abs(ev - lam)[l2 > 0] / l2[l2 > 0, None]).max()))
    assert (cross <= 1e-6).all()
    one = want["count"] == 1
    assert one.any() and not got["evals"][one].any() and (got["normal"][one] == np.array([1, 0, 0], np.float32)).all()


# ---- 11. a full table ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_full_table_drops_whole_runs(gpu_ctx):
    from icet_amd import api
    rs = np.random.RandomState(4)
    i = np.arange(1500)
    base = np.stack([i * 0.125, np.full(1500, 1.0), (i % 7) * 0.125], axis=1)
    rows = np.concatenate([base + rs.rand(1500, 3) * 0.12, base + rs.rand(1500, 3) * 0.12]).astype(np.float32)      # 1500 cells, two rows each, far apart in the scan
    model = sm.ShapeMap(0.125).add([rows], mm.pose()[None])
    assert len(model.cells) == 1500 and model.totals["points_kept"] == 3000
    keep, descs = _descs([rows])
    try:
        for lds in _both_paths(gpu_ctx):
            m = api.VoxelMap(gpu_ctx, cell=0.125, table_log2=10, shape=True)
            m.add_device(descs, mm.pose()[None])
            got = m.extract_shape(moments=True)
            st = got["stats"]
            print("map_lds", lds, st)
            assert st["status"] & api.VOXEL_MAP_TABLE_FULL and st["points_dropped"] > 0
            assert st["points_kept"] + st["points_dropped"] == 3000
            assert int(got["count"].sum()) == st["points_kept"] and st["cells_out"] == got["key"].shape[0] <= 1024
            whole = 0
            for r, (k, c) in enumerate(zip(got["key"], got["count"])):
                assert 1 <= c <= model.cells[int(k)][0]
                if c == model.cells[int(k)][0]:                       # the cell got all of its runs: its words are the model's
                    whole += 1
                    assert [int(v) for v in got["moments"][r]] == model.words(k)
                    assert np.array_equal(got["cov"][r].view(np.uint32), sm.cov(c, model.words(k), 0.125).astype(np.float32).view(np.uint32))
                else:                                                 # one of its two runs was dropped whole: the words are those of one of its rows
                    h = got["moments"][r, :3].astype(np.int64)
                    assert c == 1 and (h < 65536).all() and [int(v) for v in got["moments"][r, 3:]] == [int(h[a] * h[b]) for a, b in sm.PAIRS]
            assert whole > 500
            m.close()
    finally:
        gpu_ctx.set_option("map_lds", 1)
