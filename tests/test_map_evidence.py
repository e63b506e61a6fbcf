"""A voxel map's visibility evidence on the GPU (include/icet_hip.h icet_voxel_map_evidence_*) against the NumPy model of
tests/map_evidence_model.py, BIT FOR BIT: miss, agree and transient per cell of the index, the stats, and the queries with ICET_VOXEL_MAP_QUERY_STATIC.  Every
output buffer is filled with 0xFF before a fetch and what lies beyond the rows must still hold that."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_evidence_cases as cases
import map_evidence_model as em
import map_model as mm
import map_query_model as qm
import test_map_query as tq
from icet_amd.api import MAP_QUERY_CHUNK as CHUNK

pytestmark = pytest.mark.gpu
DEV = tq.DEV
LOG2 = tq.LOG2
KW = dict(max_range=12.0, margin=0.3, min_range=0.5, image_log2=6, window=1, min_miss=2, agree_factor=1)


def _upload_odd(scan, pad=3, shift=1):
    """A scan in a buffer of NaN: columns of ld = n + pad floats from float `shift` on, so that no column is 16-byte aligned and the padding is poison."""
    s = np.asarray(scan, np.float32).reshape(-1, 3)
    n = s.shape[0]; ld = n + pad
    host = np.full(3 * ld + shift + 4, np.nan, np.float32)
    for a in range(3):
        host[shift + a * ld: shift + a * ld + n] = s[:, a]
    b = torch.from_numpy(host).to(DEV)
    return b, (b.data_ptr() + 4 * shift, n, ld)


def _fetch(m, ctx, extra=5):
    """The evidence the map holds, through pre-filled buffers of `extra` entries more than the index has."""
    n = m.index()["cells_out"]
    miss = torch.full((n + extra,), -1, dtype=torch.int32, device=DEV); agree = torch.full((n + extra,), -1, dtype=torch.int32, device=DEV)
    tr = torch.full((n + extra,), 255, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize(DEV)
    rows = m.evidence_fetch_device(n + extra, miss.data_ptr(), agree.data_ptr(), tr.data_ptr())
    ctx.sync()
    assert rows == n
    a, b, c = miss.cpu().numpy(), agree.cpu().numpy(), tr.cpu().numpy()
    assert (a[n:] == -1).all() and (b[n:] == -1).all() and (c[n:] == 255).all(), "the fetch wrote beyond its rows"
    return dict(miss=a[:n], agree=b[:n], transient=c[:n])


def _same_evidence(got, want, what=""):
    for k in ("miss", "agree", "transient"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else got[k].shape)


def _evidence(m, ctx, descs, poses, want, what="", **kw):
    st = m.evidence_device(descs, poses, **kw)
    assert st == want["stats"], (what, st, want["stats"])
    _same_evidence(_fetch(m, ctx), want, what)


def _scans_around(n, rows, seed, spread=6.0):
    rs = np.random.RandomState(seed)
    scans = [(rs.randn(rows, 3) * [6, 6, 1.0]).astype(np.float32) for _ in range(n)]
    return scans, tq._mixed_poses(n, seed=seed + 1, spread=spread)


# ---- 1. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu_ctx):
    from icet_amd import api
    lib = api.load_library()
    d = tq._cloud()
    m = tq._cloud_map(gpu_ctx)
    n = d["ext"]["key"].shape[0]
    T2 = tq._mixed_poses(2)
    stats, ext, q0 = m.stats(), m.extract(), tq._run(m, gpu_ctx, T2, [n, n], max_range=5.0)

    def no_evidence():
        with pytest.raises(api.IcetError) as e:
            tq._run(m, gpu_ctx, T2, [n, n], max_range=5.0, static=True)
        assert e.value.status == api.ICET_ERR_BAD_ARG and "STATIC" in str(e.value)
        with pytest.raises(api.IcetError) as e:
            _fetch(m, gpu_ctx)
        assert e.value.status == api.ICET_ERR_BAD_ARG
    no_evidence()                                                     # before any evidence exists
    keep, descs = tq._descs(d["scans"])
    A = lambda ds: (api.DevScan * len(ds))(*[api.DevScan(*x) for x in ds])
    good_e = api.MapEvidence(0.5, 12.0, 0.3, 6, 1, 2, 1, 0)
    good_s = A(descs)
    dT = torch.from_numpy(d["poses"].reshape(-1).copy()).to(DEV)
    torch.cuda.synchronize(DEV)
    p0, n0, ld0 = descs[0]

    def call(k=3, scans=good_s, poses=d["poses"].ctypes.data, e=good_e, posed=False):
        f = lib.icet_voxel_map_evidence_posed_device if posed else lib.icet_voxel_map_evidence_device
        return f(m._h, k, scans, poses, C.byref(e) if e is not None else None, None)
    E = api.MapEvidence
    bad = [dict(k=-1), dict(e=None), dict(scans=None), dict(poses=None), dict(poses=None, posed=True), dict(poses=dT.data_ptr() + 2, posed=True),
           dict(scans=A([(p0, -1, ld0)] + descs[1:])), dict(scans=A([(p0, n0, n0 - 1)] + descs[1:])), dict(scans=A([(None, n0, ld0)] + descs[1:])),
           dict(scans=A(descs[:2] + [(p0 + 2, n0 - 1, ld0)])),
           dict(e=E(float("nan"), 12.0, 0.3, 6, 1, 2, 1, 0)), dict(e=E(0.5, float("inf"), 0.3, 6, 1, 2, 1, 0)), dict(e=E(0.5, 0.0, 0.3, 6, 1, 2, 1, 0)),
           dict(e=E(0.5, -3.0, 0.3, 6, 1, 2, 1, 0)), dict(e=E(0.5, 12.0, float("nan"), 6, 1, 2, 1, 0)), dict(e=E(0.5, 12.0, -0.1, 6, 1, 2, 1, 0)),
           dict(e=E(0.5, 12.0, 0.3, 3, 1, 2, 1, 0)), dict(e=E(0.5, 12.0, 0.3, 11, 1, 2, 1, 0)), dict(e=E(0.5, 12.0, 0.3, 6, -1, 2, 1, 0)), dict(e=E(0.5, 12.0, 0.3, 6, 3, 2, 1, 0)),
           dict(e=E(0.5, 12.0, 0.3, 6, 1, -1, 1, 0)), dict(e=E(0.5, 12.0, 0.3, 6, 1, 2, -1, 0)), dict(e=E(0.5, 12.0, 0.3, 6, 1, 2, 1, 1)), dict(e=E(0.5, 12.0, 0.3, 6, 1, 2, 1, -1))]
    for kw in bad:
        assert call(**kw) == api.ICET_ERR_BAD_ARG, kw
        assert lib.icet_voxel_map_last_error(m._h), kw
    for name, v in (("map_evidence_batch", 257), ("map_evidence_batch", -1), ("map_evidence_prune_", 1)):
        with pytest.raises(api.IcetError):
            gpu_ctx.set_option(name, v)
    no_evidence()                                                     # a refused call leaves none behind
    after = m.extract()
    assert m.stats() == stats and np.array_equal(after["key"], ext["key"]) and np.array_equal(after["count"], ext["count"])
    assert np.array_equal(after["xyz"].view(np.uint32), ext["xyz"].view(np.uint32))
    tq._same(tq._run(m, gpu_ctx, T2, [n, n], max_range=5.0), q0, "after the refusals")
    # the good call is good, on host and on device poses; then the fetch has its own refusals
    assert call() == api.ICET_OK and call(poses=dT.data_ptr(), posed=True) == api.ICET_OK
    want = em.evidence_extract(d["ext"], d["scans"], d["poses"], **KW)
    _same_evidence(_fetch(m, gpu_ctx), want, "the good call")
    buf = torch.full((n + 4,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize(DEV)
    rows = C.c_int64(-7)
    for args in ((buf.data_ptr(), None, None, n - 1), (buf.data_ptr() + 2, None, None, n), (None, buf.data_ptr() + 1, None, n)):
        assert lib.icet_voxel_map_evidence_fetch_device(m._h, *[C.c_void_p(a) if a else None for a in args[:3]], args[3], C.byref(rows)) == api.ICET_ERR_BAD_ARG, args
    gpu_ctx.sync()
    assert rows.value == -7 and (buf.cpu().numpy() == -1).all()
    assert m.evidence_fetch_device(n) == n                            # all three pointers left out
    static = tq._run(m, gpu_ctx, T2, [n, n], max_range=5.0, static=True)
    tq._same(static, tq._want(em.static_extract(d["ext"], want), T2, [n, n], max_range=5.0), "static")
    # an add makes it stale, together with the index
    more, md = tq._descs([d["scans"][0][:50]])
    m.add_device(md, d["poses"][:1])
    no_evidence()
    m.close()


# ---- 2. the sizes at which the kernels take another path ----------------------------------------------------------------------------------------------------------
def test_scan_rows_at_every_load_path(gpu_ctx):
    d = tq._cloud()
    m = tq._cloud_map(gpu_ctx)
    rs = np.random.RandomState(61)
    T = tq._mixed_poses(2, seed=62, spread=3.0)
    fixed = (rs.randn(300, 3) * [6, 6, 1.0]).astype(np.float32)
    for n in (0, 1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049):
        scan = (rs.randn(n, 3) * [6, 6, 1.0]).astype(np.float32)
        scan[::7, 2] = np.nan                                         # rows that take no part
        for shift, pad in ((1, 3), (0, 0), (2, 1)):
            b0, d0 = _upload_odd(scan, pad, shift); b1, d1 = _upload_odd(fixed, pad, shift + 1)
            torch.cuda.synchronize(DEV)
            want = em.evidence_extract(d["ext"], [scan, fixed], T, **KW)
            _evidence(m, gpu_ctx, [d0, d1], T, want, "rows %d, shift %d" % (n, shift), **KW)
    assert want["stats"]["rows_imaged"] > 1900 and want["miss"].sum() > 100 and want["agree"].sum() > 100
    m.close()


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1])
def test_index_sizes(gpu_ctx, n):
    from icet_amd import api
    rows = tq._line(n)
    model = mm.Map(0.125).add([rows], mm.pose()[None])
    ext = model.extract(1)
    assert ext["key"].shape[0] == n
    keep, descs = tq._descs([rows])
    m = api.VoxelMap(gpu_ctx, cell=0.125, table_log2=LOG2)
    m.add_device(descs, mm.pose()[None])
    # the sensors stand beside the line and see it (agree) or a wall behind it (miss); one stands beyond the line's end, one has a pose that is no rotation
    rs = np.random.RandomState(n)
    L = n * 0.125
    poses = np.stack([mm.pose(t=(x, -2.0, 0.4), r=(0, 0, 0.3 * j)) for j, x in enumerate((3.0, 0.5 * L, L - 1.0, L + 30.0, 0.25 * L))])
    poses[4, :3, :3] *= 0.5
    scans = []
    for T in poses:
        t = T[:3, 3].astype(np.float64)
        k = np.clip(int(t[0] / 0.125) + rs.randint(-64, 64, 400), 0, n - 1)
        world = t + (rows[k].astype(np.float64) - t) * np.where(rs.rand(400, 1) < 0.5, 1.0, 2.0)      # the line itself, or twice as far along the same ray
        scans.append(((world - t) @ T[:3, :3].astype(np.float64)).astype(np.float32))
    kw = dict(max_range=15.0, margin=0.3, min_range=0.5, image_log2=7, window=1, min_miss=1, agree_factor=1)
    want = em.evidence_extract(ext, scans, poses, **kw)
    assert want["miss"].sum() > 20 and want["agree"].sum() > 200 and 0 < want["stats"]["cells_transient"] < n
    keep2, sd = tq._descs(scans)
    try:
        for prune in (1, 0):
            gpu_ctx.set_option("map_evidence_prune", prune)
            _evidence(m, gpu_ctx, sd, poses, want, "prune %d" % prune, **kw)
    finally:
        gpu_ctx.set_option("map_evidence_prune", 1)
    # the last cell of the last chunk is one a query can drop
    st = tq._run(m, gpu_ctx, mm.pose()[None], [n], world=True, static=True)
    tq._same(st, tq._want(em.static_extract(ext, want), mm.pose()[None], [n], world=True), "static, everything")
    m.close()


def test_scan_counts_image_sizes_and_windows(gpu_ctx):
    d = tq._cloud()
    m = tq._cloud_map(gpu_ctx)
    scans, poses = _scans_around(65, 60, 71)
    keep, descs = tq._descs(scans)
    base = dict(max_range=12.0, margin=0.3, min_range=0.5, min_miss=2, agree_factor=1)
    try:
        for k, log2, window, batch in ((0, 6, 1, 0), (1, 4, 0, 0), (65, 4, 1, 0), (65, 4, 2, 64), (65, 5, 0, 0), (9, 10, 2, 0), (9, 10, 1, 0), (1, 10, 0, 0)):
            gpu_ctx.set_option("map_evidence_batch", batch)
            kw = dict(base, image_log2=log2, window=window)
            want = em.evidence_extract(d["ext"], scans[:k], poses[:k], **kw)
            _evidence(m, gpu_ctx, descs[:k], poses[:k], want, "%d scans, W %d, window %d" % (k, 1 << log2, window), **kw)
            assert want["stats"]["scans_used"] == k and (k > 0 or want["miss"].sum() + want["agree"].sum() == 0)
    finally:
        gpu_ctx.set_option("map_evidence_batch", 0)
    m.close()


# ---- 3. the tables of the CPU tests through the device ------------------------------------------------------------------------------------------------------------
def test_the_direction_table_as_scans_of_one_row(gpu_ctx):
    from icet_amd import api
    table = cases.direction_rows()
    unit = table.astype(np.float64) / np.abs(table.astype(np.float64)).max(axis=1)[:, None]
    cells = (unit / np.linalg.norm(unit, axis=1)[:, None] * 5.0).astype(np.float32)      # one cell 5 m out in every direction of the table
    model = mm.Map(0.1).add([cells], mm.pose()[None])
    ext = model.extract(1)
    keep, cd = tq._descs([cells])
    m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2)
    m.add_device(cd, mm.pose()[None])
    # a scan of one row each: the table's own rows (magnitudes 1e-30 .. 3e38), and every direction again at the cell's range (agree) and at twice that (miss)
    scans = [r[None, :] for r in table] + [c[None, :] for c in cells] + [(c * np.float32(2.0))[None, :] for c in cells]
    poses = np.tile(mm.pose()[None], (len(scans), 1, 1))
    keep2, sd = tq._descs(scans)
    for log2, window in ((4, 0), (4, 1), (5, 2), (8, 0)):
        kw = dict(max_range=40.0, margin=0.3, min_range=0.0, image_log2=log2, window=window, min_miss=1, agree_factor=0)
        want = em.evidence_extract(ext, scans, poses, **kw)
        _evidence(m, gpu_ctx, sd, poses, want, "W %d, window %d" % (1 << log2, window), **kw)
        assert want["stats"]["rows_imaged"] == len(scans) and want["miss"].sum() > 40 and want["agree"].sum() > 40
    m.close()


def test_the_tie_table_as_hand_made_cells(gpu_ctx):
    from icet_amd import api
    pt, table = cases.tie_cases()
    keep, pd = tq._descs([pt])
    m = api.VoxelMap(gpu_ctx, cell=0.125, table_log2=LOG2)
    m.add_device(pd, mm.pose()[None])
    ext = mm.Map(0.125).add([pt], mm.pose()[None]).extract(1)
    got_ext = m.extract()
    assert got_ext["xyz"].view(np.uint32).tolist() == pt.view(np.uint32).tolist()      # one point per cell: the centroid is the point
    for c in table:
        row = np.array([c["scan_row"]], np.float32)
        keep2, sd = tq._descs([row])
        kw = dict(max_range=c["mx"], margin=c["mg"], min_range=c["mn"], image_log2=8, window=0, min_miss=1, agree_factor=0)
        want = em.evidence_extract(ext, [row], mm.pose()[None], **kw)
        _evidence(m, gpu_ctx, sd, mm.pose()[None], want, str(c), **kw)
        got = _fetch(m, gpu_ctx)
        assert ("miss" if got["miss"][0] else ("agree" if got["agree"][0] else "none")) == c["want"], c
        assert got["transient"][0] == (c["want"] == "miss")
    m.close()


def test_one_pixel_hit_by_every_lane_of_a_block(gpu_ctx):
    from icet_amd import api
    rs = np.random.RandomState(81)
    r = (5.0 + rs.permutation(2 * 2048 + 5) * 1e-3).astype(np.float32)      # three blocks of rows along +x: one pixel, its minimum 5.0
    scan = np.stack([r, np.zeros_like(r), np.zeros_like(r)], axis=1)
    cells = np.array([[2.05, 0, 0], [3.05, 0, 0], [4.95, 0, 0], [5.05, 0, 0], [6.05, 0, 0], [7.05, 0, 0], [0, 3.05, 0]], np.float32)
    ext = mm.Map(0.1).add([cells], mm.pose()[None]).extract(1)
    keep, cd = tq._descs([cells]); keep2, sd = tq._descs([scan])
    m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2)
    m.add_device(cd, mm.pose()[None])
    kw = dict(max_range=40.0, margin=0.25, min_range=0.0, image_log2=8, window=0, min_miss=1, agree_factor=0)
    want = em.evidence_extract(ext, [scan], mm.pose()[None], **kw)
    assert want["miss"].sum() == 2 and want["agree"].sum() == 2 and want["stats"]["rows_imaged"] == r.shape[0]
    _evidence(m, gpu_ctx, sd, mm.pose()[None], want, **kw)
    # the host form, with its keys; and its default margin of three cells
    for host, w in ((m.evidence([scan], mm.pose()[None], **kw), want), (m.evidence([scan], mm.pose()[None], 40.0), em.evidence(mm.Map(0.1).add([cells], mm.pose()[None]), [scan], mm.pose()[None], 40.0))):
        _same_evidence(host, w, "host form")
        assert host["stats"] == w["stats"] and host["key"].dtype == np.uint64 and np.array_equal(host["key"], w["key"])
    m.close()


# ---- 4. launch shape -------------------------------------------------------------------------------------------------------------------------------------------
def test_launch_shape_changes_no_bit(gpu_ctx):
    d = tq._cloud()
    m = tq._cloud_map(gpu_ctx)
    scans, poses = _scans_around(7, 500, 91, spread=9.0)
    poses[2, 0, 3] = 15.0; poses[5, 0, 3] = -17.0                     # far out on x: most chunks of the index are out of their reach
    poses[3, :3, :3] *= 0.5                                           # no rotation: never pruned
    poses[6, 1, 1] = np.nan                                           # unusable
    keep, descs = tq._descs(scans)
    kw = dict(KW, max_range=6.0)
    want = em.evidence_extract(d["ext"], scans, poses, **kw)
    assert want["stats"]["scans_bad_pose"] == 1 and want["miss"].sum() > 100 and want["agree"].sum() > 200 and want["stats"]["cells_transient"] > 5
    try:
        for batch in (1, 3, 0):
            for prune in (1, 0):
                gpu_ctx.set_option("map_evidence_batch", batch); gpu_ctx.set_option("map_evidence_prune", prune)
                _evidence(m, gpu_ctx, descs, poses, want, "batch %d, prune %d" % (batch, prune), **kw)
        rev = em.evidence_extract(d["ext"], scans[::-1], poses[::-1], **kw)
        _same_evidence(rev, want, "the model, reversed")
        _evidence(m, gpu_ctx, descs[::-1], np.ascontiguousarray(poses[::-1]), want, "reversed", **kw)
        # two calls are two evidences, not a sum: the second replaces the first
        _evidence(m, gpu_ctx, descs[:2], poses[:2], em.evidence_extract(d["ext"], scans[:2], poses[:2], **kw), "two scans", **kw)
    finally:
        gpu_ctx.set_option("map_evidence_batch", 0); gpu_ctx.set_option("map_evidence_prune", 1)
    m.close()


# ---- 5. the drive with the car ------------------------------------------------------------------------------------------------------------------------------------
DRIVE_KW = dict(max_range=40.0, margin=0.3, min_range=0.0, image_log2=7, window=1, min_miss=2, agree_factor=1)


def _car_map(ctx, poses=None):
    from icet_amd import api
    d = cases.car_drive(16, 256)
    keep, descs = tq._descs(d["scans"])
    m = api.VoxelMap(ctx, cell=0.1, table_log2=LOG2)
    m.add_device(descs, d["poses"] if poses is None else poses)
    ctx.sync()
    return m, keep, descs


def test_the_drive_with_the_car(gpu_ctx):
    d = cases.car_drive(16, 256)
    ext = d["ext"]
    n = ext["key"].shape[0]
    assert 20000 < n < 25000
    m, keep, descs = _car_map(gpu_ctx)
    want = em.evidence_extract(ext, d["scans"], d["poses"], **DRIVE_KW)
    movers = cases.mover_cells(ext["xyz"], d["boxes"], d["ground"])
    print("cells %d, movers %d, transient %d, of them movers %d" % (n, movers.sum(), want["stats"]["cells_transient"], (movers & (want["transient"] > 0)).sum()))
    assert want["stats"]["cells_transient"] > 20
    _evidence(m, gpu_ctx, descs, d["poses"], want, "the drive", **DRIVE_KW)
    host = m.evidence_fetch()
    _same_evidence(host, want, "host fetch")
    assert np.array_equal(host["key"], ext["key"])
    still = em.static_extract(ext, want)
    everything = mm.pose(t=(0.03, 0.02, 0.01))[None]
    tq._same(tq._run(m, gpu_ctx, everything, [n], world=True, static=True), tq._want(still, everything, [n], world=True), "world, static")
    assert still["key"].shape[0] == n - want["stats"]["cells_transient"]
    T = d["poses"][[0, 3, 7]]
    for kw in (dict(min_range=0.5, max_range=10.0), dict(min_range=0.0, max_range=0.0, min_points=2)):
        tq._same(tq._run(m, gpu_ctx, T, [n] * 3, static=True, **kw), tq._want(still, T, [n] * 3, **kw), "posed, static")
        tq._same(tq._run(m, gpu_ctx, T, [n] * 3, **kw), tq._want(ext, T, [n] * 3, **kw), "posed, all cells")
    plain = tq._run(m, gpu_ctx, everything, [n], world=True)[0]
    got = m.extract()
    assert np.array_equal(plain["key"], got["key"]) and np.array_equal(plain["count"], got["count"]) and np.array_equal(plain["xyz"].view(np.uint32), got["xyz"].view(np.uint32))
    assert np.array_equal(got["xyz"].view(np.uint32), ext["xyz"].view(np.uint32))
    m.close()


# ---- 6. re-pose equals rebuild --------------------------------------------------------------------------------------------------------------------------------------
def test_a_re_pose_equals_a_rebuild(gpu_ctx):
    d = cases.car_drive(16, 256)
    true = d["poses"]
    drift = true.copy()
    for k in (2, 4, 6):
        drift[k] = mm.pose(t=(-5.0 + 1.5 * k + 0.3, -1.0 + 0.1 * k - 0.2, 0.05), r=(0, 0.01, 0.05 * k + 0.02))
    m, keep, descs = _car_map(gpu_ctx, drift)
    drifted_model = mm.Map(0.1).add(d["scans"], drift)
    _evidence(m, gpu_ctx, descs, drift, em.evidence_extract(drifted_model.extract(1), d["scans"], drift, **DRIVE_KW), "drifted", **DRIVE_KW)
    three = [descs[k] for k in (2, 4, 6)]
    m.remove_device(three, drift[[2, 4, 6]])
    m.add_device(three, true[[2, 4, 6]])
    st = m.evidence_device(descs, true, **DRIVE_KW)
    moved = _fetch(m, gpu_ctx)
    fresh, keep2, descs2 = _car_map(gpu_ctx)
    st2 = fresh.evidence_device(descs2, true, **DRIVE_KW)
    rebuilt = _fetch(fresh, gpu_ctx)
    assert st == st2
    _same_evidence(moved, rebuilt, "re-posed against rebuilt")
    want = em.evidence_extract(d["ext"], d["scans"], true, **DRIVE_KW)
    _same_evidence(moved, want, "re-posed against the model")
    assert st == want["stats"] and np.array_equal(m.evidence_fetch()["key"], d["ext"]["key"])
    m.close(); fresh.close()


# ---- 7. poses in HBM from the optimiser ---------------------------------------------------------------------------------------------------------------------------
def test_poses_on_the_device_from_the_optimiser(gpu_ctx):
    import pose_graph_cases as pc
    g = pc.graph(6, pc.CASES[3][1], pc.CASES[3][2], True)
    t = [torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(DEV) for k in ("poses", "odo_X", "odo_info")]
    res = gpu_ctx.optimize_pose_graph_device(t[0], t[1], t[2], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL)
    d_poses = res["poses"]
    assert d_poses.is_cuda and tuple(d_poses.shape) == (6, 4, 4)
    h_poses = d_poses.cpu().numpy()
    d = tq._cloud()
    m = tq._cloud_map(gpu_ctx)
    scans, _ = _scans_around(6, 400, 95)
    keep, descs = tq._descs(scans)
    want = em.evidence_extract(d["ext"], scans, h_poses, **KW)
    assert want["miss"].sum() > 50 and want["agree"].sum() > 100
    _evidence(m, gpu_ctx, descs, d_poses, want, "device poses", **KW)
    _evidence(m, gpu_ctx, descs, h_poses, want, "host poses", **KW)
    bad = d_poses.clone(); bad[2, 0, 3] = float("nan")
    torch.cuda.synchronize(DEV)
    hb = h_poses.copy(); hb[2, 0, 3] = np.nan
    want_bad = em.evidence_extract(d["ext"], scans, hb, **KW)
    assert want_bad["stats"]["scans_bad_pose"] == 1 and want_bad["stats"]["scans_used"] == 5
    _same_evidence(want_bad, em.evidence_extract(d["ext"], scans[:2] + scans[3:], np.delete(h_poses, 2, axis=0), **KW), "no evidence from that scan")
    _evidence(m, gpu_ctx, descs, bad, want_bad, "a NaN in a device pose", **KW)
    m.close()


# ---- 8. hand-over to a store without the movers -----------------------------------------------------------------------------------------------------------------
def test_put_from_map_static(gpu_ctx):
    import icet_amd
    from icet_amd import api
    d = cases.car_drive(16, 256)
    m, keep, descs = _car_map(gpu_ctx)
    want = em.evidence_extract(d["ext"], d["scans"], d["poses"], **DRIVE_KW)
    m.evidence_device(descs, d["poses"], **DRIVE_KW)
    T = d["poses"][5:6]
    all_rows = tq._want(d["ext"], T, [None])[0]["total"]
    still_rows = tq._want(em.static_extract(d["ext"], want), T, [None])[0]["total"]
    assert 0 < all_rows - still_rows <= want["stats"]["cells_transient"]
    store = icet_amd.KeyframeStore(gpu_ctx, 4)
    r0, t0, s0 = store.put_from_map([0], m, T, 0.0, static=False)
    r1, t1, s1 = store.put_from_map([1], m, T, 0.0, static=True)
    gpu_ctx.sync()
    assert (int(r0[0]), int(t0[0]), int(s0[0])) == (all_rows, all_rows, 0)
    assert (int(r1[0]), int(t1[0]), int(s1[0])) == (still_rows, still_rows, 0)
    live, ld = tq._descs([d["scans"][5]])
    out = torch.zeros((1, 48), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    store.register_device([1], ld, api.Params(7, 24, 75, 25, 0.1, 0.1, 0), out.data_ptr())
    gpu_ctx.sync()
    X = out.cpu().numpy()[0, :6]
    print("scan 5 against the static sub-map around its own pose: X =", X)
    assert np.isfinite(X).all()
    store.close(); m.close()


# ---- 9. interference ----------------------------------------------------------------------------------------------------------------------------------------------
def test_evidence_disturbs_nothing_else(gpu_ctx, frames, frames_golden):
    import icet_amd
    a, b = frames
    before = gpu_ctx.solve(a, b, 7, np.zeros(6, np.float32), 24, 75)
    assert np.abs(before["X"] - frames_golden["X"]).max() < 3e-4
    store = icet_amd.KeyframeStore(gpu_ctx, 4)
    store.put([2], [a])
    slot_before = {k: np.array(store.debug_fetch(2, k)) for k in ("hot", "fit", "slot_of_voxel")}
    d = tq._cloud()
    m = tq._cloud_map(gpu_ctx)
    ext_before = m.extract()
    keep, descs = tq._descs(d["scans"])
    _evidence(m, gpu_ctx, descs, d["poses"], em.evidence_extract(d["ext"], d["scans"], d["poses"], **KW), **KW)
    after = gpu_ctx.solve(a, b, 7, np.zeros(6, np.float32), 24, 75)
    for k in ("X", "pred_stds", "cov"):
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32))
    for k, v in slot_before.items():
        assert np.array_equal(v, np.array(store.debug_fetch(2, k)))
    ext_after = m.extract()
    assert ext_after["stats"] == ext_before["stats"] and np.array_equal(ext_after["key"], ext_before["key"]) and np.array_equal(ext_after["count"], ext_before["count"])
    assert np.array_equal(ext_after["xyz"].view(np.uint32), ext_before["xyz"].view(np.uint32))
    _same_evidence(_fetch(m, gpu_ctx), em.evidence_extract(d["ext"], d["scans"], d["poses"], **KW), "an extract leaves the evidence current")
    store.close(); m.close()
