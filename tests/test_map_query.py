"""The voxel map's query on the GPU (include/icet_hip.h icet_voxel_map_query_*) against the NumPy model of tests/map_query_model.py, BIT FOR
BIT: the rows (float32 as uint32), counts, keys and the three words of every query.  Every output buffer is filled with NaN / 0xFF before a call and what lies
beyond a query's rows must still hold that.  A call's ranges, min_points and flags are ONE record (icet_voxel_map_query), so queries that differ in them are
different calls: the 36 queries of the drive are 12 calls of the three poses."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import map_model as mm
import map_query_model as qm
from icet_amd.api import MAP_QUERY_CHUNK as CHUNK                    # the chunk of the kernels: the one place the sizes below come from

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LOG2 = 16
FILL = np.uint32(0xFFFFFFFF)                                         # as float32: a NaN



def _upload(scan):
    s = np.asarray(scan, np.float32).reshape(-1, 3)
    b = torch.from_numpy(np.ascontiguousarray(s.T) if s.shape[0] else np.zeros((3, 1), np.float32)).to(DEV)
    return b, (b.data_ptr(), s.shape[0], max(s.shape[0], 1))


def _descs(scans):
    bufs = [_upload(s) for s in scans]
    torch.cuda.synchronize(DEV)
    return [b for b, _ in bufs], [d for _, d in bufs]


def _line(n):
    """n one-point cells along x at cell 0.125."""
    i = np.arange(n)
    return np.stack([(i + 0.5) * 0.125, np.full(n, 1.0), (i % 7 + 0.5) * 0.125], axis=1).astype(np.float32)


class Outs:
    """Pre-filled device buffers of a call of Q queries: xyz (3, cap + pad) per query, counts, keys, and the words rows | total | status."""

    def __init__(self, caps, pad=3, null_xyz_at_zero=True):
        self.caps = [int(c) for c in caps]
        self.ld = [c + pad for c in self.caps]
        nan = torch.from_numpy(np.array([FILL], np.uint32).view(np.float32)).to(DEV)
        self.xyz = [nan.repeat(3 * max(l, 1)).reshape(3, max(l, 1)).contiguous() for l in self.ld]
        self.cnt = [torch.full((max(c, 1),), -1, dtype=torch.int64, device=DEV) for c in self.caps]
        self.key = [torch.full((max(c, 1),), -1, dtype=torch.int64, device=DEV) for c in self.caps]
        self.words = torch.full((3, len(self.caps)), -1, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize(DEV)
        self.descs = [((x.data_ptr() if c or not null_xyz_at_zero else None), l, c, n.data_ptr(), k.data_ptr())
                      for c, l, x, n, k in zip(self.caps, self.ld, self.xyz, self.cnt, self.key)]

    def ptrs(self):
        return dict(d_rows_ptr=self.words[0].data_ptr(), d_total_ptr=self.words[1].data_ptr(), d_status_ptr=self.words[2].data_ptr())

    def fetch(self):
        """One dict per query (xyz, count, key, rows, total, status), after checking that nothing beyond the rows was written."""
        torch.cuda.synchronize(DEV)
        w = self.words.cpu().numpy()
        res = []
        for j, c in enumerate(self.caps):
            r = int(w[0, j])
            assert 0 <= r <= c, (j, r, c)
            x = self.xyz[j].cpu().numpy().view(np.uint32); n = self.cnt[j].cpu().numpy(); k = self.key[j].cpu().numpy()
            assert (x[:, r:] == FILL).all() and (n[r:] == -1).all() and (k[r:] == -1).all(), "query %d wrote beyond its %d rows" % (j, r)
            res.append(dict(xyz=np.ascontiguousarray(x[:, :r].T).view(np.float32), count=n[:r].copy(), key=k[:r].view(np.uint64).copy(), rows=r, total=int(w[1, j]),
                            status=int(w[2, j])))
        return res


def _run(vmap, ctx, poses, caps, **kw):
    o = Outs(caps)
    vmap.query_device(poses, o.descs, **o.ptrs(), **kw)
    ctx.sync()
    return o.fetch()


def _same(got, want, what=""):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        tag = (what, j)
        assert (g["total"], g["status"]) == (w["total"], w["status"]), (tag, g["total"], g["status"], w["total"], w["status"])
        assert g["rows"] == w["key"].shape[0], tag
        assert np.array_equal(g["key"], w["key"]), tag
        assert np.array_equal(g["count"], w["count"]), tag
        assert np.array_equal(g["xyz"].view(np.uint32), w["xyz"].view(np.uint32)), tag


def _want(ext, poses, caps, **kw):
    return [qm.query_extract(ext, T, cap_rows=c, **kw) for T, c in zip(np.asarray(poses, np.float32).reshape(-1, 4, 4), caps)]


def _both(ctx):
    """Pruned and unpruned (option "map_query_prune"); the default is restored by the caller's finally."""
    for p in (1, 0):
        ctx.set_option("map_query_prune", p)
        yield p


def _mixed_poses(q, seed=3, spread=6.0):
    rs = np.random.RandomState(seed)
    return np.stack([mm.pose(t=rs.randn(3) * [spread, spread, 0.5], r=rs.randn(3) * [0.4, 0.4, 3.0]) for _ in range(q)])


_CLOUD = {}


def _cloud():
    """A map of ~2700 cells of three random scans (cell 0.1), its model and its extract."""
    if not _CLOUD:
        rs = np.random.RandomState(31)
        scans = [(rs.randn(1500, 3) * [7, 7, 1.0]).astype(np.float32) for _ in range(3)]
        poses = np.stack([mm.pose(t=(k, -0.5 * k, 0.1), r=(0.01, -0.02, 0.4 * k)) for k in range(3)])
        model = mm.Map(0.1).add(scans, poses)
        _CLOUD.update(scans=scans, poses=poses, model=model, ext=model.extract(1))
    return _CLOUD


def _cloud_map(ctx):
    from icet_amd import api
    d = _cloud()
    keep, descs = _descs(d["scans"])
    m = api.VoxelMap(ctx, cell=0.1, table_log2=LOG2)
    m.add_device(descs, d["poses"])
    ctx.sync()
    return m


# ---- 1. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_change_nothing(gpu_ctx):
    from icet_amd import api
    lib = api.load_library()
    d = _cloud()
    m = _cloud_map(gpu_ctx)
    T = _mixed_poses(2)
    n = d["ext"]["key"].shape[0]
    want = _want(d["ext"], T, [n, n], max_range=5.0)
    _same(_run(m, gpu_ctx, T, [n, n], max_range=5.0), want, "before")
    stats = m.stats()
    o = Outs([8, 8])
    good_q = api.MapQuery(0.0, 5.0, 1, 0)
    A = lambda descs: (api.MapSubmap * 2)(*[api.MapSubmap(*x) for x in descs])
    good = A(o.descs)
    rows, total, status = (o.words[k].data_ptr() for k in range(3))
    dT = torch.from_numpy(T.reshape(-1)).to(DEV)
    torch.cuda.synchronize(DEV)
    x0, ld0, c0, n0, k0 = o.descs[0]

    def call(nq=2, poses=T.ctypes.data, q=good_q, outs=good, r=rows, t=total, s=status, posed=False):
        f = lib.icet_voxel_map_query_posed_device if posed else lib.icet_voxel_map_query_device
        return f(m._h, nq, poses, C.byref(q) if q is not None else None, outs, r, t, s)
    Q = api.MapQuery
    bad = [dict(nq=0), dict(nq=-1), dict(nq=257), dict(poses=None), dict(q=None), dict(outs=None), dict(r=None),
           dict(outs=A([(x0, ld0, -1, n0, k0), o.descs[1]])), dict(outs=A([o.descs[0], (x0, c0 - 1, c0, n0, k0)])), dict(outs=A([(None, ld0, c0, n0, k0), o.descs[1]])),
           dict(outs=A([(x0 + 2, ld0, c0, n0, k0), o.descs[1]])), dict(outs=A([(x0, ld0, c0, n0 + 4, k0), o.descs[1]])), dict(outs=A([(x0, ld0, c0, n0, k0 + 4), o.descs[1]])),
           dict(r=rows + 2), dict(t=total + 1), dict(s=status + 2), dict(poses=dT.data_ptr() + 2, posed=True), dict(poses=None, posed=True),
           dict(q=Q(float("nan"), 5.0, 1, 0)), dict(q=Q(0.0, float("inf"), 1, 0)), dict(q=Q(0.0, float("-inf"), 1, 0)), dict(q=Q(0.0, 5.0, 1, 2)), dict(q=Q(0.0, 5.0, 1, -1)),
           dict(q=Q(0.0, 5.0, 1, 0, (C.c_int32 * 4)(0, 0, 0, 1))), dict(q=Q(0.0, 5.0, 1, 0, (C.c_int32 * 4)(7, 0, 0, 0)))]
    for kw in bad:
        assert call(**kw) == api.ICET_ERR_BAD_ARG, kw
        assert lib.icet_voxel_map_last_error(m._h), kw
    assert call() == api.ICET_OK and call(poses=dT.data_ptr(), posed=True) == api.ICET_OK      # (the good call is good)
    gpu_ctx.sync()
    with pytest.raises(api.IcetError):
        gpu_ctx.set_option("map_query_prune_", 1)
    assert m.stats() == stats
    _same(_run(m, gpu_ctx, T, [n, n], max_range=5.0), want, "after")
    m.close()


# ---- 2. the sizes at which the kernels take another path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1])
def test_sizes(gpu_ctx, n):
    from icet_amd import api
    c = CHUNK
    rows = _line(n)
    model = mm.Map(0.125).add([rows], mm.pose()[None])
    ext = model.extract(1)
    assert ext["key"].shape[0] == n
    keep, descs = _descs([rows])
    m = api.VoxelMap(gpu_ctx, cell=0.125, table_log2=LOG2)
    m.add_device(descs, mm.pose()[None])
    far = mm.pose(t=(-1000.0, 1.0, 0.5), r=(0, 0, 0.2))
    cut_wave = 1000.0 + 37.3 * 0.125                                  # a cut inside the first wave's first trip
    cut_chunk = 1000.0 + (c + c // 2 + 100.6) * 0.125                 # a cut inside the second chunk
    cases = [("all", mm.pose(t=(0.01, 0.02, 0.03), r=(0.1, 0.2, 0.3)), dict()), ("none", far, dict(min_range=5000.0)),
             ("left of a cut inside a wave", far, dict(max_range=cut_wave)), ("right of a cut inside a wave", far, dict(min_range=cut_wave)),
             ("left of a cut inside a chunk", far, dict(max_range=cut_chunk)), ("right of a cut inside a chunk", far, dict(min_range=cut_chunk)),
             ("around the middle", mm.pose(t=(n * 0.0625, 1.0, 0.5), r=(0.3, 0, 1.0)), dict(min_range=0.2, max_range=9.0))]
    try:
        for p in _both(gpu_ctx):
            for name, T, kw in cases:
                want = _want(ext, T[None], [n + 1], **kw)
                if name == "all":
                    assert want[0]["total"] == n
                if name == "none":
                    assert want[0]["total"] == 0
                if name == "left of a cut inside a wave":
                    assert want[0]["total"] == min(n, 37)
                if name == "right of a cut inside a chunk" and n > 2 * c:
                    assert 0 < want[0]["total"] < n - c
                _same(_run(m, gpu_ctx, T[None], [n + 1], **kw), want, "%s, prune %d" % (name, p))
            # all of them in one call of seven poses is not possible (one range per call): the three poses at one range are
            T3 = np.stack([cases[0][1], far, cases[6][1]])
            _same(_run(m, gpu_ctx, T3, [n + 1] * 3, max_range=1000.0 + n * 0.0625), _want(ext, T3, [n + 1] * 3, max_range=1000.0 + n * 0.0625), "three poses, prune %d" % p)
    finally:
        gpu_ctx.set_option("map_query_prune", 1)
    m.close()


# ---- 3. the number of queries of a call ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 2, 64, 65, 256])
def test_one_call_of_q_equals_q_calls_of_one(gpu_ctx, q):
    d = _cloud()
    m = _cloud_map(gpu_ctx)
    T = _mixed_poses(q, seed=40 + q)
    n = d["ext"]["key"].shape[0]
    caps = [n] * q
    kw = dict(min_range=0.3, max_range=6.0)
    want = _want(d["ext"], T, caps, **kw)
    assert sum(w["total"] for w in want) > 100 * q
    try:
        for p in _both(gpu_ctx):
            one = _run(m, gpu_ctx, T, caps, **kw)
            _same(one, want, "one call, prune %d" % p)
        singles = [Outs([n]) for _ in range(q)]
        for j, o in enumerate(singles):
            m.query_device(T[j:j + 1], o.descs, **o.ptrs(), **kw)
        gpu_ctx.sync()
        _same([o.fetch()[0] for o in singles], one, "%d calls of one" % q)
    finally:
        gpu_ctx.set_option("map_query_prune", 1)
    m.close()


def test_no_query_and_too_many_are_refused(gpu_ctx):
    from icet_amd import api
    m = _cloud_map(gpu_ctx)
    for q in (0, 257):
        o = Outs([4] * max(q, 1))
        with pytest.raises(api.IcetError) as e:
            m.query_device(np.tile(np.eye(4, dtype=np.float32), (q, 1, 1)), o.descs[:q], **o.ptrs())
        assert e.value.status == api.ICET_ERR_BAD_ARG
        assert (o.words.cpu().numpy() == -1).all()
    m.close()


# ---- 3b. the stages of an add and of a query grow while the previous call is still in flight -----------------------------------------------------------------------
def test_add_stage_grows_while_the_previous_call_is_in_flight(gpu_ctx):
    """Add calls of 1, 5, 2, 33 and 1 scans back to back, host poses and a pose tensor on the device in turn, one synchronisation at the end: the model of all 42."""
    d = _cloud()
    m = _cloud_map(gpu_ctx)
    rs = np.random.RandomState(77)
    scans = [(rs.randn(40 + 7 * k, 3) * [7, 7, 1.0]).astype(np.float32) for k in range(42)]
    poses = _mixed_poses(42, seed=78, spread=2.0)
    want = mm.Map(0.1).add(d["scans"], d["poses"]).add(scans, poses).extract()
    keep, descs = _descs(scans)
    calls, at = [], 0
    for j, n in enumerate((1, 5, 2, 33, 1)):
        T = poses[at:at + n]
        calls.append((descs[at:at + n], torch.from_numpy(T.copy()).to(DEV) if j % 2 else T))
        at += n
    torch.cuda.synchronize(DEV)
    for ds, T in calls:
        m.add_device(ds, T)
    gpu_ctx.sync()
    got = m.extract()
    assert got["stats"] == want["stats"] and got["stats"]["points_in"] == sum(s.shape[0] for s in scans + d["scans"])
    assert np.array_equal(got["key"], want["key"]) and np.array_equal(got["count"], want["count"])
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32))
    m.close()


def test_query_stage_grows_while_the_previous_call_is_in_flight(gpu_ctx):
    """Query calls of 1, 3, 2, 256 and 1 poses back to back, each into its own buffers, host poses and a pose tensor on the device in turn: every call is the model's."""
    d = _cloud()
    m = _cloud_map(gpu_ctx)
    m.index()                                                         # current from here on: the calls below do not synchronise
    n = d["ext"]["key"].shape[0]
    kw = dict(min_range=0.3, max_range=6.0)
    calls = []
    for j, q in enumerate((1, 3, 2, 256, 1)):
        T = _mixed_poses(q, seed=90 + j)
        calls.append((T, torch.from_numpy(T.copy()).to(DEV) if j % 2 else T, Outs([n] * q)))
    torch.cuda.synchronize(DEV)
    for T, given, o in calls:
        m.query_device(given, o.descs, **o.ptrs(), **kw)
    gpu_ctx.sync()
    rows = 0
    for T, given, o in calls:
        want = _want(d["ext"], T, [n] * T.shape[0], **kw)
        rows += sum(w["total"] for w in want)
        _same(o.fetch(), want, "%d poses" % T.shape[0])
    assert rows > 100 * 263
    m.close()


# ---- 4. the drive ------------------------------------------------------------------------------------------------------------------------------------------------
_DRIVE = {}


def _drive():
    """The 8-scan drive of tests/test_map.py, restated: scene 2000, rings 16, steps 256, noise seeds 50 + k, along a line, at the true poses; cell 0.1."""
    if not _DRIVE:
        from icet_amd import lidar_sim
        scene = lidar_sim.make_scene(2000)
        true, scans = [], []
        for k in range(8):
            t = (-5.0 + 1.5 * k, -1.0 + 0.1 * k, 0.0)
            T = mm.pose(t=t, r=(0, 0, 0.05 * k))
            true.append(T)
            s = lidar_sim.make_scan(scene, (np.array(t), T[:3, :3].astype(np.float64)), 50 + k, rings=16, steps=256)
            scans.append(np.ascontiguousarray(s.cpu().numpy().T))
        model = mm.Map(0.1).add(scans, np.stack(true))
        _DRIVE.update(scans=scans, true=np.stack(true), model=model, ext=model.extract(1))
        assert _DRIVE["ext"]["key"].shape[0] == 22121
    return _DRIVE


def _drive_map(ctx):
    from icet_amd import api
    d = _drive()
    keep, descs = _descs(d["scans"])
    m = api.VoxelMap(ctx, cell=0.1, table_log2=LOG2)
    m.add_device(descs, d["true"])
    ctx.sync()
    return m


def test_the_drive(gpu_ctx):
    d = _drive()
    ext = d["ext"]
    T = d["true"][[0, 3, 7]]
    n = ext["key"].shape[0]
    m = _drive_map(gpu_ctx)
    totals = {}
    try:
        for p in _both(gpu_ctx):
            for mp in (1, 2, 3):
                for mx in (2.0, 5.0, 10.0, 0.0):
                    for world in (False, True):
                        kw = dict(min_range=0.5, max_range=mx, min_points=mp, world=world)
                        want = _want(ext, T, [n] * 3, **kw)
                        totals[(mp, mx)] = [w["total"] for w in want]
                        _same(_run(m, gpu_ctx, T, [n] * 3, **kw), want, "min_points %d, max_range %g, world %d, prune %d" % (mp, mx, world, p))
    finally:
        gpu_ctx.set_option("map_query_prune", 1)
    ones = [t for (mp, mx), v in totals.items() if mp == 1 for t in v]
    assert min(ones) == 51 and max(ones) == 22121                     # both ends are covered
    assert totals[(3, 2.0)][:2] == [0, 0] and totals[(3, 2.0)][2] > 0
    m.close()


# ---- 5. truncation -------------------------------------------------------------------------------------------------------------------------------------------------
def test_truncation(gpu_ctx):
    from icet_amd import api
    d = _cloud()
    m = _cloud_map(gpu_ctx)
    T = _mixed_poses(4, seed=5)
    kw = dict(max_range=7.0)
    n = d["ext"]["key"].shape[0]
    full = _want(d["ext"], T, [n] * 4, **kw)
    tot = [w["total"] for w in full]
    assert min(tot) > 300
    try:
        for p in _both(gpu_ctx):
            for caps in ([tot[0] - 1, tot[1], tot[2] + 5, n], [tot[0], 1, tot[2], tot[3]], [0, tot[1], 0, 1], [0, 0, 0, 0]):
                want = _want(d["ext"], T, caps, **kw)
                got = _run(m, gpu_ctx, T, caps, **kw)             # (cap_rows 0: a NULL xyz)
                _same(got, want, "caps %s, prune %d" % (caps, p))
                for j in range(4):
                    assert got[j]["total"] == tot[j]
                    assert bool(got[j]["status"] & api.VOXEL_MAP_TRUNCATED) == (caps[j] < tot[j])
                    assert np.array_equal(got[j]["key"], full[j]["key"][:caps[j]])      # the lowest keys
    finally:
        gpu_ctx.set_option("map_query_prune", 1)
    # the host form sizes its buffers with a count-only call
    res = m.query(T, **kw)
    _same([dict(r, rows=r["key"].shape[0]) for r in res], full, "host form")
    m.close()


# ---- 6. the index follows the map ---------------------------------------------------------------------------------------------------------------------------------
def test_the_index_follows_the_map(gpu_ctx):
    from icet_amd import api
    d = _drive()
    scans, poses = d["scans"], d["true"]
    keep, descs = _descs(scans)
    m = api.VoxelMap(gpu_ctx, cell=0.1, table_log2=LOG2)
    m.add_device(descs[:4], poses[:4])
    T = poses[[1, 5]]
    kw = dict(min_range=0.5, max_range=8.0)
    model = mm.Map(0.1).add(scans[:4], poses[:4])
    e4 = model.extract(1)
    cap = 22121
    before_extract = m.extract()
    first = _run(m, gpu_ctx, T, [cap] * 2, **kw)
    _same(first, _want(e4, T, [cap] * 2, **kw), "four scans")
    assert m.index()["cells_out"] == e4["key"].shape[0]               # (current: nothing to do)
    # add a scan between two queries: the new cells appear; the extract around the query is what it was
    mid_extract = m.extract()
    for k in ("key", "count"):
        assert np.array_equal(before_extract[k], mid_extract[k])
    assert np.array_equal(before_extract["xyz"].view(np.uint32), mid_extract["xyz"].view(np.uint32)) and before_extract["stats"] == mid_extract["stats"]
    m.add_device(descs[5:6], poses[5:6])
    e5 = model.add(scans[5:6], poses[5:6]).extract(1)
    second = _run(m, gpu_ctx, T, [cap] * 2, **kw)
    _same(second, _want(e5, T, [cap] * 2, **kw), "five scans")
    assert second[1]["total"] > first[1]["total"]
    got5 = m.extract()
    assert np.array_equal(got5["key"], e5["key"]) and np.array_equal(got5["xyz"].view(np.uint32), e5["xyz"].view(np.uint32))
    # remove it: the first result, bit for bit, and the emptied cells are absent
    m.remove_device(descs[5:6], poses[5:6])
    third = _run(m, gpu_ctx, T, [cap] * 2, **kw)
    _same(third, first, "removed again")
    gone = set(e5["key"].tolist()) - set(e4["key"].tolist())
    assert gone and not gone & set(_run(m, gpu_ctx, T[:1], [cap], world=True)[0]["key"].tolist())
    after_extract = m.extract()
    assert np.array_equal(before_extract["key"], after_extract["key"]) and np.array_equal(before_extract["xyz"].view(np.uint32), after_extract["xyz"].view(np.uint32))
    # clear: every query has no rows
    m.clear()
    for r in _run(m, gpu_ctx, T, [cap] * 2, **kw):
        assert (r["rows"], r["total"], r["status"]) == (0, 0, 0)
    assert m.index()["cells_out"] == 0
    m.close()


# ---- 7. bad poses --------------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_poses(gpu_ctx):
    from icet_amd import api
    d = _cloud()
    m = _cloud_map(gpu_ctx)
    T = _mixed_poses(5, seed=7)
    T[1, 0, 3] = np.nan                                               # t_0
    T[3, 2, 1] = np.inf                                               # R[2][1]
    T[4, 3, 0] = np.nan                                               # the last row is never read
    n = d["ext"]["key"].shape[0]
    kw = dict(max_range=6.0)
    want = _want(d["ext"], T, [n] * 5, **kw)
    assert [w["status"] for w in want] == [0, api.VOXEL_MAP_QUERY_BAD_POSE, 0, api.VOXEL_MAP_QUERY_BAD_POSE, 0]
    assert all(want[j]["total"] > 100 for j in (0, 2, 4)) and want[1]["total"] == want[3]["total"] == 0
    dT = torch.from_numpy(T.copy()).to(DEV)
    torch.cuda.synchronize(DEV)
    try:
        for p in _both(gpu_ctx):
            _same(_run(m, gpu_ctx, T, [n] * 5, **kw), want, "host poses, prune %d" % p)
            _same(_run(m, gpu_ctx, dT, [n] * 5, **kw), want, "device poses, prune %d" % p)
    finally:
        gpu_ctx.set_option("map_query_prune", 1)
    m.close()


# ---- 8. poses in HBM from the optimiser ---------------------------------------------------------------------------------------------------------------------------
def test_poses_on_the_device_from_the_optimiser(gpu_ctx):
    import pose_graph_cases as pc
    g = pc.graph(6, pc.CASES[3][1], pc.CASES[3][2], True)
    t = [torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(DEV) for k in ("poses", "odo_X", "odo_info")]
    res = gpu_ctx.optimize_pose_graph_device(t[0], t[1], t[2], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL)
    d_poses = res["poses"]
    assert d_poses.is_cuda and tuple(d_poses.shape) == (6, 4, 4)
    h_poses = d_poses.cpu().numpy()
    d = _cloud()
    m = _cloud_map(gpu_ctx)
    n = d["ext"]["key"].shape[0]
    kw = dict(min_range=0.2, max_range=8.0)
    want = _want(d["ext"], h_poses, [n] * 6, **kw)
    assert sum(w["total"] for w in want) > 600
    a = _run(m, gpu_ctx, d_poses, [n] * 6, **kw)
    b = _run(m, gpu_ctx, h_poses, [n] * 6, **kw)
    _same(a, want, "device poses"); _same(b, want, "host poses")
    m.close()


# ---- 9. hand-over to a store with no host round trip ---------------------------------------------------------------------------------------------------------------
def test_sub_maps_into_a_store_with_no_host_round_trip(gpu_ctx):
    import icet_amd
    from icet_amd import api
    d = _drive()
    ext = d["ext"]
    m = _drive_map(gpu_ctx)
    m.index()                                                         # current from here on: the calls below do not synchronise
    T = d["true"][[2, 5]]
    want = _want(ext, T, [None, None])
    store = icet_amd.KeyframeStore(gpu_ctx, 6)
    # what the host does, in order: between a query and its put there is nothing -- no synchronisation, no stats, no index, no copy of a row count
    calls = []
    names = [(api.VoxelMap, "query_device", "query"), (api.KeyframeStore, "put_device", "put"), (api.VoxelMap, "index", "index"), (api.VoxelMap, "stats", "stats"),
             (api.Context, "sync", "sync"), (torch.cuda, "synchronize", "sync"), (torch.Tensor, "cpu", "copy"), (torch.Tensor, "item", "copy")]
    orig = [getattr(o, n) for o, n, _ in names]

    def spy(f, tag):
        def g(*a, **k):
            calls.append(tag)
            return f(*a, **k)
        return g
    try:
        for (o, n, tag), f in zip(names, orig):
            setattr(o, n, spy(f, tag))
        rows0, total0, status0 = store.put_from_map([0], m, T[:1], 0.0, cap_rows=want[0]["total"] + 100)      # cap_rows above the total: the put reads d_rows
        rows1, total1, status1 = store.put_from_map([1], m, T[1:], 0.0, stamps=[11])
    finally:
        for (o, n, _), f in zip(names, orig):
            setattr(o, n, f)
    assert calls.count("query") == 2 and calls.count("put") == 2, calls
    for j, tag in enumerate(calls):
        if tag == "query":
            assert calls[j + 1] == "put", calls
    assert rows1.is_cuda
    gpu_ctx.sync()
    assert (int(rows0[0]), int(total0[0]), int(status0[0])) == (want[0]["total"], want[0]["total"], 0)
    assert (int(rows1[0]), int(total1[0]), int(status1[0])) == (want[1]["total"], want[1]["total"], 0)
    assert np.array_equal(store.debug_fetch(1, "pose"), T[1]) and store.debug_fetch(1, "stamp") == 11
    # the same slots from the model's rows through the host put
    store.put([3, 4], [want[0]["xyz"], want[1]["xyz"]])
    for a, b in ((0, 3), (1, 4)):
        for k in ("hot", "fit", "slot_of_voxel"):
            assert np.array_equal(np.array(store.debug_fetch(a, k)), np.array(store.debug_fetch(b, k))), (a, k)
    # a live scan against such a slot
    live, ld = _descs([d["scans"][5]])
    out = torch.zeros((1, 48), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    store.register_device([1], ld, api.Params(7, 24, 75, 25, 0.1, 0.1, 0), out.data_ptr())
    gpu_ctx.sync()
    X = out.cpu().numpy()[0, :6]
    print("scan 5 against the sub-map around its own pose: X =", X)
    assert np.isfinite(X).all()
    store.close(); m.close()


# ---- 10. interference ----------------------------------------------------------------------------------------------------------------------------------------------
def test_queries_disturb_nothing_else(gpu_ctx, frames, frames_golden):
    import icet_amd
    a, b = frames
    before = gpu_ctx.solve(a, b, 7, np.zeros(6, np.float32), 24, 75)
    assert np.abs(before["X"] - frames_golden["X"]).max() < 3e-4
    store = icet_amd.KeyframeStore(gpu_ctx, 4)
    store.put([2], [a])
    slot_before = {k: np.array(store.debug_fetch(2, k)) for k in ("hot", "fit", "slot_of_voxel")}
    d = _cloud()
    m = _cloud_map(gpu_ctx)
    n = d["ext"]["key"].shape[0]
    T = _mixed_poses(3, seed=9)
    _same(_run(m, gpu_ctx, T, [n] * 3, max_range=6.0), _want(d["ext"], T, [n] * 3, max_range=6.0))
    store.put_from_map([0], m, T[:1], 6.0)
    gpu_ctx.sync()
    after = gpu_ctx.solve(a, b, 7, np.zeros(6, np.float32), 24, 75)
    for k in ("X", "pred_stds", "cov"):
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32))
    for k, v in slot_before.items():
        assert np.array_equal(v, np.array(store.debug_fetch(2, k)))
    store.close(); m.close()
