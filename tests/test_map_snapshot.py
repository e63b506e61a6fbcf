"""The voxel map saved, loaded and merged on the GPU (include/icet_hip.h icet_voxel_map_save / _load / _snapshot_info / _merge_device)
against the NumPy model of tests/map_snapshot_model.py: a saved file equals the model's BYTE FOR BYTE, a loaded map gives the same stats, the same extract and the
same file again, the file is a function of the map's contents alone, maps are additive file by file and table by table, and every refusal touches nothing.  Every
comparison is bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

import map_model as mm
import map_register_cases as cs
import map_shape_model as shm
import map_snapshot_model as msm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
COUNTS = (0, 1, 2, 255, 256, 257, 4095, 4096, 4097)                   # around the odd / even padding, a block, and the 4096-entry span of a table pass
POOL_CELL = 0.1


@pytest.fixture(scope="module")
def ctx2():
    import icet_amd
    c = icet_amd.Context(0)
    yield c
    c.close()


def _new(ctx, ref, log2, shaped):
    from icet_amd import api
    return api.VoxelMap(ctx, cell=ref.cell, min_range=ref.min_range, max_range=ref.max_range, table_log2=log2, shape=shaped)


def _file(m, path):
    m.save(str(path))
    return open(str(path), "rb").read()


def _extract(m):
    return m.extract_shape(moments=True) if m.shape else m.extract()


def _same_extract(a, b, what=""):
    assert a["stats"] == b["stats"], (what, a["stats"], b["stats"])
    for k in a:
        if k != "stats":
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


@functools.lru_cache(maxsize=None)
def _pool():
    """Rows of two lidar_sim scans (rings=16, steps=512) and, per row, its cell's rank by first appearance: the rows of rank < n fill exactly n cells."""
    rows = np.concatenate(cs.scene()["scans"][:2])
    cls, key, _, _ = mm.classify(rows, mm.pose(), POOL_CELL)
    rows, key = rows[cls == mm.KEPT], key[cls == mm.KEPT]
    uk, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(uk.shape[0], np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(uk.shape[0])
    assert uk.shape[0] > max(COUNTS)
    return rows, rank[inv]


@functools.lru_cache(maxsize=None)
def _count_case(n):
    rows, rank = _pool()
    scan = np.ascontiguousarray(rows[rank < n])
    model = shm.ShapeMap(POOL_CELL)
    if n:
        model.add([scan], [mm.pose()])
    assert len(model.cells) == n
    return scan, model


def _round_trip(gpu_ctx, ctx2, tmp_path, m, model, shaped):
    """m holds the model's contents: its file is the model's, and every map loaded from it is m again."""
    from icet_amd import api
    want = msm.write(model, shaped)
    raw = _file(m, tmp_path / "a.vxm")
    assert raw == want
    info = api.VoxelMap.snapshot_info(str(tmp_path / "a.vxm"))
    n = msm.read(want)["keys"].shape[0]
    assert info["payload_checksum"] == msm.checksum(want[128:]) and info["entries"] == n and info["shaped"] == shaped and info["file_bytes"] == len(want)
    ref, stats = _extract(m), m.stats()
    assert {k: stats[k] for k in msm.TOTALS} == model.totals
    for ctx in (gpu_ctx, ctx2):
        for log2 in (10, 12, 22):
            fresh = _new(ctx, model, log2, shaped)
            if n > (1 << log2):                                       # (the capacity bound: refused, nothing touched)
                with pytest.raises(api.IcetError):
                    fresh.load(str(tmp_path / "a.vxm"))
                assert len(_file(fresh, tmp_path / "b.vxm")) == 128
            else:
                fresh.load(str(tmp_path / "a.vxm"))
                assert fresh.stats() == stats, log2
                _same_extract(_extract(fresh), ref, log2)
                assert _file(fresh, tmp_path / "b.vxm") == want, log2
            fresh.close()
    built = api.VoxelMap.from_file(ctx2, str(tmp_path / "a.vxm"))
    assert built.shape == shaped and built.params.table_log2 == max(10, (2 * max(n, 1) - 1).bit_length()) and _file(built, tmp_path / "b.vxm") == want
    built.close()


@pytest.mark.parametrize("shaped", [False, True])
@pytest.mark.parametrize("n", COUNTS)
def test_round_trip_at_every_entry_count(gpu_ctx, ctx2, tmp_path, n, shaped):
    scan, model = _count_case(n)
    m = _new(gpu_ctx, model, 14, shaped)
    if n:
        m.add([scan], [mm.pose()])
    _round_trip(gpu_ctx, ctx2, tmp_path, m, model, shaped)
    m.close()


@pytest.mark.parametrize("shaped", [False, True])
@pytest.mark.parametrize("source", ["edge", "range"])
def test_round_trip_of_the_rule_s_edge_rows(gpu_ctx, ctx2, tmp_path, source, shaped):
    if source == "edge":
        model = shm.ShapeMap(0.125)
        scans = [r for r, _, _ in mm.edge_rows(0.125)]; poses = [T for _, T, _ in mm.edge_rows(0.125)]
    else:
        model = shm.ShapeMap(0.1, min_range=5.0, max_range=13.0)
        scans, poses = [mm.range_rows()[0]], [mm.pose()]
    model.add(scans, poses)
    m = _new(gpu_ctx, model, 10, shaped)
    m.add(scans, np.asarray(poses, np.float32))
    if source == "edge":
        assert model.totals["points_outside"] > 0 and model.totals["points_nonfinite"] > 0 and len(model.cells) > 10
    _round_trip(gpu_ctx, ctx2, tmp_path, m, model, shaped)
    m.close()


def test_the_file_is_a_function_of_the_contents(gpu_ctx, tmp_path):
    from icet_amd import api
    s = cs.scene()
    scans, poses = s["scans"], np.asarray(s["poses"], np.float32)
    want = msm.write(s["map"])
    files = {}
    try:
        for lds in (1, 0):
            gpu_ctx.set_option("map_lds", lds)
            for name, log2 in (("one call", 16), ("eight calls", 16), ("reversed", 16), ("another table", 18)):
                m = api.VoxelMap(gpu_ctx, cell=s["cell"], table_log2=log2, shape=True)
                if name == "eight calls":
                    for k in range(8):
                        m.add(scans[k:k + 1], poses[k:k + 1])
                elif name == "reversed":
                    m.add(scans[::-1], poses[::-1])
                else:
                    m.add(scans, poses)
                files[(lds, name)] = _file(m, tmp_path / "f.vxm")
                if (lds, name) == (1, "one call"):
                    for chunk in (1, 1000, 0):
                        gpu_ctx.set_option("map_snapshot_chunk_entries", chunk)
                        files[("chunk", chunk)] = _file(m, tmp_path / "c.vxm")
                        fresh = api.VoxelMap(gpu_ctx, cell=s["cell"], table_log2=15 + (chunk == 0), shape=True)
                        fresh.load(str(tmp_path / "c.vxm"))          # (the load moves in the same chunks)
                        _same_extract(_extract(fresh), _extract(m), chunk)
                        fresh.close()
                m.close()
    finally:
        gpu_ctx.set_option("map_lds", 1); gpu_ctx.set_option("map_snapshot_chunk_entries", 0)
    assert len(files) == 11 and msm.read(want)["keys"].shape[0] > 4096
    for k, raw in files.items():
        assert raw == want, k
    with pytest.raises(api.IcetError):
        gpu_ctx.set_option("map_snapshot_chunk_entries", -1)


def _staged(scans):
    bufs = [torch.from_numpy(np.ascontiguousarray(np.asarray(s, np.float32).T)).to(DEV) for s in scans]
    torch.cuda.synchronize(DEV)
    return bufs, [(b.data_ptr(), b.shape[1], b.shape[1]) for b in bufs]


def _answers(ctx, m, s):
    """What a map answers: the records of a scored and of a registered pose per start, a query of everything, and the slot a store builds from it."""
    import icet_amd
    keep, descs = _staged([s["held"][i][0] for i, _ in s["starts"]])
    T0 = np.stack([T for _, T in s["starts"]])
    out = dict(score=m.register_records(descs, T0, max_iters=0).tobytes(), reg=m.register_records(descs, T0, max_iters=20).tobytes())
    q = m.query(np.asarray(mm.pose(), np.float32).reshape(1, 4, 4), world=True)[0]
    out.update(q_xyz=q["xyz"].tobytes(), q_count=q["count"].tobytes(), q_key=q["key"].tobytes(), q_total=q["total"])
    store = icet_amd.KeyframeStore(ctx, 2)
    store.put_from_map([0], m, np.asarray(s["poses"][3], np.float32).reshape(1, 4, 4), 30.0)
    ctx.sync()
    for k in ("hot", "fit", "slot_of_voxel"):
        out["slot_" + k] = np.array(store.debug_fetch(0, k)).tobytes()
    store.close()
    return out


def test_maps_are_additive_through_files_and_through_merge(gpu_ctx, tmp_path):
    from icet_amd import api
    s = cs.scene()
    scans, poses = s["scans"], np.asarray(s["poses"], np.float32)
    new = lambda log2=16: api.VoxelMap(gpu_ctx, cell=s["cell"], table_log2=log2, shape=True)
    A, B, whole = new(), new(15), new()
    A.add(scans[:4], poses[:4]); B.add(scans[4:], poses[4:]); whole.add(scans, poses)
    fa, fb, fw = _file(A, tmp_path / "a.vxm"), _file(B, tmp_path / "b.vxm"), _file(whole, tmp_path / "w.vxm")
    assert fw == msm.write(s["map"]) and fa == msm.write(shm.ShapeMap(s["cell"]).add(scans[:4], poses[:4]))
    # through the files
    Cm = new(17)
    Cm.load(str(tmp_path / "a.vxm")); Cm.load(str(tmp_path / "b.vxm"))
    assert _file(Cm, tmp_path / "c.vxm") == fw and Cm.stats() == whole.stats()
    want = _answers(gpu_ctx, whole, s)
    assert _answers(gpu_ctx, Cm, s) == want
    assert msm.read(fa)["keys"].shape[0] > 1000 and len(want["q_key"]) > 8000
    # through the tables
    D = new(14)
    D.merge(A); D.merge(B)
    assert _file(D, tmp_path / "d.vxm") == fw and D.stats() == whole.stats()
    assert _answers(gpu_ctx, D, s) == want
    assert _file(A, tmp_path / "a2.vxm") == fa and _file(B, tmp_path / "b2.vxm") == fb      # the sources were only read
    # B taken out again: A's file, totals in the header included; B's own cells stay claimed in the table and nothing of them shows
    Cm.load(str(tmp_path / "b.vxm"), -1)
    assert _file(Cm, tmp_path / "c.vxm") == fa and Cm.stats() == A.stats()
    D.merge(B, -1)
    assert _file(D, tmp_path / "d.vxm") == fa
    assert np.setdiff1d(msm.read(fb)["keys"], msm.read(fa)["keys"]).shape[0] > 100      # (B has cells of its own; that they stay claimed: the capacity test)
    _same_extract(_extract(Cm), _extract(A)); _same_extract(_extract(D), _extract(A))
    for m in (A, B, whole, Cm, D):
        m.close()


def test_capacity_is_checked_before_anything_is_touched_and_grown_answers_a_full_table(gpu_ctx, tmp_path):
    from icet_amd import api
    scan, model = _count_case(4097)
    rows, rank = _pool()
    pick = lambda lo, hi: np.ascontiguousarray(rows[(rank >= lo) & (rank < hi)])
    cells1000, same100, other100 = pick(0, 1000), pick(0, 100), pick(2000, 2100)
    model1000 = shm.ShapeMap(POOL_CELL).add([cells1000], [mm.pose()])
    for shaped in (False, True):
        full = _new(gpu_ctx, model, 10, shaped)
        full.add([cells1000], [mm.pose()])
        st = full.stats()
        assert st["cells_occupied"] == 1000 and st["points_dropped"] == 0
        f1000 = _file(full, tmp_path / "k.vxm")
        assert f1000 == msm.write(model1000, shaped)
        big = full.grown(11)
        assert big.params.table_log2 == 11 and big.shape == shaped and big.stats() == st
        _same_extract(_extract(big), _extract(full))
        assert _file(big, tmp_path / "g.vxm") == f1000
        # 100 OTHER cells + 1000 new keys > 1024: refused, the map's save unchanged
        other = _new(gpu_ctx, model, 10, shaped)
        other.add([other100], [mm.pose()])
        before = _file(other, tmp_path / "o.vxm")
        with pytest.raises(api.IcetError) as e:
            other.load(str(tmp_path / "k.vxm"))
        assert e.value.status == api.ICET_ERR_BAD_ARG and "too small" in str(e.value)
        with pytest.raises(api.IcetError):
            other.merge(full)
        assert _file(other, tmp_path / "o2.vxm") == before
        # 100 of the SAME cells: the dry run counts only new keys, 900 + 100 <= 1024
        same = _new(gpu_ctx, model, 10, shaped)
        same.add([same100], [mm.pose()])
        same.load(str(tmp_path / "k.vxm"))
        both = shm.ShapeMap(POOL_CELL).add([cells1000, same100], [mm.pose(), mm.pose()])
        assert _file(same, tmp_path / "s.vxm") == msm.write(both, shaped) and same.stats()["cells_occupied"] == 1000
        # a table that is exactly full still takes what it already holds
        exact = _new(gpu_ctx, model, 10, shaped)
        exact.add([pick(0, 1024)], [mm.pose()])
        assert exact.stats()["cells_occupied"] == 1024
        exact.load(str(tmp_path / "k.vxm"))
        assert exact.stats()["cells_occupied"] == 1024 and exact.stats()["points_dropped"] == 0
        # emptied keys stay claimed: 600 + 424 cells in, the 424 out again -- the file shows 600 cells, the table still has no free entry, a grown copy has
        lo, hi = _new(gpu_ctx, model, 10, shaped), _new(gpu_ctx, model, 10, shaped)
        lo.add([pick(0, 600)], [mm.pose()]); hi.add([pick(600, 1024)], [mm.pose()])
        f600 = _file(lo, tmp_path / "lo.vxm")
        lo.merge(hi); lo.merge(hi, -1)
        assert _file(lo, tmp_path / "lo2.vxm") == f600 and lo.stats()["cells_occupied"] == 600
        other.save(str(tmp_path / "o.vxm"))
        with pytest.raises(api.IcetError):
            lo.load(str(tmp_path / "o.vxm"))
        fresh = lo.grown(10)
        fresh.load(str(tmp_path / "o.vxm"))
        assert fresh.stats()["cells_occupied"] == 700 and _file(lo, tmp_path / "lo3.vxm") == f600
        for m in (full, big, other, same, exact, lo, hi, fresh):
            m.close()


def test_negative_zero_count_and_dropped_rows_survive_the_file(gpu_ctx, tmp_path):
    from icet_amd import api
    I = np.asarray(mm.pose(), np.float32).reshape(1, 4, 4)
    for shaped in (False, True):
        model = shm.ShapeMap(0.5)
        m = _new(gpu_ctx, model, 10, shaped)
        add = [np.array([[0.1, 0.1, 0.1], [3.1, 0.2, 0.3]], np.float32)]
        rem = [np.array([[0.3, 0.2, 0.4], [7.7, 0.2, 0.3], [7.6, 0.1, 0.2]], np.float32)]      # cell 0: count 0, sums not; cell x = 15: count -2
        m.add(add, I); m.remove(rem, I)
        model.add(add, I); model.remove(rem, I)
        raw = _file(m, tmp_path / "n.vxm")
        assert raw == msm.write(model, shaped)
        img = msm.read(raw)
        assert sorted(img["words"][:, 0].astype(np.int64)) == [-2, 0, 1]
        back = _new(gpu_ctx, model, 12, shaped)
        back.load(str(tmp_path / "n.vxm"))
        st = back.stats()
        assert st == m.stats() and st["status"] & api.VOXEL_MAP_NEGATIVE and st["cells_negative"] == 1 and st["points_in"] == 5 and st["points_kept"] == -1
        assert _file(back, tmp_path / "n2.vxm") == raw
        m.close(); back.close()
        # a map that dropped rows: points_dropped and TABLE_FULL travel in the header
        scan, _ = _count_case(4097)
        small = _new(gpu_ctx, shm.ShapeMap(POOL_CELL), 10, shaped)
        small.add([scan], I)
        st = small.stats()
        assert st["points_dropped"] > 0 and st["status"] & api.VOXEL_MAP_TABLE_FULL and st["cells_occupied"] == 1024
        info_path = tmp_path / "d.vxm"
        small.save(str(info_path))
        assert api.VoxelMap.snapshot_info(str(info_path))["points_dropped"] == st["points_dropped"]
        back = api.VoxelMap.from_file(gpu_ctx, str(info_path), table_log2=13)
        assert back.stats() == st
        _same_extract(_extract(back), _extract(small))
        small.close(); back.close()


def test_the_shape_rule(gpu_ctx, tmp_path):
    from icet_amd import api
    scan, model = _count_case(257)
    I = np.asarray(mm.pose(), np.float32).reshape(1, 4, 4)
    shaped, plain = _new(gpu_ctx, model, 10, True), _new(gpu_ctx, model, 10, False)
    shaped.add([scan], I); plain.add([scan], I)
    fs, fp = _file(shaped, tmp_path / "s.vxm"), _file(plain, tmp_path / "p.vxm")
    assert len(fs) == 128 + 14 * 8 * 258 and len(fp) == 128 + 5 * 8 * 258 and fp == msm.write(model, False)
    # a shaped file into a plain map: the plain map's own file, W = 5
    into_plain = _new(gpu_ctx, model, 11, False)
    into_plain.load(str(tmp_path / "s.vxm"))
    assert _file(into_plain, tmp_path / "x.vxm") == fp
    into_plain.merge(shaped, -1)
    assert len(_file(into_plain, tmp_path / "x.vxm")) == 128
    # a plain file into a shaped map: refused, by file and by table
    into_shaped = _new(gpu_ctx, model, 11, True)
    for call in (lambda: into_shaped.load(str(tmp_path / "p.vxm")), lambda: into_shaped.merge(plain)):
        with pytest.raises(api.IcetError) as e:
            call()
        assert e.value.status == api.ICET_ERR_BAD_ARG and "plain" in str(e.value)
    assert len(_file(into_shaped, tmp_path / "y.vxm")) == 128
    # after loading a plain file, enable_shape is refused, as on a map that has read rows
    late = _new(gpu_ctx, model, 11, False)
    late.load(str(tmp_path / "p.vxm"))
    with pytest.raises(api.IcetError):
        late.enable_shape()
    assert not late.shape and _file(late, tmp_path / "z.vxm") == fp
    for m in (shaped, plain, into_plain, into_shaped, late):
        m.close()


def test_a_load_makes_index_evidence_and_gaussians_stale(gpu_ctx, tmp_path):
    from icet_amd import api
    s = cs.scene()
    scans, poses = s["scans"], np.asarray(s["poses"], np.float32)
    A = api.VoxelMap(gpu_ctx, cell=s["cell"], table_log2=16, shape=True)
    B = api.VoxelMap(gpu_ctx, cell=s["cell"], table_log2=16, shape=True)
    whole = api.VoxelMap(gpu_ctx, cell=s["cell"], table_log2=16, shape=True)
    A.add(scans[:4], poses[:4]); B.add(scans[4:], poses[4:]); whole.add(scans, poses)
    B.save(str(tmp_path / "b.vxm"))
    keep, descs = _staged([s["held"][1][0]])
    T0 = np.stack([s["starts"][3][1]])
    I = np.asarray(mm.pose(), np.float32).reshape(1, 4, 4)
    # an index, the evidence and the Gaussians of A as it is
    A.index()
    A.evidence(scans[:2], poses[:2], 40.0)
    before = A.register_records(descs, T0, max_iters=20).tobytes()
    q_before = A.query(I, world=True)[0]
    A.load(str(tmp_path / "b.vxm"))
    want_q = whole.query(I, world=True)[0]
    got_q = A.query(I, world=True)[0]
    assert got_q["total"] == want_q["total"] > q_before["total"]
    for k in ("xyz", "count", "key"):
        assert np.array_equal(got_q[k], want_q[k]), k
    after = A.register_records(descs, T0, max_iters=20).tobytes()
    assert after == whole.register_records(descs, T0, max_iters=20).tobytes() and after != before
    with pytest.raises(api.IcetError):                                # the evidence went with the index it was computed on
        A.query(I, world=True, static=True)
    # a save changes nothing: index, evidence and Gaussians stay current
    whole.index(); whole.evidence(scans[:2], poses[:2], 40.0)
    static_before = whole.query(I, world=True, static=True)[0]
    whole.save(str(tmp_path / "w.vxm"))
    static_after = whole.query(I, world=True, static=True)[0]
    assert np.array_equal(static_before["key"], static_after["key"])
    for m in (A, B, whole):
        m.close()


def test_refusals_touch_nothing_and_nothing_else_is_disturbed(gpu_ctx, ctx2, tmp_path, frames):
    import icet_amd
    from icet_amd import api
    lib = api.load_library()
    a, b = frames
    solved = gpu_ctx.solve(a, b, 7, np.zeros(6, np.float32), 24, 75)
    store = icet_amd.KeyframeStore(gpu_ctx, 2)
    store.put([1], [a])
    slot = {k: np.array(store.debug_fetch(1, k)) for k in ("hot", "fit", "slot_of_voxel")}
    scan, model = _count_case(257)
    I = np.asarray(mm.pose(), np.float32).reshape(1, 4, 4)
    m = _new(gpu_ctx, model, 10, True)
    m.add([scan], I)
    before = _file(m, tmp_path / "m.vxm")
    good = os.fsencode(str(tmp_path / "m.vxm"))
    other_cell = api.VoxelMap(gpu_ctx, cell=0.2, table_log2=10, shape=True)
    elsewhere = api.VoxelMap(ctx2, cell=POOL_CELL, table_log2=10, shape=True)
    damaged = bytearray(before); damaged[1000] ^= 0x10
    (tmp_path / "bad.vxm").write_bytes(damaged)
    (tmp_path / "short.vxm").write_bytes(before[:-16])
    B = api.ICET_ERR_BAD_ARG
    refusals = [
        ("a NULL path", lambda: lib.icet_voxel_map_load(m._h, None, 1)),
        ("a NULL path to save", lambda: lib.icet_voxel_map_save(m._h, None)),
        ("a missing file", lambda: lib.icet_voxel_map_load(m._h, os.fsencode(str(tmp_path / "none.vxm")), 1)),
        ("a damaged file", lambda: lib.icet_voxel_map_load(m._h, os.fsencode(str(tmp_path / "bad.vxm")), 1)),
        ("a short file", lambda: lib.icet_voxel_map_load(m._h, os.fsencode(str(tmp_path / "short.vxm")), 1)),
        ("sign 0", lambda: lib.icet_voxel_map_load(m._h, good, 0)),
        ("sign 2", lambda: lib.icet_voxel_map_load(m._h, good, 2)),
        ("merge sign 0", lambda: lib.icet_voxel_map_merge_device(m._h, other_cell._h, 0)),
        ("a NULL source", lambda: lib.icet_voxel_map_merge_device(m._h, None, 1)),
        ("itself", lambda: lib.icet_voxel_map_merge_device(m._h, m._h, 1)),
        ("another cell", lambda: lib.icet_voxel_map_merge_device(m._h, other_cell._h, 1)),
        ("another context", lambda: lib.icet_voxel_map_merge_device(m._h, elsewhere._h, 1)),
        ("an unopenable path", lambda: lib.icet_voxel_map_save(m._h, os.fsencode(str(tmp_path / "no_such_dir" / "x.vxm")))),
    ]
    for k, (what, call) in enumerate(refusals):
        assert call() == B, what
        assert lib.icet_voxel_map_last_error(m._h), what
        assert _file(m, tmp_path / ("after%d.vxm" % k)) == before, what
    other_cell.save(str(tmp_path / "cell.vxm"))
    with pytest.raises(api.IcetError) as e:
        m.load(str(tmp_path / "cell.vxm"))
    assert "cell" in str(e.value) and _file(m, tmp_path / "m2.vxm") == before
    # a failed save leaves nothing at path: the directory is missing, and the temporary's place is taken by a directory
    assert not os.path.exists(str(tmp_path / "no_such_dir"))
    os.mkdir(str(tmp_path / "t.vxm.tmp"))
    with pytest.raises(api.IcetError):
        m.save(str(tmp_path / "t.vxm"))
    assert not os.path.exists(str(tmp_path / "t.vxm")) and os.listdir(str(tmp_path / "t.vxm.tmp")) == []
    assert not any(f.endswith(".tmp") and os.path.isfile(str(tmp_path / f)) for f in os.listdir(str(tmp_path)))
    # a load and a merge that do run leave the context's solve and the store's slot alone
    copy = m.grown(11)
    m.load(str(tmp_path / "m.vxm")); m.merge(copy, -1)
    assert _file(m, tmp_path / "m3.vxm") == before
    copy.close()
    gpu_ctx.sync()
    again = gpu_ctx.solve(a, b, 7, np.zeros(6, np.float32), 24, 75)
    for k in ("X", "pred_stds", "cov"):
        assert np.array_equal(solved[k].view(np.uint32), again[k].view(np.uint32)), k
    for k, v in slot.items():
        assert np.array_equal(v, np.array(store.debug_fetch(1, k))), k
    store.close()
    for x in (m, other_cell, elsewhere):
        x.close()
