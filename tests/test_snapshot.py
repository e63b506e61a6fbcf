"""Snapshots of the keyframe store (include/icet_hip.h: icet_keyframe_store_save / _load / _snapshot_info / _snapshot_slots): a map saved
to a file and loaded back, bit for bit.  On the CPU the format's header (icet_amd/csrc/icet_snapshot.h) is held to the NumPy model of tests/snapshot_model.py
and to itself under AddressSanitizer + UBSan (tests/cpp/test_snapshot.cpp, a stand-alone program).  On the GPU a saved store must come back with every
debug_fetch table equal, answer every query with the same bytes, agree with the model in both directions, and leave everything alone when it refuses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import closure_model as cm
import snapshot_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icet_keyframe_store_save", "icet_keyframe_store_load", "icet_keyframe_store_snapshot_info", "icet_keyframe_store_snapshot_slots")
APP_WORDS = [10, 5, 0x42A00000, 0xC0400000, 0x41400000, 0, 0, 0]        # 10 sectors, 5 rings (Rp = 2: padded parts), rho_max 80, z -3 .. 12
COARSE_WORDS = [64, 0x3E800000, 0xC0400000, 0x41400000, 0x3F000000, 0, 0, 0]


def test_snapshot_entry_points_are_exported_and_refuse_null_arguments(tmp_path):
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    B = api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_save(None, b"x", 0, None) == B and lib.icet_keyframe_store_load(None, b"x", 0) == B
    info = api.SnapshotInfo(); n = C.c_int32(0)
    assert lib.icet_keyframe_store_snapshot_info(None, C.byref(info)) == B and lib.icet_keyframe_store_snapshot_info(b"x", None) == B
    assert lib.icet_keyframe_store_snapshot_info(os.fsencode(str(tmp_path / "missing.kfs")), C.byref(info)) == B
    assert lib.icet_keyframe_store_snapshot_slots(None, 0, None, None, C.byref(n)) == B
    with pytest.raises(api.IcetError):
        api.KeyframeStore.snapshot_info(str(tmp_path / "missing.kfs"))


def test_snapshot_info_reads_what_the_model_writes_and_refuses_a_damaged_file(tmp_path):
    """The host-only calls need no device: the library's validation against a file of the model's."""
    from icet_amd import api
    img = sm.synthetic((7, 3), (0, 1, 21, 5), APP_WORDS, COARSE_WORDS, seed=3)
    raw = sm.write(img)
    p = tmp_path / "model.kfs"; p.write_bytes(raw)
    info = api.KeyframeStore.snapshot_info(str(p))
    assert (info["num_bins_phi"], info["num_bins_theta"], info["n"], info["V"], info["entries"], info["highest_slot"], info["file_bytes"]) == (3, 7, 25, 21, 4, 10, len(raw))
    assert info["thresh"] == np.float32(0.1) and info["buff"] == np.float32(0.1) and info["flags"] == 0
    assert info["appearance"] == dict(sectors=10, rings=5, rho_max=80.0, z_lo=-3.0, z_hi=12.0) and info["coarse"] == dict(cells=64, cell=0.25, z_lo=-3.0, z_hi=12.0, min_span=0.5)
    assert list(info["slots"]) == [1, 4, 7, 10] and list(info["stamps"]) == [1000, -1, 1002, -1]
    for bad in (raw[:-1], raw[:200], raw[:len(raw) // 2] + bytes([raw[len(raw) // 2] ^ 4]) + raw[len(raw) // 2 + 1:], b""):
        p.write_bytes(bad)
        with pytest.raises(api.IcetError) as e:
            api.KeyframeStore.snapshot_info(str(p))
        assert e.value.status == api.ICET_ERR_BAD_ARG
        with pytest.raises(sm.Refused):
            sm.read(bad)


def test_model_checksum_is_the_splitmix_sum():
    """The checksum in wrapping uint64 arithmetic against plain Python integers."""
    M = 2 ** 64

    def mix(z):
        z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 % M; z ^= z >> 27; z = z * 0x94D049BB133111EB % M; z ^= z >> 31
        return z
    rs = np.random.RandomState(1)
    raw = rs.randint(0, 256, 8 * 37, dtype=np.uint8).tobytes()
    words = [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(37)]
    assert sm.checksum(raw) == sum(mix((w + (i + 1) * 0x9E3779B97F4A7C15) % M) for i, w in enumerate(words)) % M
    assert sm.checksum(b"") == 0


@pytest.fixture(scope="module")
def snapshot_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("snapshot") / "test_snapshot")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "test_snapshot.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_header_round_trips_prefixes_byte_changes_and_bad_contents_under_sanitizers(snapshot_exe, tmp_path):
    out = subprocess.run([snapshot_exe, "selftest"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "snapshot ok: 8 images" in out.stdout, out.stderr[-2000:]


@pytest.mark.parametrize("shape,n_slots,app,coarse", [((7, 3), (0, 1, 21, 5), APP_WORDS, COARSE_WORDS), ((7, 3), (21, 0), None, None), ((75, 24), (1, 1800, 0), APP_WORDS, None),
                                                      ((75, 24), (), None, COARSE_WORDS)])
def test_header_and_model_write_the_same_bytes_for_the_same_content(snapshot_exe, tmp_path, shape, n_slots, app, coarse):
    """Model -> header -> bytes and header -> model -> bytes: identical, and the model's reader returns what its writer was given."""
    img = sm.synthetic(shape, n_slots, app, coarse, seed=len(n_slots))
    raw = sm.write(img)
    back = sm.read(raw)
    assert sm.write(back) == raw and len(back["entries"]) == len(n_slots)
    for a, b in zip(img["entries"], back["entries"]):
        assert all(np.array_equal(a[k], b[k]) for k in ("hot", "fit", "sov")) and a["slot"] == b["slot"] and a["stamp"] == b["stamp"]
    src, dst = tmp_path / "model.kfs", tmp_path / "header.kfs"
    src.write_bytes(raw)
    r = subprocess.run([snapshot_exe, "rewrite", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert dst.read_bytes() == raw
    own = tmp_path / "own.kfs"
    assert subprocess.run([snapshot_exe, "write", str(own)], capture_output=True, text=True).returncode == 0
    theirs = own.read_bytes()
    assert sm.write(sm.read(theirs)) == theirs
    src.write_bytes(raw[:-16])                                           # and a refusal is a refusal on both sides
    assert subprocess.run([snapshot_exe, "rewrite", str(src), str(dst)], capture_output=True, text=True).returncode == 2


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

DEV = torch.device("cuda", 0)
SLOTS = [0, 3, 4, 9, 63]
GRIDS = {"7x3": (3, 7), "75x24": (24, 75)}                              # bins_phi, bins_theta: V = 21 (odd: the padded slot_of_voxel row matters) and 1800
WHAT = ("n_slots", "hot", "fit", "slot_of_voxel", "pose", "stamp", "descriptor", "weights", "grid")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).to(DEV)


def _desc(t):
    return (t.data_ptr(), t.shape[1], t.shape[1])


def _scan(scene, T, seed, **kw):
    from icet_amd import lidar_sim as ls
    return np.ascontiguousarray(ls.make_scan(scene, (T[:3, 3].astype(np.float64), T[:3, :3].astype(np.float64)), seed, **kw).numpy().T)


KF_T = [cm.pose_yaw((-5.0 + 1.5 * k, -1.0 + 0.1 * k, 0.0), 0.05 * k) for k in range(4)]
LIVE_T = [cm.pose_yaw((KF_T[k][0, 3] + 0.2, KF_T[k][1, 3] - 0.1, 0.0), 0.05 * k + 0.1) for k in (1, 2)]
THREE = np.array([[5.0, 0.0, 0.0], [0.0, 6.0, 0.5], [-4.0, 1.0, 0.2]], np.float32)      # three points: no voxel holds n of them, a slot with n_slots == 0


@pytest.fixture(scope="module")
def scans():
    """Four keyframes 1.5 m apart and two revisits in lidar_sim scene 2000, another scene's scan, and the scan of three points."""
    from icet_amd import lidar_sim as ls
    scene = ls.make_scene(2000)
    return dict(kf=[_scan(scene, T, 100 + k) for k, T in enumerate(KF_T)], live=[_scan(scene, T, 200 + k) for k, T in enumerate(LIVE_T)],
                other=_scan(ls.make_scene(2001), cm.pose_yaw((0.0, 0.0, 0.0), 0.0), 500), three=THREE)


def test_the_scan_of_three_points_has_no_active_voxel_on_the_oracle(scans):
    from oracle import pyoracle as po
    for bins_phi, bins_theta in GRIDS.values():
        r = po.solve(scans["three"], scans["three"], runlen=1, bins_phi=bins_phi, bins_theta=bins_theta, trace=True)
        assert not np.asarray(r["trace"]["has_fit"]).any()


def _fetch(st, slot):
    """Every debug_fetch table of a slot as bytes (what = 0 .. 8); None for an unoccupied slot, None entries for what the slot lacks."""
    from icet_amd import api
    out = []
    for what in WHAT:
        try:
            v = st.debug_fetch(slot, what)
            out.append(np.asarray(v).tobytes() if not isinstance(v, int) else v)
        except api.IcetError as e:
            assert e.status == api.ICET_ERR_BAD_ARG
            if what == "n_slots":
                return None
            out.append(None)
    return tuple(out)


def _state(st, capacity):
    return [_fetch(st, s) for s in range(capacity)]


def _new_store(ctx, grid, capacity=64, app=True, coarse=True, app_kw=None, coarse_kw=None):
    import icet_amd
    st = icet_amd.KeyframeStore(ctx, capacity, num_bins_phi=GRIDS[grid][0], num_bins_theta=GRIDS[grid][1])
    if coarse:
        st.enable_coarse(**(coarse_kw or {}))
    if app:
        st.enable_appearance(**(app_kw or {}))
    return st


def _fill(st, scans):
    """Slots 0, 3, 4 with poses, 9 with a stamp only, 63 the scan of three points with nothing."""
    st.put(SLOTS, scans["kf"] + [scans["three"]])
    st.set_pose(SLOTS[:3], np.stack(KF_T[:3]), [10, 20, 30])
    st.set_stamp([9], [40])
    st._ctx.sync()


@pytest.fixture(scope="module")
def saved_stores(scans, tmp_path_factory):
    """A filled store of each grid on a context of its own, its state, and the file it saves: made when first asked for."""
    import icet_amd
    made = {}

    def get(grid):
        if grid not in made:
            ctx = icet_amd.Context(0)
            st = _new_store(ctx, grid)
            _fill(st, scans)
            path = str(tmp_path_factory.mktemp("kfs") / ("map_%s.kfs" % grid))
            st.save(path)
            made[grid] = dict(ctx=ctx, st=st, path=path, grid=grid, state=_state(st, 64))
        return made[grid]
    yield get
    for d in made.values():
        d["st"].close(); d["ctx"].close()


@pytest.fixture(params=list(GRIDS))
def saved(request, saved_stores):
    return saved_stores(request.param)


@pytest.fixture
def saved_full(saved_stores):
    """The 75 x 24 store: registrations need its voxels."""
    return saved_stores("75x24")


def _check_filled(state):
    for s in range(64):
        assert (state[s] is not None) == (s in SLOTS), s
    rows = [state[s] for s in SLOTS]
    assert rows[4][0] == 0 and all(r[0] > 0 for r in rows[:4])          # n_slots: the scan of three points gives none
    assert [r[5] for r in rows] == [10, 20, 30, 40, -1]                  # stamps
    for k, r in enumerate(rows):
        T = np.frombuffer(r[4], np.float32).reshape(4, 4)
        assert np.isnan(T[:3]).all() if k >= 3 else np.array_equal(T, KF_T[k].astype(np.float32))
    assert all(r[6] is not None and r[7] is not None and r[8] is not None for r in rows)


@pytest.mark.gpu
def test_round_trip_gives_every_table_back_bit_for_bit(saved):
    """1: save, then load into a fresh store on the same context, into one on a new context, and through from_file."""
    import icet_amd
    from icet_amd import api
    _check_filled(saved["state"])
    info = api.KeyframeStore.snapshot_info(saved["path"])
    assert list(info["slots"]) == SLOTS and list(info["stamps"]) == [10, 20, 30, 40, -1] and info["highest_slot"] == 63 and info["file_bytes"] == os.path.getsize(saved["path"])
    same = _new_store(saved["ctx"], saved["grid"])
    same.load(saved["path"])
    assert _state(same, 64) == saved["state"]
    assert _state(saved["st"], 64) == saved["state"]                     # and the save left the saved store alone
    same.close()
    ctx = icet_amd.Context(0)
    fresh = _new_store(ctx, saved["grid"])
    fresh.load(saved["path"])
    assert _state(fresh, 64) == saved["state"]
    fresh.close()
    made = api.KeyframeStore.from_file(ctx, saved["path"])
    assert made.appearance.sectors == 120 and made.coarse.cells == 256 and _state(made, 64) == saved["state"]
    made.close(); ctx.close()


def _answers(st, scans, live):
    """The four query calls with the same queries: every output buffer as bytes."""
    from icet_amd import api
    ctx = st._ctx
    prm = st._params(7, 0)
    res = []
    out = torch.full((4, 48), float("nan"), dtype=torch.float32, device=DEV); sc = torch.zeros((4, 8), dtype=torch.int32, device=DEV)
    x0 = torch.zeros((4, 6), dtype=torch.float32, device=DEV); x0[:, 0] = torch.tensor([0.0, 0.02, -0.01, 0.03], device=DEV)
    torch.cuda.synchronize()
    st.register_scored_device([3, 4, 0, 9], [_desc(live[0]), _desc(live[1]), _desc(live[0]), _desc(live[1])], prm, out.data_ptr(), sc.data_ptr(), x0.data_ptr())
    ctx.sync()
    res += [out.cpu().numpy().tobytes(), sc.cpu().numpy().tobytes()]
    Q, K, S = 2, 2, 2
    descs = [_desc(t) for t in live]
    poses, stamps = np.stack(LIVE_T), [1000, 1001]

    def run(call):
        rec = torch.zeros((Q, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
        cand = torch.full((Q, K), -7, dtype=torch.int32, device=DEV)
        x0 = torch.full((Q * K * S, 6), float("nan"), dtype=torch.float32, device=DEV); out = torch.full((Q * K * S, 48), float("nan"), dtype=torch.float32, device=DEV)
        sc = torch.zeros((Q * K * S, 8), dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        call(rec.data_ptr(), cand.data_ptr(), x0.data_ptr(), out.data_ptr(), sc.data_ptr())
        ctx.sync()
        recs = np.frombuffer(rec.cpu().numpy().tobytes(), api.CLOSURE_DTYPE)
        return [t.cpu().numpy().tobytes() for t in (rec, cand, x0, out, sc)], recs
    starts = api.LATTICE_STARTS[3:3 + S]
    by_pose, r1 = run(lambda rec, *o: st.close_device(descs, poses, stamps, prm, api.ClosureQuery(3.0, K, 0, S, float("inf"), 0, 0), rec, starts, *o))
    by_app, r2 = run(lambda rec, *o: st.close_appearance_device(descs, stamps, prm, api.ClosureQuery(float("inf"), K, 0, S, float("inf"), 0, 0), rec, starts, *o))
    se = api.KeyframeStore.coarse_search(12, 1, np.pi / 120, True)
    coarse, r3 = run(lambda rec, *o: st.close_coarse_device(descs, None, stamps, prm, api.ClosureQuery(float("inf"), K, 0, S, float("inf"), 0, 0), se, rec, starts, *o))
    assert all((r["n_candidates"] >= 1).all() for r in (r1, r2, r3))     # (the queries are no empty ones)
    return res + by_pose + by_app + coarse


@pytest.mark.gpu
def test_a_loaded_store_answers_every_query_with_the_same_bytes(saved_full, scans):
    """2: register_scored_device, close_device, close_appearance_device and close_coarse_device on the original and on a loaded store."""
    import icet_amd
    from icet_amd import api
    saved = saved_full
    live = [_dev(s) for s in scans["live"]]
    want = _answers(saved["st"], scans, live)
    ctx = icet_amd.Context(0)
    loaded = api.KeyframeStore.from_file(ctx, saved["path"], capacity=64)
    got = _answers(loaded, scans, live)
    assert len(got) == len(want) == 17 and all(a == b for a, b in zip(got, want)), [a == b for a, b in zip(got, want)]
    loaded.close(); ctx.close()


def _model_entry(state_slot, slot, st):
    """A model entry from a slot's debug_fetch tables."""
    n_slots, hot, fit, sov, pose, stamp, desc, weights, grid = state_slot
    V = st.V
    T = np.frombuffer(pose, np.float32).reshape(4, 4)
    tR = np.concatenate([T[:3, 3], T[:3, :3].reshape(9)]).view(np.uint32)
    row = np.full((V + 1) & ~1, 0, np.int16); row[:V] = np.frombuffer(sov, np.int16)
    e = dict(slot=slot, stamp=stamp, pose=None if np.isnan(T[:3]).all() else tR, hot=np.frombuffer(hot, np.uint32).reshape(n_slots, 12),
             fit=np.frombuffer(fit, np.uint32).reshape(n_slots, 20), sov=row)
    if desc is not None:
        a = st.appearance
        e["desc"] = sm.pack_descriptor(np.frombuffer(desc, np.uint8).reshape(a.rings, a.sectors)); e["weights"] = np.frombuffer(weights, np.uint32)
    if grid is not None:
        e["grid"] = np.frombuffer(grid, np.uint32)
    return e


def _params_words(p):
    return np.frombuffer(bytes(p), np.uint32).copy()


@pytest.mark.gpu
def test_the_file_and_the_model_agree_in_both_directions(saved, tmp_path):
    """3: the saved file parsed by the model equals debug_fetch, with the model's checksums; a file the model writes from debug_fetch loads to the same bits."""
    st, state = saved["st"], saved["state"]
    raw = open(saved["path"], "rb").read()
    img = sm.read(raw)                                                   # (every checksum the device summed is the model's, or this refuses)
    V = st.V
    assert img["shape"] == dict(bins_phi=GRIDS[saved["grid"]][0], bins_theta=GRIDS[saved["grid"]][1], n=25, thresh_bits=0x3DCCCCCD, buff_bits=0x3DCCCCCD, flags=0)
    assert np.array_equal(img["appearance"], _params_words(st.appearance)) and np.array_equal(img["coarse"], _params_words(st.coarse))
    assert [e["slot"] for e in img["entries"]] == SLOTS
    model = dict(img, entries=[])
    for e in img["entries"]:
        want = _model_entry(state[e["slot"]], e["slot"], st)
        pad = e["sov"][V:]
        want["sov"][V:] = pad                                            # (the row's padding entry is carried as the store holds it)
        for k in ("hot", "fit", "sov", "desc", "weights", "grid"):
            assert np.array_equal(e[k], want[k]), (e["slot"], k)
        assert e["stamp"] == want["stamp"] and (e["pose"] is None) == (want["pose"] is None) and (e["pose"] is None or np.array_equal(e["pose"], want["pose"]))
        model["entries"].append(want)
    assert sm.write(model) == raw                                        # the model writes the very file
    for e in model["entries"]:                                           # and one with other padding entries loads to the same tables
        e["sov"][V:] = -1
    other = tmp_path / "model.kfs"; other.write_bytes(sm.write(model))
    back = _new_store(saved["ctx"], saved["grid"])
    back.load(str(other))
    assert _state(back, 64) == state
    back.close()


@pytest.mark.gpu
def test_a_subset_merges_into_a_store_that_holds_other_keyframes(saved, scans, tmp_path):
    """4: two of the five slots, loaded 7 slots further into a store with keyframes, poses, descriptors and grids of its own."""
    st, state = saved["st"], saved["state"]
    part = str(tmp_path / "part.kfs")
    st.save(part, [9, 3])                                                # (any order; the file is ascending)
    assert list(type(st).snapshot_info(part)["slots"]) == [3, 9]
    host = _new_store(saved["ctx"], saved["grid"], capacity=20)
    host.put([10, 16, 2, 17], [scans["other"], scans["kf"][0], scans["live"][0], scans["live"][1]])
    host.set_pose([10, 16, 2], np.stack([KF_T[3], KF_T[0], KF_T[1]]), [7, 8, 9])
    before = _state(host, 20)
    assert before[10] is not None and before[16] is not None
    host.load(part, 7)
    after = _state(host, 20)
    assert after[10] == state[3] and after[16] == state[9]               # both targets replaced: slot 16's pose is gone, its stamp the entry's
    assert np.isnan(np.frombuffer(after[16][4], np.float32)[:12]).all() and after[16][5] == 40
    assert all(after[s] == before[s] for s in range(20) if s not in (10, 16))
    host.close()


@pytest.mark.gpu
def test_the_chunk_size_changes_neither_the_file_nor_the_loaded_store(saved, tmp_path):
    """5: every entry its own chunk, then the default."""
    st, ctx = saved["st"], saved["ctx"]
    small, again = str(tmp_path / "small.kfs"), str(tmp_path / "again.kfs")
    ctx.set_option("snapshot_chunk_bytes", 16)                           # below every entry: clamped to the largest, one entry per chunk
    st.save(small)
    a = _new_store(ctx, saved["grid"]); a.load(saved["path"])           # (a default-size file through one-entry chunks)
    ctx.set_option("snapshot_chunk_bytes", 0)
    st.save(again)
    b = _new_store(ctx, saved["grid"]); b.load(small)
    raw = open(saved["path"], "rb").read()
    assert open(small, "rb").read() == raw and open(again, "rb").read() == raw
    assert _state(a, 64) == saved["state"] and _state(b, 64) == saved["state"]
    a.close(); b.close()


@pytest.mark.gpu
def test_feature_matrix(saved, scans, tmp_path):
    """6: file with / without each feature x store with / without it; parameters one bit apart; a store without a feature still refuses its calls."""
    from icet_amd import api
    ctx, grid, state = saved["ctx"], saved["grid"], saved["state"]
    B = api.ICET_ERR_BAD_ARG
    files = {(True, True): saved["path"]}
    for app, coarse in ((False, False), (True, False), (False, True)):
        src = _new_store(ctx, grid, app=app, coarse=coarse)
        _fill(src, scans)
        files[(app, coarse)] = str(tmp_path / ("f%d%d.kfs" % (app, coarse)))
        src.save(files[(app, coarse)])
        info = api.KeyframeStore.snapshot_info(files[(app, coarse)])
        assert (info["appearance"] is not None) == app and (info["coarse"] is not None) == coarse
        src.close()
    for (fa, fc), path in files.items():
        for sa, sc in ((True, True), (False, False), (True, False), (False, True)):
            st = _new_store(ctx, grid, app=sa, coarse=sc)
            st.load(path)
            got = _state(st, 64)
            for s in SLOTS:
                assert got[s][:6] == state[s][:6], (fa, fc, sa, sc, s)                                       # tables, pose and stamp always
                assert got[s][6:8] == (state[s][6:8] if fa and sa else (None, None)), (fa, fc, sa, sc, s)   # descriptors only where both have them
                assert got[s][8] == (state[s][8] if fc and sc else None), (fa, fc, sa, sc, s)
            if not sa:                                                   # as before: the feature's calls are refused
                with pytest.raises(api.IcetError) as e:
                    st.candidates_by_appearance([scans["live"][0]], 2, float("inf"))
                assert e.value.status == B
            elif not fa:                                                 # loaded without descriptors: never an appearance candidate
                cand = st.candidates_by_appearance([scans["live"][0]], 4, float("inf"))[0]
                assert (cand == -1).all()
            if not sc:
                with pytest.raises(api.IcetError) as e:
                    st.coarse_grid([scans["live"][0]])
                assert e.value.status == B
            st.close()
    one_bit = np.float32(80.0).view(np.uint32) ^ np.uint32(1)
    for kw_app, kw_coarse in ((dict(rho_max=float(one_bit.view(np.float32))), None), (None, dict(cell=float((np.float32(0.25).view(np.uint32) ^ np.uint32(1)).view(np.float32)))),
                              (dict(rings=21), None), (None, dict(cells=224))):
        st = _new_store(ctx, grid, app_kw=kw_app, coarse_kw=kw_coarse)
        with pytest.raises(api.IcetError) as e:
            st.load(saved["path"])
        assert e.value.status == B and _state(st, 64) == [None] * 64
        st.close()


@pytest.mark.gpu
def test_a_replayed_graph_reads_the_loaded_keyframe(saved_full, scans, tmp_path):
    """7: a small register_device call is a captured graph from its second call on; a load into the slot it names is what the next replay registers against."""
    saved = saved_full
    ctx = saved["ctx"]
    live = _dev(scans["live"][0])
    one = str(tmp_path / "one.kfs")
    saved["st"].save(one, [4])                                           # keyframe 2
    st = _new_store(ctx, saved["grid"], capacity=8)
    st.put([4], [scans["kf"][1]])
    prm = st._params(7, 0)
    out = torch.zeros((1, 48), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()

    def register(store):
        out.zero_(); torch.cuda.synchronize()
        store.register_device([4], [_desc(live)], prm, out.data_ptr()); ctx.sync()
        return out.cpu().numpy().tobytes()
    first = [register(st) for _ in range(3)]                             # the same call three times: captured, then replayed
    assert first[0] == first[1] == first[2]
    st.load(one)
    second = register(st)
    ref = _new_store(ctx, saved["grid"], capacity=8)
    ref.put([4], [scans["kf"][2]])
    assert second == register(ref) and second != first[0]
    st.close(); ref.close()


@pytest.mark.gpu
def test_refusals_leave_every_slot_and_the_parked_keyframe_alone(saved, scans, tmp_path):
    """8."""
    import icet_amd
    from icet_amd import api
    ctx, grid = saved["ctx"], saved["grid"]
    B = api.ICET_ERR_BAD_ARG
    st = _new_store(ctx, grid, capacity=64)
    st.put([1, 5], [scans["kf"][3], scans["other"]])
    st.set_pose([5], KF_T[1][None], [5])
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    a, b = _dev(scans["kf"][0]), _dev(scans["live"][0])
    ctx.keyframe_device([_desc(a)], prm)

    def parked():
        out = torch.zeros((1, 48), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        ctx.register_device([_desc(b)], prm, out.data_ptr()); ctx.sync()
        return out.cpu().numpy().tobytes()
    want_parked, before = parked(), _state(st, 64)

    def refused(fn, *args, status=B):
        with pytest.raises(icet_amd.IcetError) as e:
            fn(*args)
        assert e.value.status == status, e.value
        assert _state(st, 64) == before
        return str(e.value)
    raw = open(saved["path"], "rb").read()
    other_grid = _new_store(ctx, "7x3" if grid == "75x24" else "75x24")
    refused(other_grid.load, saved["path"])                              # shape: the grid
    other_grid.close()
    other_n = icet_amd.KeyframeStore(ctx, 64, num_bins_phi=GRIDS[grid][0], num_bins_theta=GRIDS[grid][1], n=24)
    refused(other_n.load, saved["path"])                                 # shape: n
    other_n.close()
    refused(st.load, saved["path"], 1)                                   # slot 63 + 1 is beyond the capacity
    refused(st.load, saved["path"], -1)                                  # slot 0 - 1 is no slot
    cut = tmp_path / "cut.kfs"; cut.write_bytes(raw[:len(raw) - 16])
    refused(st.load, str(cut))                                           # truncated
    img = sm.read(raw)
    at = 160 + 128 * len(SLOTS) + 48 * 3 + 5                             # a byte of the first payload
    flipped = tmp_path / "flipped.kfs"; flipped.write_bytes(raw[:at] + bytes([raw[at] ^ 0x10]) + raw[at + 1:])
    assert len(img["entries"][0]["hot"]) > 3
    refused(st.load, str(flipped))                                       # one flipped payload byte
    assert "missing.kfs" in refused(st.load, str(tmp_path / "missing.kfs"))      # a missing path: the reason is in last_error
    for slots in ([1, 2], [1, 1], [64], [-1]):                           # an unoccupied, a repeated, an impossible slot in save
        target = tmp_path / "never.kfs"
        refused(st.save, str(target), slots)
        assert not target.exists() and not (tmp_path / "never.kfs.tmp").exists()
    refused(st.save, str(tmp_path / "no_such_dir" / "x.kfs"))            # a path that cannot be opened
    ctx.set_option("keep", 1)
    refused(st.load, saved["path"], 0, status=api.ICET_ERR_UNSUPPORTED)
    refused(st.save, str(tmp_path / "never.kfs"), None, status=api.ICET_ERR_UNSUPPORTED)
    ctx.set_option("keep", 0)
    assert not (tmp_path / "never.kfs").exists()
    assert parked() == want_parked                                       # the context's parked keyframe is still parked, with its bits
    good = tmp_path / "good.kfs"
    st.save(str(good), [5])                                              # and a save that succeeds leaves no temporary file
    assert good.exists() and not (tmp_path / "good.kfs.tmp").exists() and parked() == want_parked
    st.close()


@pytest.mark.gpu
def test_loaded_slots_survive_what_put_slots_survive(saved, scans, frames):
    """9: reserve, puts into other slots, a whole solve on the context, another store's calls."""
    import icet_amd
    ctx = icet_amd.Context(0)
    st = _new_store(ctx, saved["grid"])
    st.load(saved["path"])
    assert _state(st, 64) == saved["state"]
    st.reserve(80)
    st.put([1, 70], [scans["other"], scans["live"][0]])
    ctx.solve(frames[0], frames[1], 7, np.zeros(6), 24, 75)
    other = _new_store(ctx, "75x24", capacity=4)
    other.put([2], [scans["kf"][0]])
    other.find_closures([scans["live"][0]], LIVE_T[:1], [99], 7, 100.0, 1)
    got = _state(st, 80)
    assert [got[s] for s in SLOTS] == [saved["state"][s] for s in SLOTS]
    assert all((got[s] is not None) == (s in SLOTS + [1, 70]) for s in range(80))
    other.close(); st.close(); ctx.close()
