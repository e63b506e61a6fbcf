"""The loop-closure query of the keyframe store (include/icet_hip.h: icet_keyframe_store_set_pose / _candidates_device / _close_device,
icet_pose_step_from_x).  The rule is held to the NumPy model of tests/closure_model.py: on the host through the header the
kernels compile (tests/cpp/test_closure.cpp), on the GPU through the calls themselves; the registrations of a query are held, bit for bit, to the
entries a caller would otherwise chain by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import closure_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icet_keyframe_store_set_pose", "icet_keyframe_store_candidates_device", "icet_keyframe_store_close_device", "icet_pose_step_from_x")
KNOWN_X0 = np.array([0.38235973, -0.31032409, 0.0, 0.0, 0.0, 0.4])      # keyframe (3, -2, 0) yaw 0.7, live scan (3.45, -1.8, 0) yaw 1.1, in double


def test_closure_entry_points_are_exported_and_refuse_a_null_store():
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "icet_pose_step_from_x" in api._NON_STATUS
    p = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    q = api.ClosureQuery(5.0, 4, 0, 1, float("inf"), 0, 0)
    idx = (C.c_int32 * 1)(0)
    T = np.eye(4, dtype=np.float32); st = np.zeros(1, np.int64)
    assert lib.icet_keyframe_store_set_pose(None, 1, idx, T.ctypes.data, st.ctypes.data) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_candidates_device(None, 1, T.ctypes.data, st.ctypes.data, C.byref(q), None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_close_device(None, C.byref(p), 1, None, T.ctypes.data, st.ctypes.data, C.byref(q), None, None, None, None, None, None) == api.ICET_ERR_BAD_ARG
    # the host helper needs no device: one step of X = (1, 2, 3, 0, 0, pi / 2) is [Rz(-90 deg)^T ...]: R(X)^T and R(X)^T X_t of the model
    X = np.array([1.0, 2.0, 3.0, 0.1, -0.2, 1.3], np.float32)
    assert np.allclose(api.pose_step_from_X(X), cm.pose_step64(X), rtol=0, atol=1e-6)
    assert np.array_equal(api.pose_step_from_X(np.zeros(6)), np.eye(4, dtype=np.float32))


def test_record_sizes_match_the_ctypes_mirrors(tmp_path):
    from icet_amd import api
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icet_hip.h"\nint main(void){ printf("%d %d %d %d %d\\n", (int)sizeof(icet_closure), (int)sizeof(icet_closure_query), '
                   '(int)offsetof(icet_closure, out), (int)offsetof(icet_closure, score), (int)offsetof(icet_closure_query, n_starts)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
    assert got == [C.sizeof(api.Closure), C.sizeof(api.ClosureQuery), api.Closure.out.offset, api.Closure.score.offset, api.ClosureQuery.n_starts.offset]
    assert got[0] % 16 == 0 and got[1] % 4 == 0
    assert api.CLOSURE_DTYPE.itemsize == got[0] and api.CLOSURE_DTYPE.fields["out"][1] == got[2] and api.CLOSURE_DTYPE.fields["score"][1] == got[3]


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    """tests/cpp/test_closure.cpp: icet_closure.h compiled for the host, nothing contracted."""
    exe = str(tmp_path_factory.mktemp("closure") / "test_closure")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_closure.cpp"), "-o", exe])
    return exe


def _run(exe, mode, arr, out_dtype, tmp):
    fin, fout = os.path.join(tmp, mode + ".in"), os.path.join(tmp, mode + ".out")
    np.ascontiguousarray(arr).tofile(fin)
    subprocess.check_call([exe, mode, fin, fout])
    return np.fromfile(fout, out_dtype)


def _within_one_ulp(got, model32):
    """|got - model| <= 1 float32 ulp of the model, or both zero."""
    got = np.asarray(got, np.float32); model32 = np.asarray(model32, np.float32)
    return (np.abs(got.astype(np.float64) - model32.astype(np.float64)) <= np.spacing(np.abs(model32)).astype(np.float64)) | ((got == 0) & (model32 == 0))


def _random_pose(rs, span=100.0):
    ang = np.array([rs.uniform(-1.5, 1.5), rs.uniform(-1.5, 1.5), rs.uniform(-np.pi, np.pi)])
    return cm.pose(rs.uniform(-span, span, 3), cm.euler_R(*ang).T)


def test_rule_integer_parts_and_key_order(rule_exe, tmp_path):
    assert subprocess.check_output([rule_exe, "self"]).strip().endswith(b"self ok")
    # keys against the model's order: ties in d2 go to the lower slot, a NaN pose is never a candidate, d2 == radius^2 is in
    rs = np.random.RandomState(5)
    n = 400
    ts = rs.uniform(-20, 20, (n, 3)).astype(np.float32)
    ts[50:60] = ts[40:50]                                               # ties
    ts[7, 1] = np.nan; ts[9] = np.nan
    ts[11] = (3.0, 4.0, 0.0)                                            # d2 = 25 exactly from the origin
    tq = np.zeros(3, np.float32)
    for radius in (5.0, 12.5, 0.0):
        rec = np.zeros((n, 8), np.float32); rec[:, 0:3] = tq; rec[:, 3:6] = ts; rec[:, 6] = radius; rec[:, 7] = np.arange(n)
        keys = _run(rule_exe, "key", rec, np.uint64, str(tmp_path))
        el = np.nonzero(keys != np.uint64(0xFFFFFFFFFFFFFFFF))[0]
        order = el[np.argsort(keys[el], kind="stable")]
        want, _ = cm.candidates(tq, 0, ts, np.zeros(n, np.int64), np.ones(n, bool), radius, n)
        assert np.array_equal(order, want[want >= 0])
        assert 7 not in order and 9 not in order
        assert (11 in order) == (radius >= 5.0)
    assert list(cm.candidates(ts[40], 0, ts, np.zeros(n, np.int64), np.ones(n, bool), 0.0, 4)[0]) == [40, 50, -1, -1]


def test_rule_start_pose_against_the_double_model(rule_exe, tmp_path):
    kf, live = cm.pose_yaw((3.0, -2.0, 0.0), 0.7), cm.pose_yaw((3.45, -1.8, 0.0), 1.1)
    got = _run(rule_exe, "start", np.concatenate([live.ravel(), kf.ravel()]), np.float32, str(tmp_path))
    # the poses are float32: 3.45 and 1.8 carry up to 1.2e-7 + 6e-8, the rotation entries 6e-8 x |d| = 0.5, the result one rounding of 3e-8
    assert np.abs(got - KNOWN_X0).max() < 5e-7, got
    assert np.abs(cm.start_pose64(live, kf) - KNOWN_X0).max() < 5e-7
    c, s_ = np.cos(1.1), np.sin(1.1)                                    # the same answer from the unrounded poses, in double
    exact = np.array([[c, -s_], [s_, c]]).T @ np.array([0.45, 0.2])
    assert np.abs(exact - KNOWN_X0[:2]).max() < 5e-9 and abs((1.1 - 0.7) - KNOWN_X0[5]) < 1e-15
    rs = np.random.RandomState(1)
    pairs = np.stack([np.concatenate([_random_pose(rs).ravel(), _random_pose(rs).ravel()]) for _ in range(2000)]).astype(np.float32)
    got = _run(rule_exe, "start", pairs, np.float32, str(tmp_path)).reshape(-1, 6)
    model = np.stack([cm.start_pose(p[:16], p[16:]) for p in pairs])
    ok = _within_one_ulp(got, model)
    assert ok.all(), (np.argwhere(~ok)[:5], got[~ok][:5], model[~ok][:5])
    # euler -> R -> euler in double
    ang = np.stack([rs.uniform(-1.5, 1.5, 2000), rs.uniform(-1.5, 1.5, 2000), rs.uniform(-np.pi, np.pi, 2000)], 1)
    back = _run(rule_exe, "euler", ang, np.float64, str(tmp_path)).reshape(-1, 3)
    print("euler round trip worst %.2e" % np.abs(back - ang).max())
    assert np.abs(back - ang).max() <= 1e-14


def test_pose_step_then_start_pose_returns_X(rule_exe, tmp_path):
    rs = np.random.RandomState(3)
    n = 20000
    X = np.concatenate([rs.uniform(-10, 10, (n, 3)), rs.uniform(-1.2, 1.2, (n, 2)), rs.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)
    T = _run(rule_exe, "step", X, np.float32, str(tmp_path)).reshape(-1, 16)
    assert np.abs(T[:5].reshape(5, 4, 4) - np.stack([cm.pose_step64(x) for x in X[:5]])).max() < 1e-6
    ident = np.tile(np.eye(4, dtype=np.float32).ravel(), (n, 1))
    back = _run(rule_exe, "start", np.concatenate([T, ident], 1), np.float32, str(tmp_path)).reshape(-1, 6)
    dt = np.abs(back[:, :3] - X[:, :3]).max()
    da = np.abs(back[:, 3:].astype(np.float64) - X[:, 3:]); da = np.minimum(da, 2 * np.pi - da).max()      # (yaw = +-pi is one angle)
    print("step -> start pose: worst |dt| %.2e m, |dangle| %.2e rad" % (dt, da))
    assert dt <= 2e-6 and da <= 3e-7


def test_oracle_converges_from_the_rule_start_pose_and_not_from_zero(rule_exe, tmp_path):
    """Why the feature exists: a revisit 0.49 m and 0.4 rad of yaw from its keyframe registers from the rule's X0 (and from that X0 under the drift a stored
    pose may carry), and does not from X0 = 0."""
    from icet_amd import lidar_sim as ls
    from oracle import pyoracle as po
    scene = ls.make_scene(2000)
    kf, live = cm.pose_yaw((3.0, -2.0, 0.0), 0.7), cm.pose_yaw((3.45, -1.8, 0.0), 1.1)
    s1 = ls.make_scan(scene, (kf[:3, 3].astype(np.float64), kf[:3, :3].astype(np.float64)), 11).numpy().T
    s2 = ls.make_scan(scene, (live[:3, 3].astype(np.float64), live[:3, :3].astype(np.float64)), 12).numpy().T
    x0 = _run(rule_exe, "start", np.concatenate([live.ravel(), kf.ravel()]), np.float32, str(tmp_path))
    for name, start in (("rule", x0), ("drifted", x0 + np.array([0.15, -0.10, 0, 0, 0, 0.01], np.float32))):
        r = po.solve(s1, s2, x0=start.astype(np.float32), runlen=7, bins_phi=24, bins_theta=75)
        dt, dr = np.abs(r["X"][:3] - x0[:3]).max(), np.abs(r["X"][3:] - x0[3:]).max()
        print("%s: |dt| %.4f m |dr| %.4f rad" % (name, dt, dr))
        assert dt <= 0.02 and dr <= 0.035
    r = po.solve(s1, s2, x0=np.zeros(6, np.float32), runlen=7, bins_phi=24, bins_theta=75)
    dt = np.abs(r["X"][:3] - x0[:3]).max()
    print("zero: |dt| %.4f m" % dt)
    assert dt > 0.2


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

DEV = torch.device("cuda", 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).to(DEV)


def _desc(t):
    return (t.data_ptr(), t.shape[1], t.shape[1])


def _recs(t):
    from icet_amd import api
    return np.frombuffer(t.cpu().numpy().tobytes(), api.CLOSURE_DTYPE).copy()


def _scores(t):
    from icet_amd import api
    return np.frombuffer(t.cpu().numpy().tobytes(), api.SCORE_DTYPE).copy()


class _PoseBook:
    """The host's copy of what the store should hold: pose, stamp, has-pose per slot."""

    def __init__(self, cap):
        self.T = np.full((cap, 4, 4), np.nan, np.float32); self.stamp = np.full(cap, -1, np.int64); self.has = np.zeros(cap, bool)

    def grow(self, cap):
        old = self.has.size
        T = np.full((cap, 4, 4), np.nan, np.float32); T[:old] = self.T
        st = np.full(cap, -1, np.int64); st[:old] = self.stamp
        has = np.zeros(cap, bool); has[:old] = self.has
        self.T, self.stamp, self.has = T, st, has

    def set(self, slots, T, stamps):
        self.T[slots] = T; self.stamp[slots] = stamps; self.has[slots] = True

    def clear(self, slots):
        self.T[slots] = np.nan; self.stamp[slots] = -1; self.has[slots] = False

    def candidates(self, Tq, sq, radius, k, gap):
        return cm.candidates(Tq[:3, 3], sq, self.T[:, :3, 3], self.stamp, self.has, radius, k, gap)


def _check_candidates(store, book, Tq, sq, radius, k, gap):
    cand, x0 = store.candidates(Tq, sq, radius, k, gap)
    counts = []
    for q in range(len(Tq)):
        want, _ = book.candidates(Tq[q], sq[q], radius, k, gap)
        assert np.array_equal(cand[q], want), (q, radius, k, gap, cand[q], want)
        for j in range(k):
            model = cm.start_pose(Tq[q], book.T[want[j]]) if want[j] >= 0 else np.zeros(6, np.float32)
            assert _within_one_ulp(x0[q, j], model).all(), (q, j, x0[q, j], model)
        counts.append(int((book.candidates(Tq[q], sq[q], radius, 4096, gap)[0] >= 0).sum()))
    return counts


@pytest.mark.gpu
def test_candidates_equal_the_rule_exactly(frames, sample_pc):
    import icet_amd
    from test_keyframe_store import _keyframes
    kf, _ = _keyframes(frames, sample_pc)
    ctx = icet_amd.Context(0)
    cap = 4096
    st = icet_amd.KeyframeStore(ctx, cap)
    n_put = 15 * 256                                                    # slots 3840 .. 4095 stay empty
    for first in range(0, n_put, 256):
        st.put_device(list(range(first, first + 256)), [_desc(kf[(first + i) % 4]) for i in range(256)])
    rs = np.random.RandomState(17)
    book = _PoseBook(cap)
    posed = np.sort(rs.choice(n_put, 3500, replace=False))              # 340 occupied slots keep no pose
    T = np.stack([_random_pose(rs) for _ in posed])
    T[:, 2, 3] = rs.uniform(-2, 2, posed.size).astype(np.float32)
    T[100:160, :3, 3] = T[200:260, :3, 3]                               # duplicated positions: ties in d2
    T[[5, 900, 2000], 0, 3] = np.nan; T[1500, :3, 3] = np.nan           # a few NaN poses
    stamps = rs.randint(0, 4000, posed.size).astype(np.int64)
    st.set_pose(posed, T, stamps)
    book.set(posed, T, stamps)
    assert np.array_equal(st.debug_fetch(int(posed[3]), "pose"), T[3]) and st.debug_fetch(int(posed[3]), "stamp") == int(stamps[3])
    unposed = int(np.setdiff1d(np.arange(n_put), posed)[0])
    assert np.isnan(st.debug_fetch(unposed, "pose")[:3, 3]).all() and st.debug_fetch(unposed, "stamp") == -1
    Tq = np.stack([_random_pose(rs) for _ in range(5)])
    Tq[0, :3, 3] = T[210, :3, 3]                                        # on a duplicated position: d2 == 0 twice
    Tq[1, :3, 3] = T[10, :3, 3] + np.float32(0.25)
    sq = np.array([2000, 10, 3990, 1234, 50], np.int64)
    seen = set()
    for k in (1, 7, 32):
        for radius in (1e-3, 8.0, 30.0):
            for gap in (0, 50):
                for n in _check_candidates(st, book, Tq, sq, radius, k, gap):
                    seen.add("none" if n == 0 else ("fewer" if n < k else "more"))
    assert seen == {"none", "fewer", "more"}
    # a radius that reaches a slot exactly: d2 == radius^2 is in
    d2 = cm.dist2(Tq[2, :3, 3], book.T[:, :3, 3]); d2 = d2[book.has & np.isfinite(d2)]
    r_edge = np.sqrt(np.sort(d2)[3].astype(np.float64))
    for radius in (np.float32(r_edge), np.nextafter(np.float32(r_edge), np.float32(0)), np.nextafter(np.float32(r_edge), np.float32(1e9))):
        _check_candidates(st, book, Tq[2:3], sq[2:3], float(radius), 7, 0)
    # reserve carries poses and stamps over
    st.reserve(5000); book.grow(5000)
    _check_candidates(st, book, Tq, sq, 8.0, 7, 0)
    assert np.array_equal(st.debug_fetch(int(posed[3]), "pose"), T[3]) and st.debug_fetch(int(posed[3]), "stamp") == int(stamps[3])
    # a put replaces a posed slot: its pose is gone; a new slot beyond the old capacity gets one
    gone = int(book.candidates(Tq[1], sq[1], 30.0, 1, 0)[0][0])
    st.put_device([gone, 4500], [_desc(kf[0]), _desc(kf[1])]); book.clear([gone])
    st.set_pose([4500], Tq[3:4], [77]); book.set([4500], Tq[3], [77])
    assert np.isnan(st.debug_fetch(gone, "pose")[:3, 3]).all()
    for k in (1, 32):
        _check_candidates(st, book, Tq, sq, 30.0, k, 0)
    assert int(st.candidates(Tq[3:4], sq[3:4], 1.0, 1)[0][0, 0]) == 4500
    # refusals: an empty slot, a slot named twice
    for bad in ([4000], [1, 1]):
        with pytest.raises(icet_amd.IcetError) as e:
            st.set_pose(bad, Tq[:len(bad)], [0] * len(bad))
        assert e.value.status == icet_amd.api.ICET_ERR_BAD_ARG
    st.close(); ctx.close()


KF_SLOTS = [3, 0, 9, 5, 12, 7, 1, 14]
OFFSETS = np.array([[0, 0, 0, 0, 0, 0], [0.05, 0, 0, 0, 0, 0.005], [-0.05, 0.02, 0, 0, 0, -0.005]], np.float32)


@pytest.fixture(scope="module")
def drive():
    """A closed drive through scene 2000: 8 keyframes along a line, stored with a drift of at most 0.15 m / 0.01 rad; 4 revisit scans 0.3 - 0.6 m and
    0.2 - 0.5 rad of yaw from their nearest keyframe."""
    import icet_amd
    from icet_amd import lidar_sim as ls
    scene = ls.make_scene(2000)
    rs = np.random.RandomState(23)
    ctx = icet_amd.Context(0)
    st = icet_amd.KeyframeStore(ctx, 16)
    true_kf = [cm.pose_yaw((-5.0 + 1.5 * k, -1.0 + 0.1 * k, 0.0), 0.05 * k) for k in range(8)]
    kf_scans = [ls.make_scan(scene, (T[:3, 3].astype(np.float64), T[:3, :3].astype(np.float64)), 100 + k, device=DEV) for k, T in enumerate(true_kf)]
    st.put_device(KF_SLOTS, [_desc(t) for t in kf_scans])
    stored = []
    for k, T in enumerate(true_kf):
        d = rs.uniform(-0.08, 0.08, 2)
        stored.append(cm.pose_yaw((T[0, 3] + d[0], T[1, 3] + d[1], 0.0), 0.05 * k + rs.uniform(-0.01, 0.01)))
    stamps = np.arange(8, dtype=np.int64) * 10
    st.set_pose(KF_SLOTS, np.stack(stored), stamps)
    near = [1, 3, 5, 7]
    off = [(0.35, 0.20, 0.30), (-0.30, 0.30, 0.45), (0.25, -0.35, -0.25), (0.40, 0.10, 0.20)]
    live = [cm.pose_yaw((true_kf[k][0, 3] + o[0], true_kf[k][1, 3] + o[1], 0.0), 0.05 * k + o[2]) for k, o in zip(near, off)]
    scans = [ls.make_scan(scene, (T[:3, 3].astype(np.float64), T[:3, :3].astype(np.float64)), 200 + i, device=DEV) for i, T in enumerate(live)]
    book = _PoseBook(16); book.set(KF_SLOTS, np.stack(stored), stamps)
    torch.cuda.synchronize()
    yield dict(ctx=ctx, st=st, scans=scans, live=np.stack(live), live_stamps=np.array([500, 510, 520, 530], np.int64), book=book, near=[KF_SLOTS[k] for k in near],
               kf_scans=kf_scans)
    st.close(); ctx.close()


def _close(d, qs, radius, K, S=3, max_chi2=float("inf"), min_voxels=0, gap=0, outputs=True, runlen=7, poses=None, flags=0):
    """One close_device call for the queries `qs` of the drive; returns records (and cand, x0, out, score when every output is asked for)."""
    from icet_amd import api
    st = d["st"]
    Q, R = len(qs), len(qs) * K * S
    rec = torch.zeros((Q, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    cand = torch.full((Q, K), -7, dtype=torch.int32, device=DEV)
    x0 = torch.full((R, 6), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((R, 48), float("nan"), dtype=torch.float32, device=DEV)
    sc = torch.zeros((R, 8), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    query = api.ClosureQuery(float(radius), K, gap, S, float(max_chi2), int(min_voxels), 0)
    T = d["live"][qs] if poses is None else poses
    ptr = (lambda t: t.data_ptr()) if outputs else (lambda t: None)
    offsets = OFFSETS[:S] if 1 <= S <= len(OFFSETS) else None
    st.close_device([_desc(d["scans"][q]) for q in qs], T, d["live_stamps"][qs], st._params(runlen, flags), query, rec.data_ptr(), offsets,
                    ptr(cand), ptr(x0), ptr(out), ptr(sc))
    d["ctx"].sync()
    return dict(rec=_recs(rec), cand=cand.cpu().numpy(), x0=x0.cpu().numpy(), out=out.cpu().numpy(), score=_scores(sc), sc_dev=sc, out_dev=out, x0_dev=x0)


def _same_record(a, b, skip=()):
    a, b = a.copy(), b.copy()
    for f in skip:
        a[f] = 0; b[f] = 0
    return a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_query_carries_the_bits_of_the_path_it_replaces(drive):
    from icet_amd import api
    d = drive
    st, ctx, K, S = d["st"], d["ctx"], 4, 3
    qs = [0, 1, 2, 3]
    res = _close(d, qs, 2.6, K, S)
    rec, cand, x0 = res["rec"], res["cand"], res["x0"]
    for i, q in enumerate(qs):
        want, wd2 = d["book"].candidates(d["live"][q], d["live_stamps"][q], 2.6, K, 0)
        assert np.array_equal(cand[i], want) and want[0] == d["near"][q]
        assert rec[i]["n_candidates"] == int((want >= 0).sum())
    assert (cand >= 0).sum() < cand.size and (cand >= 0).sum() >= 8         # some padding, mostly live
    # the start poses: the rule (within 1 ulp of the double model), then the offsets added in float32
    cand2, xb = st.candidates(d["live"][qs], d["live_stamps"][qs], 2.6, K)
    assert np.array_equal(cand2, cand)
    for i in range(len(qs)):
        for k in range(K):
            model = cm.start_pose(d["live"][qs[i]], d["book"].T[cand[i, k]]) if cand[i, k] >= 0 else np.zeros(6, np.float32)
            assert _within_one_ulp(xb[i, k], model).all()
            for s in range(S):
                r = (i * K + k) * S + s
                want_x0 = (xb[i, k] + OFFSETS[s]) if cand[i, k] >= 0 else np.zeros(6, np.float32)
                assert x0[r].tobytes() == want_x0.astype(np.float32).tobytes()
    # the live registrations: bitwise what the store's scored entry gives for the same slots, scans and the x0 the call reported
    live = [r for r in range(len(qs) * K * S) if cand.reshape(-1)[r // S] >= 0]
    slots = [int(cand.reshape(-1)[r // S]) for r in live]
    descs = [_desc(d["scans"][qs[r // (K * S)]]) for r in live]
    xl = res["x0_dev"][live].contiguous()
    out2 = torch.zeros((len(live), 48), dtype=torch.float32, device=DEV); sc2 = torch.zeros((len(live), 8), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st.register_scored_device(slots, descs, st._params(7, 0), out2.data_ptr(), sc2.data_ptr(), xl.data_ptr())
    ctx.sync()
    assert np.array_equal(out2.cpu().numpy().view(np.uint32), res["out"][live].view(np.uint32))
    assert _scores(sc2).tobytes() == res["score"][live].tobytes()
    pad = [r for r in range(len(qs) * K * S) if r not in live]
    assert (res["score"]["voxels"][pad] == 0).all()
    # the winner: icet_select_best_device on those scores, group = query
    best = torch.full((len(qs),), -9, dtype=torch.int32, device=DEV)
    group = np.repeat(np.arange(len(qs), dtype=np.int32), K * S)
    ctx.select_best_device(group, len(qs), res["sc_dev"].data_ptr(), best.data_ptr())
    ctx.sync()
    best = best.cpu().numpy()
    assert np.array_equal(best, api.select_best(res["score"], group, len(qs)))
    for i in range(len(qs)):
        r = int(best[i])
        assert r >= 0 and rec[i]["reg"] == r and rec[i]["slot"] == cand.reshape(-1)[r // S] and rec[i]["accepted"] == 1
        assert rec[i]["out"].tobytes() == res["out"][r].tobytes() and rec[i]["score"].tobytes() == res["score"][r].tobytes() and rec[i]["x0"].tobytes() == x0[r].tobytes()
        assert rec[i]["stamp"] == d["book"].stamp[rec[i]["slot"]]
        _, wd2 = d["book"].candidates(d["live"][qs[i]], d["live_stamps"][qs[i]], 2.6, K, 0)
        assert rec[i]["d2"].tobytes() == wd2[(r // S) % K].tobytes()
    # the same records when the store uses buffers of its own
    own = _close(d, qs, 2.6, K, S, outputs=False)["rec"]
    assert own.tobytes() == rec.tobytes()
    # find_closures: the host-scan form returns the same winners
    got = st.find_closures([t.cpu().numpy().T for t in d["scans"]], d["live"], d["live_stamps"], 7, 2.6, K, starts=OFFSETS)
    for i in range(len(qs)):
        assert got[i]["slot"] == int(rec[i]["slot"]) and got[i]["accepted"] and np.array_equal(got[i]["X"], rec[i]["out"][:6]) and got[i]["score"]["voxels"] == int(rec[i]["score"]["voxels"])


@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["ROUNDTRIP_SCAN2", "DOUBLE_W", "REJECT_MOVING"])
def test_per_call_flags_reach_the_registrations(drive, flag):
    """The per-call flags apply as in the store's own entries: with padding registrations in the call, the live ones still carry the scored entry's bits."""
    from icet_amd import api
    d = drive
    st, ctx, K, S = d["st"], d["ctx"], 4, 2
    fl = getattr(api, "FLAG_" + flag)
    res = _close(d, [1, 3], 2.6, K, S, flags=fl)
    cand = res["cand"].reshape(-1)
    live = [r for r in range(2 * K * S) if cand[r // S] >= 0]
    assert 0 < len(live) < 2 * K * S
    descs = [_desc(d["scans"][[1, 3][r // (K * S)]]) for r in live]
    xl = res["x0_dev"][live].contiguous()
    out2 = torch.zeros((len(live), 48), dtype=torch.float32, device=DEV); sc2 = torch.zeros((len(live), 8), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st.register_scored_device([int(cand[r // S]) for r in live], descs, st._params(7, fl), out2.data_ptr(), sc2.data_ptr(), xl.data_ptr())
    ctx.sync()
    assert np.array_equal(out2.cpu().numpy().view(np.uint32), res["out"][live].view(np.uint32))
    assert _scores(sc2).tobytes() == res["score"][live].tobytes()
    plain = _close(d, [1, 3], 2.6, K, S)
    assert np.array_equal(plain["cand"], res["cand"]) and (res["rec"]["slot"] >= 0).all()
    if flag == "ROUNDTRIP_SCAN2":
        assert plain["out"][live].tobytes() != res["out"][live].tobytes()      # (the flag did reach the loop)


@pytest.mark.gpu
def test_the_gate(drive):
    d = drive
    base = _close(d, [0, 1], 2.6, 4)["rec"]
    assert (base["slot"] >= 0).all() and (base["accepted"] == 1).all()
    chi, vox = np.float32(base[0]["score"]["chi2_per_voxel"]), int(base[0]["score"]["voxels"])
    assert np.isfinite(chi) and vox > 0
    for max_chi2, min_voxels, want in ((np.nextafter(chi, np.float32(-np.inf)), 0, 0), (chi, 0, 1), (np.nextafter(chi, np.float32(np.inf)), 0, 1),
                                       (float("inf"), vox + 1, 0), (float("inf"), vox, 1), (chi, vox, 1), (np.nextafter(chi, np.float32(-np.inf)), vox + 1, 0)):
        rec = _close(d, [0, 1], 2.6, 4, max_chi2=max_chi2, min_voxels=min_voxels)["rec"]
        assert rec[0]["accepted"] == want, (max_chi2, min_voxels)
        assert _same_record(rec[0], base[0], skip=("accepted",))


@pytest.mark.gpu
def test_padding_and_empties(drive):
    import icet_amd
    d = drive
    # query 3 (near the last keyframe): a radius that admits exactly two slots
    d2 = np.sort(cm.dist2(d["live"][3][:3, 3], d["book"].T[:, :3, 3])[d["book"].has])
    radius = float(np.sqrt((np.float64(d2[1]) + np.float64(d2[2])) / 2))
    wide, tight = _close(d, [0, 3], radius, 8), _close(d, [0, 3], radius, 2)
    assert (wide["cand"][1] >= 0).sum() == 2 and np.array_equal(wide["cand"][1][:2], tight["cand"][1])
    a, b = wide["rec"][1], tight["rec"][1]
    assert a["slot"] >= 0 and a["n_candidates"] == 2
    assert _same_record(a, b, skip=("reg",))
    assert (int(a["reg"]) - 1 * 8 * 3) == (int(b["reg"]) - 1 * 2 * 3)           # the same (candidate, start) in the other numbering
    # a query that finds none
    far = d["live"][[0, 1]].copy(); far[1, :3, 3] += np.float32(1000.0)
    res = _close(d, [0, 1], 2.6, 4, poses=far)
    r = res["rec"][1]
    assert r["slot"] == -1 and r["reg"] == -1 and r["accepted"] == 0 and r["n_candidates"] == 0 and not r["out"].any() and not r["x0"].any() and r["score"]["voxels"] == 0
    assert res["rec"][0]["slot"] == d["near"][0]
    # a store without any pose, and a store without any keyframe: ICET_OK and Q empty records
    st2 = icet_amd.KeyframeStore(d["ctx"], 8)
    keep = d["st"]
    try:
        for filled in (False, True):
            if filled:
                st2.put_device([2, 5], [_desc(d["kf_scans"][0]), _desc(d["kf_scans"][1])])
            d["st"] = st2
            rec = _close(d, [0, 1, 2], 50.0, 4)["rec"]
            assert (rec["slot"] == -1).all() and (rec["accepted"] == 0).all() and (rec["n_candidates"] == 0).all() and not rec["out"].any()
    finally:
        d["st"] = keep
        st2.close()


@pytest.mark.gpu
def test_batching_and_consecutive_calls(drive):
    d = drive
    K, S = 4, 3
    batch = _close(d, [0, 1, 2, 3], 2.6, K, S)
    for q in range(4):
        one = _close(d, [q], 2.6, K, S)
        a, b = batch["rec"][q].copy(), one["rec"][0].copy()
        assert int(a["reg"]) - q * K * S == int(b["reg"])                # (the registration number counts the queries in front)
        assert _same_record(a, b, skip=("reg",))
        assert np.array_equal(batch["cand"][q], one["cand"][0])
    # two consecutive calls of one shape with different query poses, nothing waited for in between: each gets its own candidates
    from icet_amd import api
    st = d["st"]
    recs = [torch.zeros((1, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=DEV) for _ in range(3)]
    cands = [torch.full((1, K), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    query = api.ClosureQuery(2.6, K, 0, S, float("inf"), 0, 0)
    order = [0, 2, 0]
    for i, q in enumerate(order):                                       # the same scan every time: only the pose differs
        st.close_device([_desc(d["scans"][0])], d["live"][q:q + 1], d["live_stamps"][q:q + 1], st._params(7, 0), query, recs[i].data_ptr(), OFFSETS, cands[i].data_ptr())
    d["ctx"].sync()
    for i, q in enumerate(order):
        want, _ = d["book"].candidates(d["live"][q], d["live_stamps"][q], 2.6, K, 0)
        assert np.array_equal(cands[i].cpu().numpy()[0], want)
    assert not np.array_equal(cands[0].cpu().numpy(), cands[1].cpu().numpy())
    assert _recs(recs[0]).tobytes() == _recs(recs[2]).tobytes() == batch["rec"][0:1].tobytes()


@pytest.mark.gpu
def test_queries_and_refused_calls_move_nothing_else(drive):
    import icet_amd
    from icet_amd import api
    from test_keyframe_store import _bytes, _same_bytes
    d = drive
    st, ctx = d["st"], d["ctx"]
    prm = st._params(7, 0)

    def parked():
        out = torch.zeros((1, 48), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        ctx.register_device([_desc(d["scans"][1])], prm, out.data_ptr())
        ctx.sync()
        return out.cpu().numpy()

    def state():
        return [(_bytes(st, s), st.debug_fetch(s, "pose"), st.debug_fetch(s, "stamp")) for s in KF_SLOTS]

    def same(a, b):
        return all(_same_bytes(x[0], y[0]) and x[1].tobytes() == y[1].tobytes() and x[2] == y[2] for x, y in zip(a, b))

    ctx.keyframe_device([_desc(d["kf_scans"][2])], prm)
    before, out_before = state(), parked()
    assert np.isfinite(out_before).all()
    _close(d, [0, 1, 2, 3], 2.6, 4)
    _close(d, [2], 10.0, 8, outputs=False)
    st.candidates(d["live"], d["live_stamps"], 3.0, 5)
    assert same(before, state()) and parked().tobytes() == out_before.tobytes()
    # refused calls change nothing
    for kw in (dict(K=33), dict(radius=float("nan")), dict(radius=-1.0), dict(S=17), dict(K=0), dict(S=0)):
        args = dict(radius=2.6, K=4, S=3); args.update(kw)
        with pytest.raises(icet_amd.IcetError) as e:
            _close(d, [0, 1], **args)
        assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError) as e:                        # another grid than the store's
        rec = torch.zeros((1, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
        st.close_device([_desc(d["scans"][0])], d["live"][:1], d["live_stamps"][:1], api.Params(7, 20, 75, 25, 0.1, 0.1, 0), api.ClosureQuery(2.6, 4, 0, 1, float("inf"), 0, 0), rec.data_ptr())
    assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError) as e:                        # poses and scans differ in number
        st.candidates(d["live"][:2], d["live_stamps"][:3], 3.0, 5)
    assert e.value.status == api.ICET_ERR_BAD_ARG
    ctx.set_option("keep", 1)
    try:
        with pytest.raises(icet_amd.IcetError) as e:
            _close(d, [0], 2.6, 4)
        assert e.value.status == api.ICET_ERR_UNSUPPORTED
    finally:
        ctx.set_option("keep", 0)
    assert same(before, state()) and parked().tobytes() == out_before.tobytes()
