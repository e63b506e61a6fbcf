"""Loop closure by appearance (include/icet_hip.h: icet_keyframe_store_enable_appearance / _describe_device / _set_stamp / _candidates_appearance_device /
_close_appearance_device).  The rule is held to the NumPy model of tests/appearance_model.py: on the host through the header the
kernels compile (tests/cpp/test_appearance.cpp), on the GPU through the calls themselves, bit for bit; the registrations of a query are held to the entries
a caller would otherwise chain by hand.  What the rule is FOR -- finding the revisited place and its yaw without any pose -- is checked on simulated scenes
and on the CPU oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import appearance_model as am
import closure_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icet_keyframe_store_enable_appearance", "icet_keyframe_store_describe_device", "icet_keyframe_store_set_stamp",
               "icet_keyframe_store_candidates_appearance_device", "icet_keyframe_store_close_appearance_device")
P0 = am.Params()
# the bounds of test_loop_closure.py's oracle test, which the issue of this feature takes over
TOL_T, TOL_R = 0.02, 0.035


def test_appearance_entry_points_are_exported_and_refuse_a_null_store():
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    p = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    q = api.ClosureQuery(0.5, 4, 0, 1, float("inf"), 0, 0)
    idx = (C.c_int32 * 1)(0)
    st = np.zeros(1, np.int64)
    assert lib.icet_keyframe_store_enable_appearance(None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_describe_device(None, 0, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_set_stamp(None, 1, idx, st.ctypes.data) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_candidates_appearance_device(None, 1, None, st.ctypes.data, C.byref(q), None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_close_appearance_device(None, C.byref(p), 1, None, st.ctypes.data, C.byref(q), None, None, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert api.LATTICE_STARTS.shape == (9, 6) and not api.LATTICE_STARTS[4].any() and set(np.unique(api.LATTICE_STARTS)) == {np.float32(-0.3), np.float32(0), np.float32(0.3)}


def test_appearance_record_size_matches_the_ctypes_mirror(tmp_path):
    from icet_amd import api
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icet_hip.h"\nint main(void){ printf("%d %d %d %d\\n", (int)sizeof(icet_appearance_params), '
                   '(int)offsetof(icet_appearance_params, rho_max), (int)offsetof(icet_appearance_params, z_hi), (int)offsetof(icet_appearance_params, reserved)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
    assert got == [C.sizeof(api.AppearanceParams), api.AppearanceParams.rho_max.offset, api.AppearanceParams.z_hi.offset, api.AppearanceParams.reserved.offset]
    assert got[0] == 32


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    """tests/cpp/test_appearance.cpp: icet_appearance.h compiled for the host, nothing contracted."""
    exe = str(tmp_path_factory.mktemp("appearance") / "test_appearance")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_appearance.cpp"), "-o", exe])
    return exe


def _run(exe, mode, P, arr, out_dtype, tmp):
    fin, fout = os.path.join(tmp, mode + ".in"), os.path.join(tmp, mode + ".out")
    cmd = [exe, mode] + P.args()
    if arr is not None:
        open(fin, "wb").write(arr if isinstance(arr, bytes) else np.ascontiguousarray(arr).tobytes())
        cmd.append(fin)
    subprocess.check_call(cmd + [fout])
    return np.fromfile(fout, out_dtype)


PARAM_SETS = [am.Params(), am.Params(60, 20), am.Params(8, 1, 10.0, 0.0, 1.0), am.Params(360, 64, 120.0, -5.0, 25.0), am.Params(90, 7, 55.5, -2.25, 7.75)]


def _edge_points(P, rs):
    """Points on and next to everything the cell rule has an edge at."""
    pts = []
    for r in (1e-3, 0.5, 3.0, float(P.rho_max) / P.Rn, float(P.rho_max) / 2, float(P.rho_max), np.nextafter(P.rho_max, np.float32(0)), float(P.rho_max) * 1.5, 1e20, 1e-30):
        for a in np.concatenate([np.arange(P.A + 1) * (2 * np.pi / P.A) - np.pi, [np.pi, -np.pi, 0.0, np.pi / 2, -np.pi / 2]]):
            for da in (0.0, 1e-7, -1e-7):
                pts.append((r * np.cos(a + da), r * np.sin(a + da), rs.uniform(-5, 15)))
    pts = np.array(pts, np.float32)
    special = np.array([(-1, 0, 0), (-1, -0.0, 0), (-3, 1e-30, 1), (-3, -1e-30, 1), (0, 0, 0), (-0.0, 0.0, 1), (0, -0.0, -0.0), (0, 1, 0), (0, -1, 0), (1, 0, 0),
                        (np.nan, 1, 1), (1, np.nan, 1), (1, 1, np.nan), (np.inf, 1, 1), (1, -np.inf, 1), (1, 1, np.inf), (1, 1, -np.inf), (1e25, 1e25, 0), (1e-25, 1e-25, 0),
                        (2, 2, float(P.z_lo)), (2, 2, float(P.z_hi)), (2, 2, np.nextafter(P.z_lo, np.float32(-100))), (2, 2, np.nextafter(P.z_hi, np.float32(100))),
                        (2, 2, -1e9), (2, 2, 1e9), (2, 2, np.nextafter(P.z_hi, np.float32(-100)))], np.float32)
    ring_edges = np.array([(k * float(P.rho_max) / P.Rn, 0, 0) for k in range(P.Rn + 2)], np.float32)
    return np.concatenate([pts, special, ring_edges, -ring_edges])


def test_header_constants_cells_and_codes_equal_the_model(rule_exe, tmp_path):
    assert subprocess.check_output([rule_exe, "self"]).strip().endswith(b"self ok")
    rs = np.random.RandomState(11)
    for P in PARAM_SETS:
        k = _run(rule_exe, "consts", P, None, np.float32, str(tmp_path))
        assert k.tobytes() == np.array([P.kr, P.ka, P.kz], np.float32).tobytes()
        rnd = np.concatenate([rs.uniform(-1.2, 1.2, (100000, 2)) * float(P.rho_max), rs.uniform(float(P.z_lo) - 2, float(P.z_hi) + 2, (100000, 1))], 1).astype(np.float32)
        pts = np.concatenate([rnd, _edge_points(P, rs)])
        got = _run(rule_exe, "cells", P, pts, np.int32, str(tmp_path)).reshape(-1, 4)
        ok, ring, sec, q = am.cells(P, pts)
        want = np.stack([ok.astype(np.int64), ring, sec, q], 1)
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (P.args(), pts[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert ok.sum() > 50000 and (~ok).sum() > 1000
        assert (ring[ok] < P.Rn).all() and (sec[ok] < P.A).all() and (q[ok] >= 1).all() and (q[ok] <= 255).all()
        assert set(np.unique(sec[ok])) == set(range(P.A)) and set(np.unique(ring[ok])) == set(range(P.Rn))
    # az = +-pi: sector 0 both; an exact-zero row does not count; z outside [z_lo, z_hi] takes the end codes
    ok, ring, sec, q = am.cells(P0, np.array([(-1, 0.0, 0), (-1, -0.0, 0), (0, 0, 5), (2, 2, -100), (2, 2, 100), (80, 0, 0)], np.float32))
    assert list(ok) == [True, True, False, True, True, False] and sec[0] == 0 and sec[1] == 0 and q[3] == 1 and q[4] in (254, 255)       # (15 m x fl(254 / 15) rounds to 254 or just below it)


def _random_descriptor(rs, P, fill, empty_cols=0):
    D = (rs.randint(1, 256, (P.Rn, P.A)) * (rs.uniform(size=(P.Rn, P.A)) < fill)).astype(np.uint8)
    if empty_cols:
        D[:, rs.choice(P.A, empty_cols, replace=False)] = 0
    return D


def test_header_weights_distances_and_shifts_equal_the_model(rule_exe, tmp_path):
    rs = np.random.RandomState(12)
    for P in (am.Params(), am.Params(60, 20), am.Params(8, 1, 10.0, 0.0, 1.0), am.Params(90, 7, 55.5, -2.25, 7.75), am.Params(36, 64)):
        pairs = []
        for i in range(24):
            fill = [1.0, 0.6, 0.3, 0.05][i % 4]
            Dq = _random_descriptor(rs, P, fill, empty_cols=[0, P.A // 3, (3 * P.A) // 4 + 1, P.A - 1][(i // 4) % 4])
            Dc = _random_descriptor(rs, P, fill, empty_cols=[0, P.A // 5, P.A // 2, 0][(i // 8) % 4])
            if i == 5: Dc = np.roll(Dq, 3, axis=1)
            if i == 6: Dc = Dq.copy()
            if i == 7: Dq[:] = 0
            if i == 9: Dq[:] = 255; Dc[:] = 255                        # every shift ties at distance 0: shift 0
            pairs.append((Dq, Dc))
        D_all = np.stack([d for pr in pairs for d in pr])
        w = _run(rule_exe, "weights", P, D_all, np.float32, str(tmp_path)).reshape(-1, P.A)
        assert w.tobytes() == np.stack([am.weights(d) for d in D_all]).tobytes()
        rec = b"".join(Dq.tobytes() + Dc.tobytes() + am.weights(Dq).tobytes() + am.weights(Dc).tobytes() for Dq, Dc in pairs)
        got = _run(rule_exe, "dist", P, rec, np.dtype([("d", "<f4"), ("s", "<i4")]), str(tmp_path))
        seen_inf = seen_fin = 0
        for i, (Dq, Dc) in enumerate(pairs):
            d, s = am.distance(Dq, am.weights(Dq), Dc, am.weights(Dc))
            assert got[i]["d"].tobytes() == np.float32(d).tobytes() and got[i]["s"] == s, (P.args(), i, got[i], d, s)
            seen_inf += int(np.isinf(d)); seen_fin += int(np.isfinite(d))
        assert seen_inf >= 2 and seen_fin >= 10                          # the m < ceil(A / 4) case and the ordinary one both occur
        if P.Rn == 1:                                                    # (one ring: every pair of non-empty columns has cosine 1, so shifts tie)
            continue
        assert got[5]["s"] == 3 and got[6]["s"] == 0 and got[6]["d"] <= 1e-6 and np.isinf(got[7]["d"]) and got[9]["s"] == 0 and got[9]["d"] <= 1e-6


def test_a_rolled_descriptor_has_its_best_shift_at_the_roll_and_every_shift_its_yaw(rule_exe, tmp_path):
    rs = np.random.RandomState(13)
    for P in (am.Params(), am.Params(60, 20), am.Params(8, 3, 10.0, 0.0, 1.0), am.Params(360, 4)):
        D = _random_descriptor(rs, P, 0.5, empty_cols=P.A // 6)
        shifts = sorted(set([0, 1, P.A // 2, P.A - 1] + list(rs.randint(0, P.A, 4))))
        rec = b"".join(D.tobytes() + np.roll(D, s, axis=1).tobytes() + am.weights(D).tobytes() + am.weights(np.roll(D, s, axis=1)).tobytes() for s in shifts)
        got = _run(rule_exe, "dist", P, rec, np.dtype([("d", "<f4"), ("s", "<i4")]), str(tmp_path))
        assert list(got["s"]) == shifts and (got["d"] <= 1e-6).all()
        for s in shifts:
            assert am.distance(D, am.weights(D), np.roll(D, s, axis=1), am.weights(np.roll(D, s, axis=1)))[1] == s
        yaw = _run(rule_exe, "yaw", P, None, np.float32, str(tmp_path))
        want = np.array([am.shift_yaw(s, P.A) for s in range(P.A)], np.float32)
        assert yaw.tobytes() == want.tobytes()
        assert yaw[0] == 0 and yaw[P.A // 2] == np.float32(np.pi) and (yaw[P.A // 2 + 1:] < 0).all() and (np.diff(yaw[:P.A // 2 + 1]) > 0).all()
        assert np.abs(np.diff(yaw[P.A // 2 + 1:]) - 2 * np.pi / P.A).max() < 1e-6


def _scan(scene, T, seed):
    from icet_amd import lidar_sim as ls
    return np.ascontiguousarray(ls.make_scan(scene, (T[:3, 3].astype(np.float64), T[:3, :3].astype(np.float64)), seed).numpy().T)


def _wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def test_place_and_yaw_are_found_among_twelve_scenes():
    """12 scenes, one keyframe each at a random yaw, each revisited 0 - 0.6 m away at a yaw difference of up to +-3 rad: the right keyframe is the nearest
    descriptor every time, and the best shift gives the yaw of the start pose to within one sector."""
    from icet_amd import lidar_sim as ls
    rs = np.random.RandomState(5)
    kfs, lives, truth = [], [], []
    for k in range(12):
        scene = ls.make_scene(2000 + k)
        yaw = rs.uniform(-np.pi, np.pi)
        r, phi, dyaw = rs.uniform(0.0, 0.6), rs.uniform(-np.pi, np.pi), rs.uniform(-3.0, 3.0)
        Tk = cm.pose_yaw((0.0, 0.0, 0.0), yaw); Tl = cm.pose_yaw((r * np.cos(phi), r * np.sin(phi), 0.0), yaw + dyaw)
        kfs.append(am.descriptor(P0, _scan(scene, Tk, 300 + k))); lives.append(am.descriptor(P0, _scan(scene, Tl, 400 + k)))
        truth.append(cm.start_pose64(Tl, Tk)[5])
    worst_yaw, worst_ratio = 0.0, np.inf
    for k in range(12):
        ds = [am.distance(lives[k][0], lives[k][1], D, w) for D, w in kfs]
        d = np.array([x[0] for x in ds])
        order = np.argsort(d, kind="stable")
        err = abs(_wrap(float(am.shift_yaw(ds[k][1], P0.A)) - truth[k]))
        print("scene %d: rank of the right keyframe %d, d %.4f, runner-up %.4f, yaw %.3f (true %.3f, error %.4f)" % (2000 + k, list(order).index(k), d[k], d[order[1]],
                                                                                                              am.shift_yaw(ds[k][1], P0.A), truth[k], err))
        assert order[0] == k
        worst_yaw = max(worst_yaw, err); worst_ratio = min(worst_ratio, d[order[1]] / d[k])
        assert err <= 2 * np.pi / P0.A
    print("worst yaw error %.4f rad (one sector: %.4f), runner-up at least %.2f x the winner" % (worst_yaw, 2 * np.pi / P0.A, worst_ratio))


KF_SLOTS = [3, 0, 9, 5, 12, 7, 1, 14]                                   # the drive of tests/test_loop_closure.py
DISTRACTOR_SLOTS = [2, 4, 6, 8, 10, 11, 13, 15]
NEAR = [1, 3, 5, 7]
# per revisit, a lattice start (row of api.LATTICE_STARTS) from which the CPU oracle ends within TOL_T / TOL_R of the truth: test_oracle_converges_... asserts it
ORACLE_STARTS = [7, 3, 6, 3]


@pytest.fixture(scope="module")
def drive_scans():
    """The drive of tests/test_loop_closure.py on the host: 8 keyframes 1.5 m apart in scene 2000, 4 revisits 0.3 - 0.6 m and 0.2 - 0.5 rad of yaw from their nearest
    keyframe; 8 keyframes of scenes 2001 - 2008 as distractors.  No pose is stored anywhere: the true poses only say what the answer is."""
    from icet_amd import lidar_sim as ls
    scene = ls.make_scene(2000)
    true_kf = [cm.pose_yaw((-5.0 + 1.5 * k, -1.0 + 0.1 * k, 0.0), 0.05 * k) for k in range(8)]
    off = [(0.35, 0.20, 0.30), (-0.30, 0.30, 0.45), (0.25, -0.35, -0.25), (0.40, 0.10, 0.20)]
    live = [cm.pose_yaw((true_kf[k][0, 3] + o[0], true_kf[k][1, 3] + o[1], 0.0), 0.05 * k + o[2]) for k, o in zip(NEAR, off)]
    kf_scans = [_scan(scene, T, 100 + k) for k, T in enumerate(true_kf)]
    live_scans = [_scan(scene, T, 200 + i) for i, T in enumerate(live)]
    distractors = [_scan(ls.make_scene(2001 + k), cm.pose_yaw((0.0, 0.0, 0.0), 0.0), 500 + k) for k in range(8)]
    truth = [cm.start_pose(live[i], true_kf[k]) for i, k in enumerate(NEAR)]
    return dict(kf=kf_scans, live=live_scans, distractors=distractors, truth=np.stack(truth), near=[KF_SLOTS[k] for k in NEAR])


def _drive_book(d, P):
    book = {}
    for slot, s in zip(KF_SLOTS + DISTRACTOR_SLOTS, d["kf"] + d["distractors"]):
        book[slot] = am.descriptor(P, s) + (-1,)
    return book


def test_drive_the_nearest_keyframe_ranks_first(drive_scans):
    d = drive_scans
    for P in (am.Params(), am.Params(60, 20)):
        book = _drive_book(d, P)
        for i, s in enumerate(d["live"]):
            Dq, wq = am.descriptor(P, s)
            cand, dist, shift, x0 = am.candidates(Dq, wq, book, 0, np.inf, 16)
            err = abs(_wrap(float(x0[0, 5]) - float(d["truth"][i, 5])))
            print("A = %d, revisit %d: first %s, distances %s, yaw error %.4f" % (P.A, i, cand[:3], dist[:3], err))
            assert cand[0] == d["near"][i] and (cand >= 0).all()
            assert len(set(dist.tolist())) == 16                         # the distance never ties
            assert err <= 2 * np.pi / P.A


def _oracle_converging(d, i):
    from icet_amd import api
    from oracle import pyoracle as po
    Dq, wq = am.descriptor(P0, d["live"][i])
    D, w = am.descriptor(P0, d["kf"][NEAR[i]])
    yaw = am.shift_yaw(am.distance(Dq, wq, D, w)[1], P0.A)
    good = []
    for s, off in enumerate(api.LATTICE_STARTS):
        x0 = (np.array([0, 0, 0, 0, 0, yaw], np.float32) + off).astype(np.float32)
        r = po.solve(d["kf"][NEAR[i]], d["live"][i], x0=x0, runlen=7, bins_phi=24, bins_theta=75)
        dt, dr = np.abs(r["X"][:3] - d["truth"][i, :3]).max(), np.abs(r["X"][3:] - d["truth"][i, 3:]).max()
        print("    revisit %d start %d: |dt| %.4f m |dr| %.4f rad" % (i, s, dt, dr))
        if dt <= TOL_T and dr <= TOL_R:
            good.append((s, float(dt)))
    return good


def test_oracle_converges_from_the_shift_yaw_and_the_lattice_of_starts(drive_scans):
    """End to end on the CPU oracle, no pose used anywhere: X0 = (0, 0, 0, 0, 0, yaw of the shift) plus the 3 x 3 lattice; every revisit has at least one start that
    ends within 0.02 m / 0.035 rad of the truth at runlen 7 (36 oracle solves)."""
    for i in range(4):
        good = _oracle_converging(drive_scans, i)
        print("revisit %d: converging starts %s, best |dt| %.4f m" % (i, [g[0] for g in good], min([g[1] for g in good] or [np.nan])))
        assert len(good) >= 1
        assert ORACLE_STARTS[i] in [g[0] for g in good]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

DEV = torch.device("cuda", 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).to(DEV)


def _desc(t, n=None):
    return (t.data_ptr(), t.shape[1] if n is None else int(n), t.shape[1])


def _describe(st, tensors, P, rows=None, ns=None):
    n = len(tensors)
    D = torch.full((n, P.Rn, P.A), 77, dtype=torch.uint8, device=DEV); w = torch.full((n, P.A), float("nan"), dtype=torch.float32, device=DEV)
    rows_t = torch.tensor(rows, dtype=torch.int32, device=DEV) if rows is not None else None
    torch.cuda.synchronize()
    st.describe_device([_desc(t, None if ns is None else ns[i]) for i, t in enumerate(tensors)], D.data_ptr(), w.data_ptr(), rows_t.data_ptr() if rows_t is not None else None)
    st._ctx.sync()
    return D.cpu().numpy(), w.cpu().numpy()


def _same_descriptor(got_D, got_w, scan, P):
    D, w = am.descriptor(P, scan)
    return got_D.tobytes() == D.tobytes() and got_w.tobytes() == w.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [am.Params(), am.Params(60, 20), am.Params(360, 64, 120.0, -5.0, 25.0), am.Params(90, 7, 55.5, -2.25, 7.75)], ids=lambda p: "A%d_R%d" % (p.A, p.Rn))
def test_descriptors_equal_the_model_bit_for_bit(frames, sample_pc, P):
    import icet_amd
    import param_sweep
    from icet_amd import lidar_sim as ls
    rng = np.random.default_rng(7)
    sa, sb, _ = ls.make_batch_pair(0)
    scans = [frames[0], frames[1], sample_pc[0], sample_pc[1], np.ascontiguousarray(sa.numpy().T), np.ascontiguousarray(sb.numpy().T)]
    assert (np.abs(sample_pc[0]).sum(1) == 0).sum() > 1000              # the real pair carries thousands of exact-zero rows
    spoiled = []
    for k in range(6):
        o, what = param_sweep.spoil(rng, scans[k % len(scans)])
        spoiled.append(o)
    scans += spoiled + [np.zeros((0, 3), np.float32), np.zeros((50, 3), np.float32), frames[0][:1], frames[0][:300]]
    ctx = icet_amd.Context(0)
    st = icet_amd.KeyframeStore(ctx, 100)
    st.enable_appearance(P.A, P.Rn, float(P.rho_max), float(P.z_lo), float(P.z_hi))
    t = [_dev(s) for s in scans]
    # describe_device, all in one call
    D, w = _describe(st, t, P)
    for i, s in enumerate(scans):
        assert _same_descriptor(D[i], w[i], s, P), i
    assert D[:6].any(axis=(1, 2)).all() and not D[12].any() and not D[13].any() and not w[13].any()
    # put_device: the same bytes through debug_fetch, whatever the batch: every scan alone, and again in one batch into other slots
    big = [i for i, s in enumerate(scans) if s.shape[0] > 0]
    for i in big[:4]:
        st.put_device([i], [_desc(t[i])])
    st.put_device([50 + i for i in big], [_desc(t[i]) for i in big])
    for i in big:
        for slot in ([i] if i in big[:4] else []) + [50 + i]:
            assert _same_descriptor(st.debug_fetch(slot, "descriptor"), st.debug_fetch(slot, "weights"), scans[i], P), (i, slot)
    # ragged d_rows: the device-side count cuts the scan; a count above n or below 0 is clamped
    rows = [1000, 0, 10 ** 9, -5, 70000, 1]
    want_n = [min(max(r, 0), scans[i].shape[0]) for i, r in enumerate(rows)]
    D, w = _describe(st, t[:6], P, rows=rows)
    for i in range(6):
        assert _same_descriptor(D[i], w[i], scans[i][:want_n[i]], P), i
    rows_t = torch.tensor(rows, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st.put_device([90 + i for i in range(6)], [_desc(x) for x in t[:6]], rows_t.data_ptr())
    for i in range(6):
        assert _same_descriptor(st.debug_fetch(90 + i, "descriptor"), st.debug_fetch(90 + i, "weights"), scans[i][:want_n[i]], P), i
    # a padded leading dimension with NaN in the padding (n < ld; ld not a multiple of 4)
    padded = []
    for s in scans[:4]:
        buf = torch.full((3, s.shape[0] + 37), float("nan"), dtype=torch.float32, device=DEV)
        buf[:, :s.shape[0]] = torch.from_numpy(np.ascontiguousarray(s.T)).to(DEV)
        padded.append(buf)
    D, w = _describe(st, padded, P, ns=[s.shape[0] for s in scans[:4]])
    for i in range(4):
        assert _same_descriptor(D[i], w[i], scans[i], P), i
    # one scan alone against the same scan in a batch of 64 (two launches' worth of blocks, other scans around it)
    D64, w64 = _describe(st, [t[(i * 5) % 12] for i in range(64)], P)
    D1, w1 = _describe(st, [t[4]], P)
    for i in range(64):
        if (i * 5) % 12 == 4:
            assert D64[i].tobytes() == D1[0].tobytes() and w64[i].tobytes() == w1[0].tobytes()
        assert _same_descriptor(D64[i], w64[i], scans[(i * 5) % 12], P), i
    D70, w70 = _describe(st, [t[i % 6] for i in range(70)], P)          # more than one batch of 64
    assert all(_same_descriptor(D70[i], w70[i], scans[i % 6], P) for i in (0, 63, 64, 69))
    st.close(); ctx.close()


class _Book:
    """The host's copy of what the store should hold: descriptor, weights and stamp of every slot that has a descriptor."""

    def __init__(self, P):
        self.P, self.slots = P, {}

    def put(self, slots, scans):
        for s, sc in zip(slots, scans):
            self.slots[s] = am.descriptor(self.P, sc) + (-1,)

    def stamp(self, slots, stamps):
        for s, v in zip(slots, stamps):
            self.slots[s] = self.slots[s][:2] + (int(v),)

    def candidates(self, scan, sq, max_distance, k, gap=0):
        Dq, wq = am.descriptor(self.P, scan)
        return am.candidates(Dq, wq, self.slots, sq, max_distance, k, gap)


def _check_search(st, book, scans, k, max_distance, stamps=None, gap=0):
    cand, dist, shift, x0 = st.candidates_by_appearance(scans, k, max_distance, stamps, gap)
    n = []
    for q, s in enumerate(scans):
        wc, wd, ws, wx = book.candidates(s, 0 if stamps is None else stamps[q], max_distance, k, gap)
        assert np.array_equal(cand[q], wc), (q, k, max_distance, gap, cand[q], wc)
        assert dist[q].tobytes() == wd.tobytes() and np.array_equal(shift[q], ws) and x0[q].tobytes() == wx.tobytes(), (q, dist[q], wd, shift[q], ws)
        n.append(int((wc >= 0).sum()))
    return cand, dist, n


@pytest.fixture(scope="module")
def app_drive(drive_scans):
    """The drive in a store of 40 slots with appearance enabled and NO pose anywhere.  Slots 30 and 31 were put before enabling; slot 20 holds the same scan as slot 0."""
    import icet_amd
    d = drive_scans
    ctx = icet_amd.Context(0)
    st = icet_amd.KeyframeStore(ctx, 40)
    st.put([30, 31], [d["kf"][1], d["kf"][3]])
    st.enable_appearance()
    book = _Book(P0)
    slots, scans = KF_SLOTS + DISTRACTOR_SLOTS + [20], d["kf"] + d["distractors"] + [d["kf"][1]]
    st.put(slots, scans); book.put(slots, scans)
    dev = dict(live=[_dev(s) for s in d["live"]])
    torch.cuda.synchronize()
    yield dict(ctx=ctx, st=st, book=book, d=d, dev=dev)
    st.close(); ctx.close()


@pytest.mark.gpu
def test_search_equals_the_model_exactly(app_drive):
    import icet_amd
    from icet_amd import api
    st, book, d = app_drive["st"], app_drive["book"], app_drive["d"]
    live = d["live"]
    # slots put before enabling have no descriptor: never candidates, and no descriptor to fetch
    with pytest.raises(icet_amd.IcetError):
        st.debug_fetch(30, "descriptor")
    for k in (1, 4, 32):                                                # K = 32 is above the 17 eligible slots: -1 behind the last
        cand, dist, n = _check_search(st, book, live, k, np.inf)
        assert 30 not in cand and 31 not in cand
        if k == 32:
            assert n == [17] * 4 and (cand[:, 17:] == -1).all() and np.isinf(dist[:, 17:]).all()
    # the same scan in slots 0 and 20: the tie goes to the lower slot
    cand, dist, _ = _check_search(st, book, [live[0]], 4, np.inf)
    assert list(cand[0][:2]) == [0, 20] and dist[0][0].tobytes() == dist[0][1].tobytes()
    assert cand[0][0] == d["near"][0]
    # a keyframe's own scan: distance 0 at shift 0
    cand, dist, _ = _check_search(st, book, [d["kf"][4]], 2, np.inf)
    assert cand[0][0] == KF_SLOTS[4] and dist[0][0] <= 1e-6
    # Q = 8, and Q = 1 gives the same rows
    eight = live + [d["kf"][2], d["distractors"][5], d["kf"][7], live[1]]
    c8, d8, _ = _check_search(st, book, eight, 5, np.inf)
    for q in (0, 5, 7):
        c1, d1, _ = _check_search(st, book, [eight[q]], 5, np.inf)
        assert np.array_equal(c1[0], c8[q]) and d1[0].tobytes() == d8[q].tobytes()
    # max_distance: exactly the third distance is in, the float below it is not
    _, dist, _ = _check_search(st, book, [live[2]], 8, np.inf)
    edge = np.float32(dist[0][2])
    assert _check_search(st, book, [live[2]], 8, float(edge))[2] == [3]
    assert _check_search(st, book, [live[2]], 8, float(np.nextafter(edge, np.float32(0))))[2] == [2]
    assert _check_search(st, book, [live[2]], 8, 0.0)[2] == [0]
    # stamps without poses: the frames just behind the vehicle are not revisits
    slots = KF_SLOTS + DISTRACTOR_SLOTS
    stamps = [10 * i for i in range(len(slots))]
    st.set_stamp(slots, stamps); book.stamp(slots, stamps)
    assert st.debug_fetch(KF_SLOTS[2], "stamp") == 20 and np.isnan(st.debug_fetch(KF_SLOTS[2], "pose")[:3, 3]).all() and st.debug_fetch(20, "stamp") == -1
    seen = set()
    for gap in (0, 15, 60, 1000):
        _, _, n = _check_search(st, book, live, 6, np.inf, stamps=[75, 30, 0, 155], gap=gap)
        seen.update(n)
    assert 0 in seen and 6 in seen and len(seen) >= 3
    # two consecutive calls of one shape with other scans, nothing waited for in between
    K = 4
    bufs = [torch.full((1, K), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    dists = [torch.zeros((1, K), dtype=torch.float32, device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    order = [0, 2, 0]
    for i, q in enumerate(order):
        st.candidates_appearance_device([_desc(app_drive["dev"]["live"][q])], None, api.ClosureQuery(float("inf"), K, 0, 1, float("inf"), 0, 0), bufs[i].data_ptr(), dists[i].data_ptr())
    app_drive["ctx"].sync()
    for i, q in enumerate(order):
        wc, wd, _, _ = book.candidates(live[q], 0, np.inf, K)
        assert np.array_equal(bufs[i].cpu().numpy()[0], wc) and dists[i].cpu().numpy()[0].tobytes() == wd.tobytes()
    assert not np.array_equal(bufs[0].cpu().numpy(), bufs[1].cpu().numpy())
    # a put replaces a stamped slot: its stamp is gone and its descriptor is the new scan's
    st.put([KF_SLOTS[0]], [d["distractors"][0]]); book.put([KF_SLOTS[0]], [d["distractors"][0]])
    assert st.debug_fetch(KF_SLOTS[0], "stamp") == -1
    _check_search(st, book, live[:2], 6, np.inf, stamps=[75, 30], gap=15)
    st.put([KF_SLOTS[0]], [d["kf"][0]]); book.put([KF_SLOTS[0]], [d["kf"][0]])
    st.set_stamp([KF_SLOTS[0]], [0]); book.stamp([KF_SLOTS[0]], [0])


def _recs(t):
    from icet_amd import api
    return np.frombuffer(t.cpu().numpy().tobytes(), api.CLOSURE_DTYPE).copy()


def _scores(t):
    from icet_amd import api
    return np.frombuffer(t.cpu().numpy().tobytes(), api.SCORE_DTYPE).copy()


def _close(a, qs, K, S, max_distance=np.inf, outputs=True, flags=0, max_chi2=float("inf"), min_voxels=0, stamps=None, gap=0, runlen=7):
    from icet_amd import api
    st = a["st"]
    Q, R = len(qs), len(qs) * K * S
    rec = torch.zeros((Q, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    cand = torch.full((Q, K), -7, dtype=torch.int32, device=DEV)
    x0 = torch.full((R, 6), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((R, 48), float("nan"), dtype=torch.float32, device=DEV)
    sc = torch.zeros((R, 8), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    query = api.ClosureQuery(float(max_distance), K, gap, S, float(max_chi2), int(min_voxels), 0)
    ptr = (lambda t: t.data_ptr()) if outputs else (lambda t: None)
    st.close_appearance_device([_desc(a["dev"]["live"][q]) for q in qs], stamps, st._params(runlen, flags), query, rec.data_ptr(), api.LATTICE_STARTS[:S],
                               ptr(cand), ptr(x0), ptr(out), ptr(sc))
    a["ctx"].sync()
    return dict(rec=_recs(rec), cand=cand.cpu().numpy(), x0=x0.cpu().numpy(), out=out.cpu().numpy(), score=_scores(sc), x0_dev=x0)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [None, "ROUNDTRIP_SCAN2", "DOUBLE_W"])
def test_query_carries_the_bits_of_the_manual_path(app_drive, flag):
    """close_appearance_device against what a caller would chain by hand: the model's candidates and starts, register_scored_device, icet_select_best_device, the gate."""
    from icet_amd import api
    a = app_drive
    st, ctx, book, d = a["st"], a["ctx"], a["book"], a["d"]
    fl = 0 if flag is None else getattr(api, "FLAG_" + flag)
    qs, S = [0, 1, 2, 3], 3
    plain = None
    for K, max_distance in ((4, np.inf), (6, None)):
        if max_distance is None:                                        # a bound that leaves some queries fewer than K candidates: padding registrations in the call
            max_distance = float(np.sort(book.candidates(d["live"][0], 0, np.inf, 32)[1])[3])
        res = _close(a, qs, K, S, max_distance, flags=fl)
        rec, cand = res["rec"], res["cand"]
        want_x0 = np.zeros((len(qs) * K * S, 6), np.float32)
        model = []
        for i, q in enumerate(qs):
            wc, wd, ws, wx = book.candidates(d["live"][q], 0, max_distance, K)
            model.append((wc, wd, ws))
            assert np.array_equal(cand[i], wc)
            for k in range(K):
                for s in range(S):
                    if wc[k] >= 0:
                        want_x0[(i * K + k) * S + s] = wx[k] + api.LATTICE_STARTS[s]
        assert res["x0"].tobytes() == want_x0.tobytes()
        if K == 6:
            assert (cand < 0).any() and (cand >= 0).any()
        live = [r for r in range(len(qs) * K * S) if cand.reshape(-1)[r // S] >= 0]
        slots = [int(cand.reshape(-1)[r // S]) for r in live]
        descs = [_desc(a["dev"]["live"][qs[r // (K * S)]]) for r in live]
        xl = torch.from_numpy(want_x0[live]).to(DEV)
        out2 = torch.zeros((len(live), 48), dtype=torch.float32, device=DEV); sc2 = torch.zeros((len(live), 8), dtype=torch.int32, device=DEV)
        best = torch.full((len(qs),), -9, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        st.register_scored_device(slots, descs, st._params(7, fl), out2.data_ptr(), sc2.data_ptr(), xl.data_ptr())
        group = np.array([r // (K * S) for r in live], np.int32)
        ctx.select_best_device(group, len(qs), sc2.data_ptr(), best.data_ptr())
        ctx.sync()
        out2, sc2, best = out2.cpu().numpy(), _scores(sc2), best.cpu().numpy()
        assert np.array_equal(out2.view(np.uint32), res["out"][live].view(np.uint32)) and sc2.tobytes() == res["score"][live].tobytes()
        pad = [r for r in range(len(qs) * K * S) if r not in live]
        assert (res["score"]["voxels"][pad] == 0).all()
        want = np.zeros(len(qs), api.CLOSURE_DTYPE)
        for i in range(len(qs)):
            wc, wd, ws = model[i]
            want[i]["n_candidates"] = int((wc >= 0).sum())
            b = int(best[i])
            if b < 0:
                want[i]["slot"] = -1; want[i]["reg"] = -1
                continue
            r = live[b]; k = (r // S) % K
            want[i]["slot"] = wc[k]; want[i]["reg"] = r; want[i]["stamp"] = book.slots[int(wc[k])][2]; want[i]["d2"] = wd[k]; want[i]["reserved0"] = ws[k]
            want[i]["x0"] = want_x0[r]; want[i]["out"] = out2[b]; want[i]["score"] = sc2[b]
            want[i]["accepted"] = 1
        assert (want["slot"] >= 0).all()
        assert rec.tobytes() == want.tobytes(), [(n, rec[n], want[n]) for n in rec.dtype.names if rec[n].tobytes() != want[n].tobytes()]
        # the same records when the store uses buffers of its own
        assert _close(a, qs, K, S, max_distance, outputs=False, flags=fl)["rec"].tobytes() == rec.tobytes()
        if K == 4:
            plain = res
    # the gate, on the records of the first call
    base = plain["rec"]
    chi, vox = np.float32(base[0]["score"]["chi2_per_voxel"]), int(base[0]["score"]["voxels"])
    for max_chi2, min_voxels, acc in ((np.nextafter(chi, np.float32(-np.inf)), 0, 0), (chi, vox, 1), (float("inf"), vox + 1, 0)):
        r = _close(a, qs, 4, S, flags=fl, max_chi2=max_chi2, min_voxels=min_voxels)["rec"]
        assert r[0]["accepted"] == acc
        x, y = r[0].copy(), base[0].copy(); x["accepted"] = 0; y["accepted"] = 0
        assert x.tobytes() == y.tobytes()
    if flag == "ROUNDTRIP_SCAN2":
        assert _close(a, qs, 4, S)["out"].tobytes() != plain["out"].tobytes()       # (the flag did reach the loop)
    if flag is None:
        got = st.find_closures_by_appearance(d["live"], 7, 4, starts=api.LATTICE_STARTS[:S])
        for i in range(4):
            assert got[i]["slot"] == int(base[i]["slot"]) and got[i]["accepted"] and np.array_equal(got[i]["X"], base[i]["out"][:6]) and got[i]["shift"] == int(base[i]["reserved0"])


@pytest.mark.gpu
def test_drive_closes_without_any_pose(app_drive, tmp_path):
    """No pose set anywhere, K = 4, S = 9: the registration of each revisit against its nearest slot, from a start the CPU oracle converges from, ends within
    0.02 m / 0.035 rad of the truth.  Which slot WINS each query is printed and written to $ICET_TEST_OUT_DIR/appearance_drive_winners.txt, not asserted: a neighbouring keyframe 1.5 m away may legitimately score better."""
    a = app_drive
    d = a["d"]
    K, S = 4, 9
    res = _close(a, [0, 1, 2, 3], K, S)
    lines = []
    for i in range(4):
        cand = list(res["cand"][i])
        assert d["near"][i] in cand
        k = cand.index(d["near"][i])
        r = (i * K + k) * S + ORACLE_STARTS[i]
        X = res["out"][r][:6]
        dt, dr = np.abs(X[:3] - d["truth"][i, :3]).max(), np.abs(X[3:] - d["truth"][i, 3:]).max()
        rec = res["rec"][i]
        lines.append("revisit %d: candidates %s, nearest slot %d from start %d: |dt| %.4f m |dr| %.4f rad; winner slot %d reg %d (start %d) chi2/voxel %.3f voxels %d distance %.4f shift %d"
                     % (i, cand, d["near"][i], ORACLE_STARTS[i], dt, dr, rec["slot"], rec["reg"], rec["reg"] % S, rec["score"]["chi2_per_voxel"], rec["score"]["voxels"], rec["d2"], rec["reserved0"]))
        print(lines[-1])
    out_dir = os.environ.get("ICET_TEST_OUT_DIR") or str(tmp_path)       # (a run that keeps its output names the directory; otherwise pytest's)
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "appearance_drive_winners.txt"), "w").write("\n".join(lines) + "\n")
    for i in range(4):
        k = list(res["cand"][i]).index(d["near"][i])
        X = res["out"][(i * K + k) * S + ORACLE_STARTS[i]][:6]
        assert np.abs(X[:3] - d["truth"][i, :3]).max() <= TOL_T and np.abs(X[3:] - d["truth"][i, 3:]).max() <= TOL_R


@pytest.mark.gpu
def test_nothing_else_moves(app_drive, frames):
    import icet_amd
    from icet_amd import api
    from test_keyframe_store import _bytes, _same_bytes
    a = app_drive
    st, ctx, d = a["st"], a["ctx"], a["d"]
    prm = st._params(7, 0)
    watched = KF_SLOTS + [20, 30]

    def parked():
        out = torch.zeros((1, 48), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        ctx.register_device([_desc(a["dev"]["live"][1])], prm, out.data_ptr())
        ctx.sync()
        return out.cpu().numpy()

    def state():
        return [(_bytes(st, s), st.debug_fetch(s, "pose"), st.debug_fetch(s, "stamp"),
                 (st.debug_fetch(s, "descriptor"), st.debug_fetch(s, "weights")) if s != 30 else None) for s in watched]

    def same(x, y):
        return all(_same_bytes(p[0], q[0]) and p[1].tobytes() == q[1].tobytes() and p[2] == q[2] and
                   (p[3] is None or (p[3][0].tobytes() == q[3][0].tobytes() and p[3][1].tobytes() == q[3][1].tobytes())) for p, q in zip(x, y))

    kf2 = _dev(d["kf"][2])
    torch.cuda.synchronize()
    ctx.keyframe_device([_desc(kf2)], prm)
    before, out_before = state(), parked()
    assert np.isfinite(out_before).all()
    # queries, describe calls and whole solves leave everything as it was
    _close(a, [0, 1, 2, 3], 4, 3)
    _close(a, [2], 8, 9, outputs=False)
    st.candidates_by_appearance(d["live"], 5, 0.5)
    assert same(before, state()) and parked().tobytes() == out_before.tobytes()
    st.describe([frames[0]])
    ctx.solve(frames[0], frames[1], 3, np.zeros(6, np.float32), 24, 75)
    ctx.keyframe_device([_desc(kf2)], prm)
    assert same(before, state()) and parked().tobytes() == out_before.tobytes()
    # another store's calls (with other appearance parameters), and puts into other slots of this one
    st2 = icet_amd.KeyframeStore(ctx, 8)
    st2.enable_appearance(60, 16)
    st2.put([1, 2], [d["live"][0], d["live"][1]])
    st2.candidates_by_appearance([d["live"][2]], 2, 1.0)
    st2.close()
    st.put([33], [d["live"][3]])
    ctx.keyframe_device([_desc(kf2)], prm)
    assert same(before, state()) and parked().tobytes() == out_before.tobytes()
    assert st.debug_fetch(33, "descriptor").tobytes() == am.descriptor(P0, d["live"][3])[0].tobytes()
    # reserve carries descriptors (and stamps) over; a slot beyond the old capacity gets one; the search sees all of them
    st.reserve(64)
    assert same(before, state())
    st.put([50], [d["live"][2]])
    a["book"].put([33, 50], [d["live"][3], d["live"][2]])
    cand, dist, _ = _check_search(st, a["book"], [d["live"][2], d["live"][3]], 6, np.inf)
    assert cand[0][0] == 50 and cand[1][0] == 33 and dist[0][0] <= 1e-6
    # a put replaces exactly its own slot's descriptor
    st.put([50], [d["kf"][5]]); a["book"].put([50], [d["kf"][5]])
    assert st.debug_fetch(50, "descriptor").tobytes() == am.descriptor(P0, d["kf"][5])[0].tobytes()
    ctx.keyframe_device([_desc(kf2)], prm)
    assert same(before, state())
    # refused calls change nothing
    out_before = parked()
    for kw in (dict(K=33), dict(K=0), dict(S=17), dict(S=0), dict(max_distance=float("nan")), dict(max_distance=-1.0), dict(gap=5)):      # (gap > 0 without stamps)
        args = dict(K=4, S=3); args.update(kw)
        with pytest.raises(icet_amd.IcetError) as e:
            _close(a, [0, 1], **args)
        assert e.value.status == api.ICET_ERR_BAD_ARG
    rec = torch.zeros((1, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    q1 = api.ClosureQuery(1.0, 4, 0, 1, float("inf"), 0, 0)
    with pytest.raises(icet_amd.IcetError) as e:                        # another grid than the store's
        st.close_appearance_device([_desc(a["dev"]["live"][0])], None, api.Params(7, 20, 75, 25, 0.1, 0.1, 0), q1, rec.data_ptr())
    assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError) as e:                        # a bad scan descriptor (n > ld)
        st.close_appearance_device([(a["dev"]["live"][0].data_ptr(), 10, 5)], None, prm, q1, rec.data_ptr())
    assert e.value.status == api.ICET_ERR_BAD_ARG
    for bad in ([34], [1, 1]):                                          # an empty slot, a slot named twice
        with pytest.raises(icet_amd.IcetError) as e:
            st.set_stamp(bad, [0] * len(bad))
        assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError) as e:                        # enabling twice
        st.enable_appearance()
    assert e.value.status == api.ICET_ERR_BAD_ARG
    st3 = icet_amd.KeyframeStore(ctx, 4)
    for kw in (dict(sectors=121), dict(sectors=6), dict(sectors=362), dict(rings=0), dict(rings=65), dict(rho_max=0.0), dict(z_lo=1.0, z_hi=1.0)):
        with pytest.raises(icet_amd.IcetError) as e:
            st3.enable_appearance(**kw)
        assert e.value.status == api.ICET_ERR_BAD_ARG
    for call in (lambda: st3.candidates_by_appearance([d["live"][0]], 2, 1.0), lambda: st3.describe([d["live"][0]]),
                 lambda: st3.close_appearance_device([_desc(a["dev"]["live"][0])], None, prm, q1, rec.data_ptr())):
        with pytest.raises(icet_amd.IcetError) as e:                    # appearance not enabled
            call()
        assert e.value.status == api.ICET_ERR_BAD_ARG
    st3.close()
    ctx.set_option("keep", 1)
    try:
        with pytest.raises(icet_amd.IcetError) as e:
            _close(a, [0], 4, 3)
        assert e.value.status == api.ICET_ERR_UNSUPPORTED
    finally:
        ctx.set_option("keep", 0)
    ctx.keyframe_device([_desc(kf2)], prm)
    assert same(before, state()) and parked().tobytes() == out_before.tobytes()
