"""The node's tail -- map ring, aligned cloud, snail trail, pose chain, quaternion (icet_nodes.hip: ring_add_scan_row, align_row, frame_tail; icet_node_tail.h) --
held to tests/node_tail_model.py at the node's OWN X, so that no solve tolerance stands between the kernels and their model, on a drive that really rotates
(every angle above 5 mrad on every frame whose X survives the guard: a wrong Euler order, a swapped subtract / rotate or a reversed pose product is then more than a hundred times the bound).

The down-sample draw needs no hook: a TWIN node with the same settings and frames but a guard of 1e-6 trips on every frame (X = 0, R = I), so its ring holds the
drawn rows untouched, in the same places -- twin.map()[i] is the raw row of node.map()[i].

CPU: the model against the oracle's node; every named fault of the model leaves its bound by more than a factor of ten; the hook icet_debug_node_tail (the body
frame_tail calls) over 2000 seeded inputs and over every branch of the quaternion; the pure functions in a stand-alone program under address and
undefined-behaviour sanitizers.  GPU: after every push the accessors return the float32 restatement's BITS and lie within the derived bounds of the exact model --
a small ring that wraps, a ring equal to the draw, the second trip of the ring's and of the cloud's grid-stride loop, and the group's launch forms.
"""
import os
import subprocess

import numpy as np
import pytest
import torch   # before libicet_hip.so is loaded: both must share one HIP runtime (torch ships its own libamdhip64)

from tests import node_tail_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTION = (0.30, -0.12, 0.04, 0.02, -0.015, 0.04)
F32 = np.float32


def _drive(n_frames, rings=32, steps=1024, **kw):
    from icet_amd import lidar_sim as ls
    return [np.ascontiguousarray(s.T.numpy()) for s in ls.make_sequence(n_frames, motion=MOTION, rings=rings, steps=steps, **kw)]


def _range_filter(scan, min_range):
    x, y, z = scan[:, 0], scan[:, 1], scan[:, 2]
    d = np.sqrt((x * x + y * y) + z * z)          # float32 throughout, no fused multiply-add in NumPy
    return scan[d > np.float32(min_range)]


def _map_maker_settings(**kw):
    from icet_amd import api
    d = dict(api.MAP_MAKER_NODE); d.update(map_capacity=5000, map_downsample=2000, flags=api.NODE_ALIGNED_CLOUD | api.NODE_SNAIL_TRAIL); d.update(kw)
    return d


def _twin_settings(kw):
    return dict(kw, trans_thresh=1e-6, rot_thresh=1e-6)


def _same_bits(got, want, what):
    got = np.ascontiguousarray(got, F32); want = np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what                          # (which NaN comes out of an operation on a NaN row is not part of the contract)
    bad = tm.bits(got)[~nan] != tm.bits(want)[~nan]
    assert not bad.any(), (what, int(bad.sum()), got[~nan][bad][:4], want[~nan][bad][:4])


class _Held:
    """One stream's outputs held to the two models, frame by frame.  frame() takes what the node and its twin returned for a push and what their accessors return
    after it; bit_exact: the float32 restatement, given the hook's R for the node's X, must give the node's bits (off for the models with a named fault)."""

    def __init__(self, kw, bit_exact, _fault=None):
        from icet_amd import api
        self.cap, self.down = kw["map_capacity"], kw["map_downsample"]
        al, sn = bool(kw.get("flags", 0) & api.NODE_ALIGNED_CLOUD), bool(kw.get("flags", 0) & api.NODE_SNAIL_TRAIL)
        self.exact = tm.ExactTail(self.cap, al, sn, _fault=_fault)
        self.f32 = tm.F32Tail(self.cap, al, sn) if bit_exact else None
        self.pose = np.eye(4, dtype=F32)
        self.twin_map = np.zeros((0, 3), F32)
        self.worst = dict(map=0.0, aligned=0.0, snail=0.0, pose=0.0, quat=0.0)
        self.live_writes = np.zeros(self.cap, np.int64); self.window_writes = np.zeros(self.cap, np.int64)
        self.enforce = _fault is None
        self.n_rotating = self.n_guarded = 0

    def frame(self, res, res_twin, node_map=None, twin_map=None, aligned=None, snail=None, scan=None, x_free=False):
        from icet_amd import api
        if res_twin is not None:
            assert res["n_kept"] == res_twin["n_kept"] and res["map_rows"] == res_twin["map_rows"] and res["solved"] == res_twin["solved"]
        if not res["solved"]:
            assert np.array_equal(res["pose"], self.pose) and (node_map is None or len(node_map) == len(self.twin_map))
            return
        X = res["X"]
        assert res_twin is None or not res_twin["X"].any()             # the twin's guard has tripped (or its solve returned no motion at all): R = I, t = 0
        if res["diverged"]:                                            # the node's own guard (the map maker's 0.3) zeroed this frame's X: the tail runs on, with R = I
            assert not X.any()
            self.n_guarded += 1
        elif not x_free:                                               # the drive rotates: nothing here asks X to be near the motion, only to be far from "no rotation"
            assert (np.abs(X[3:]) > 5e-3).all() and (np.abs(X[:3]) > 0.05).any(), X
            self.n_rotating += 1
        ex, f = self.exact, self.f32
        raw = None
        if self.cap > 0:
            m = min(self.down, res["n_kept"])
            L = len(twin_map)
            assert L == len(node_map) == res["map_rows"] == min(len(self.twin_map) + m, self.cap)
            # the twin's older rows have not moved since the last push: its ring is the draw, untouched
            assert np.array_equal(tm.bits(twin_map[:L - m]), tm.bits(self.twin_map[len(self.twin_map) - (L - m):]))
            raw = twin_map[L - m:]
            self.twin_map = twin_map.copy()
        if f is not None:
            hook = api.debug_node_tail(X, self.pose)
            R = hook["R"]
            assert np.abs(R.astype(tm.LD) - tm.exact_R(X[3:])).max() <= tm.C_R * tm.U
            out = f.frame(X, R, raw, scan)
            _same_bits(hook["Rinv"], f.Ri, "the hook's R^-1 against the restatement")
            _same_bits(res["pose"], f.pose, "pose"); _same_bits(res["quat"], f.quat, "quaternion")
            _same_bits(hook["pose"], f.pose, "the hook's pose"); _same_bits(hook["quat"], f.quat, "the hook's quaternion")
            if self.cap > 0: _same_bits(node_map, f.map(), "map ring")
            if aligned is not None: _same_bits(aligned, out, "aligned cloud")
            if snail is not None: _same_bits(snail, f.snail, "snail trail")
        ex.frame(X, raw, scan)
        r = {}
        if self.cap > 0:
            r["map"] = tm.row_ratio(node_map, ex.map(), ex.map_bound())
            live = np.zeros(self.cap, bool); live[ex.ring.order()] = True
            self.live_writes += live; self.window_writes[ex.ring.last_window] += 1
        if aligned is not None: r["aligned"] = tm.row_ratio(aligned, ex.aligned, ex.aligned_bound)
        if snail is not None:
            assert len(snail) == len(ex.snail) and not snail[-1].any()
            r["snail"] = tm.row_ratio(snail, ex.snail, ex.snail_bound)
        err = np.abs(res["pose"].astype(tm.LD) - ex.pose)
        if self.enforce: assert (err[ex.pose_B == 0] == 0).all()
        r["pose"] = float((err[ex.pose_B > 0] / ex.pose_B[ex.pose_B > 0]).max())
        qe = max(tm.quat_error(res["quat"], ex.quat), abs(float(np.sqrt((res["quat"].astype(np.float64) ** 2).sum())) - 1.0))
        r["quat"] = qe / ex.quat_E
        for k, v in r.items():
            self.worst[k] = max(self.worst[k], v)
            if self.enforce: assert v <= 1.0, (k, v)
        self.pose = res["pose"].copy()
        return r


def _report(what, worst, h=None):
    frames = "" if h is None else " (%d frames rotate, %d zeroed by the guard)" % (h.n_rotating, h.n_guarded)
    print("%s%s: worst error / bound  " % (what, frames) + "  ".join("%s %.3f" % (k, v) for k, v in worst.items()))


ALL = ("map", "aligned", "snail", "pose", "quat")


def _held(worst, keys=ALL):
    """Every array the case has was compared (a ratio of exactly 0 would mean nothing was) and stayed within its bound."""
    return all(0 < worst[k] <= 1.0 for k in keys)


# ================================================================================================ CPU: the oracle's node, the hook, the stand-alone program

@pytest.fixture(scope="module")
def oracle_drive():
    """The 10-frame drive through the oracle's node (map-maker settings, ring of 5000, draw of 2000, aligned cloud and snail trail) and its twin: per frame what a
    _Held.frame() call takes.  Computed once, left unchanged."""
    from oracle import pyoracle as po
    kw = _map_maker_settings()
    seq = _drive(10)
    node, twin = po.Node(**kw), po.Node(**_twin_settings(kw))
    rec = []
    for k, s in enumerate(seq):
        r, rt = node.push(s), twin.push(s)
        rec.append(dict(res=r, res_twin=rt, node_map=node.map(), twin_map=twin.map(), aligned=node.aligned() if k else None, snail=node.snail_trail(),
                        scan=_range_filter(s, kw["min_range"]) if k else s))
    node.close(); twin.close()
    return kw, rec


def _run(kw, rec, bit_exact=False, _fault=None):
    h = _Held(kw, bit_exact, _fault=_fault)
    for f in rec:
        h.frame(**f)
    return h


def test_model_holds_the_oracle_node_on_a_rotating_drive(oracle_drive):
    kw, rec = oracle_drive
    h = _run(kw, rec, bit_exact=True)                                 # (the oracle evaluates the same float expressions over the same C library: its bits too)
    # the ring wraps on the third solved frame with its write window split across the end
    pos = [(2000 * k) % 5000 for k in range(10)]
    assert pos[2] + 2000 > 5000 and rec[3]["res"]["map_rows"] == 5000 and rec[2]["res"]["map_rows"] == 4000
    assert (h.window_writes >= 3).all() and (h.live_writes[:2000] == 9).all()
    _report("oracle node, 10 frames", h.worst, h)
    assert h.n_rotating >= 5
    assert _held(h.worst)


@pytest.mark.parametrize("fault,checks", [("transposed_inverse", ("map", "aligned", "snail")), ("euler_reversed", ("map", "aligned", "snail", "pose")),
                                          ("subtract_then_rotate", ("aligned", "snail")), ("rotate_then_subtract", ("map",)), ("pose_reversed", ("pose", "quat")),
                                          ("window_off_by_one", ("map",)), ("no_wrap", ("map",))])
def test_every_named_fault_leaves_its_bound(oracle_drive, fault, checks):
    """The model with one named fault against the (fault-free) oracle node: more than ten times the bound on at least one row or entry of every check the fault names.
    The faults are applied on every frame; pose_reversed can only show from the second solved frame on (the first pose is the identity)."""
    kw, rec = oracle_drive
    h = _run(kw, rec, _fault=fault)
    _report("fault %s" % fault, h.worst)
    for c in checks:
        assert h.worst[c] > 10.0, (fault, c, h.worst[c])
    untouched = {"subtract_then_rotate": ("map", "pose", "quat"), "rotate_then_subtract": ("aligned", "snail", "pose", "quat"), "pose_reversed": ("map", "aligned", "snail"),
                 "window_off_by_one": ("aligned", "snail", "pose", "quat"), "no_wrap": ("aligned", "snail", "pose", "quat")}
    for c in untouched.get(fault, ()):
        assert h.worst[c] <= 1.0, (fault, c, h.worst[c])           # ... and a fault does not leak into the checks it does not name


def _random_pose(rs):
    q, r = np.linalg.qr(rs.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0: q[:, 0] = -q[:, 0]
    P = np.eye(4); P[:3, :3] = q; P[:3, 3] = rs.uniform(-50, 50, 3)
    return P.astype(F32)


def test_hook_over_seeded_inputs():
    """icet_debug_node_tail -- the body frame_tail calls -- over 2000 seeded X (angles in +-pi, translations in +-50 m) with random orthonormal poses, the drive's
    small angles, X = 0 and single-axis rotations of exactly +-pi/2 and pi: R within its bound of the exact R; R^-1 the restatement's bits given that R and within its
    bound of R^T; the pose the restatement's bits and within its bound of the exact product; the quaternion the restatement's bits."""
    from icet_amd import api
    rs = np.random.RandomState(20261019)
    cases = [(np.concatenate([rs.uniform(-50, 50, 3), rs.uniform(-np.pi, np.pi, 3)]).astype(F32), _random_pose(rs)) for _ in range(2000)]
    eye = np.eye(4, dtype=F32)
    cases += [(np.array(MOTION, F32), eye), (np.array((0.25, 0.02, 0.005, 0.001, -0.001, 0.006), F32), _random_pose(rs)), (np.zeros(6, F32), eye), (np.zeros(6, F32), _random_pose(rs))]
    for axis in range(3):
        for ang in (np.pi / 2, -np.pi / 2, np.pi, -np.pi):
            X = np.zeros(6, F32); X[3 + axis] = F32(ang); X[:3] = (1.0, -2.0, 3.0)
            cases.append((X, _random_pose(rs)))
    worst = dict(R=0.0, Rinv=0.0, pose=0.0)
    for X, P in cases:
        h = api.debug_node_tail(X, P)
        R = tm.exact_R(X[3:])
        worst["R"] = max(worst["R"], float(np.abs(h["R"].astype(tm.LD) - R).max() / (tm.C_R * tm.U)))
        _same_bits(h["Rinv"], tm.inverse3_lu(h["R"]), ("R^-1", X))
        worst["Rinv"] = max(worst["Rinv"], float(np.abs(h["Rinv"].astype(tm.LD) - R.T).max() / (tm.C_RI * tm.U)))
        _same_bits(h["pose"], tm.pose_chain(P, h["R"], X[:3]), ("pose", X))
        H = np.eye(4, dtype=tm.LD); H[:3, :3] = R; H[:3, 3] = X[:3].astype(tm.LD)
        Pe = P.astype(tm.LD); B = tm.pose_bound(Pe, np.zeros((4, 4), tm.LD), H)
        err = np.abs(h["pose"].astype(tm.LD) - Pe @ H)
        assert (err[B == 0] == 0).all()
        worst["pose"] = max(worst["pose"], float((err[B > 0] / B[B > 0]).max()))
        _same_bits(h["quat"], tm.quat_of(h["pose"]), ("quaternion", X))
    _report("hook, %d inputs" % len(cases), worst)
    assert all(0 < v <= 1.0 for v in worst.values())
    # the output pose may be the input pose's own memory, and a missing pointer is refused
    import ctypes as C
    import icet_amd
    L = icet_amd.load_library()
    X, P = cases[0]; want = api.debug_node_tail(X, P)["pose"]
    buf = P.copy().reshape(16); o9a, o9b, o4 = np.zeros(9, F32), np.zeros(9, F32), np.zeros(4, F32)
    assert L.icet_debug_node_tail(X.ctypes.data, buf.ctypes.data, o9a.ctypes.data, o9b.ctypes.data, buf.ctypes.data, o4.ctypes.data) == api.ICET_OK
    assert np.array_equal(tm.bits(buf.reshape(4, 4)), tm.bits(want))
    assert L.icet_debug_node_tail(None, buf.ctypes.data, o9a.ctypes.data, o9b.ctypes.data, buf.ctypes.data, o4.ctypes.data) == api.ICET_ERR_BAD_ARG
    assert L.icet_debug_node_tail(X.ctypes.data, buf.ctypes.data, o9a.ctypes.data, o9b.ctypes.data, buf.ctypes.data, None) == api.ICET_ERR_BAD_ARG
    assert "icet_debug_node_tail" in api.EXPORTED_SYMBOLS


def _axis_angle(axis, ang):
    """Rodrigues' rotation about `axis` by `ang` in longdouble, and its exact quaternion (x, y, z, w)."""
    a = np.asarray(axis, tm.LD); a = a / np.sqrt((a * a).sum()); ang = tm.LD(ang)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], tm.LD)
    R = np.eye(3, dtype=tm.LD) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    return R, np.concatenate([a * np.sin(ang / 2), [np.cos(ang / 2)]])


def test_quaternion_every_branch_and_tie():
    """Rotations by 0, 2.0, 2.2, 3.0 and pi about x, y, z and (1, 1, 1) / sqrt 3, plus three matrices made by hand -- the turn by 120 degrees about (1, 1, 1) (a
    permutation matrix: trace exactly 0 and both ties), the half turns about (1, 1, 0) / sqrt 2 (m11 == m00) and (0, 1, 1) / sqrt 2 (m22 == m[i][i] with i = 1) --
    fed to the hook as poses (X = 0 leaves a pose as it is).  The set reaches all four branches, decided from the float32 pose by the model; the hook's quaternion is
    the restatement's bits, within the derived bound of the exact quaternion up to sign, and its norm within that bound of 1."""
    from icet_amd import api
    poses = []
    s3 = 1 / np.sqrt(tm.LD(3))
    for axis in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (s3, s3, s3)):
        for ang in (0.0, 2.0, 2.2, 3.0, np.pi):
            poses.append(_axis_angle(axis, ang))
    h = np.sqrt(tm.LD(0.5))
    by_hand = [(np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], tm.LD), np.array([0.5, 0.5, 0.5, 0.5], tm.LD)),
               (np.array([[0, 1, 0], [1, 0, 0], [0, 0, -1]], tm.LD), np.array([h, h, 0, 0], tm.LD)),
               (np.array([[-1, 0, 0], [0, 0, 1], [0, 1, 0]], tm.LD), np.array([0, h, h, 0], tm.LD))]
    for R, q in by_hand:                                               # (they are rotations, and the quaternions are theirs)
        assert np.array_equal(R @ R.T, np.eye(3)) and abs(float(np.linalg.det(R.astype(np.float64))) - 1) < 1e-15
    poses += by_hand
    branches, trace0, tie10, tie2i, worst = set(), False, False, False, 0.0
    for k, (R, q) in enumerate(poses):
        P = np.eye(4, dtype=F32); P[:3, :3] = R.astype(F32); P[:3, 3] = (3.0, -4.0, 5.0)
        eps = float(np.abs(P[:3, :3].astype(tm.LD) - R).max())
        assert eps <= tm.U
        out = api.debug_node_tail(np.zeros(6, F32), P)
        assert np.array_equal(out["pose"], P)                        # (numerically: a zero may have changed its sign)
        m = out["pose"]
        b = tm.quat_branch(m); branches.add(b)
        t = (m[0, 0] + m[1, 1]) + m[2, 2]
        trace0 |= bool(t == 0)
        if b != 3:
            tie10 |= bool(m[1, 1] == m[0, 0])
            i = 1 if m[1, 1] > m[0, 0] else 0
            tie2i |= bool(m[2, 2] == m[i, i])
        _same_bits(out["quat"], tm.quat_of(m), ("quaternion", k))
        qh = out["quat"].astype(np.float64)
        E = tm.quat_bound(eps)
        e1, e2 = tm.quat_error(qh, q), tm.quat_error(qh, tm.exact_quat(m))      # the rotation's own quaternion, and the branch-free route on the float32 matrix
        nrm = abs(float(np.sqrt((qh * qh).sum())) - 1.0)
        worst = max(worst, e1 / E, e2 / tm.quat_bound(3 * tm.U), nrm / E)
        assert e1 <= E and e2 <= tm.quat_bound(3 * tm.U) and nrm <= E, (k, b, e1, e2, nrm, E)
    assert branches == {0, 1, 2, 3}, branches
    assert trace0 and tie10 and tie2i
    print("quaternion, %d poses: worst error / bound %.3f" % (len(poses), worst))


def test_node_tail_standalone_under_sanitizers(tmp_path):
    """tests/cpp/test_node_tail.cpp -- icet_node_tail.h alone, degenerate inputs (singular matrices, NaN and inf in X, a pose of zeros) -- built plain and with
    -fsanitize=address,undefined: both run clean and print the same bytes; and the library's compiled body (through the hook) gives the bits the program prints for
    an ordinary X."""
    from icet_amd import api
    src = os.path.join(ROOT, "tests", "cpp", "test_node_tail.cpp")
    outs = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("test_node_tail_" + name))
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", ROOT, src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (name, r.stderr[-2000:])
        outs[name] = r.stdout
    assert outs["plain"] == outs["san"] and outs["plain"].endswith(b"OK\n")
    lines = outs["plain"].decode().splitlines()
    k = lines.index("tail ordinary X, identity pose")
    h = api.debug_node_tail(np.array(MOTION, F32), np.eye(4, dtype=F32))
    for line, key in zip(lines[k + 1:k + 5], ("R", "Rinv", "pose", "quat")):
        words = np.array([int(w, 16) for w in line.split()[1:]], np.uint32)
        assert np.array_equal(words, tm.bits(h[key]).reshape(-1)), (key, line)


# ================================================================================================ GPU: bits and bounds after every push

def _node_frame(h, node, twin, scan, kw, first, **extra):
    from icet_amd import api
    res, rt = node.push(scan), (twin.push(scan) if twin is not None else None)
    fl = kw.get("flags", 0)
    return h.frame(res, rt, node_map=node.map() if kw["map_capacity"] > 0 else None, twin_map=twin.map() if twin is not None else None,
                   aligned=node.aligned() if (fl & api.NODE_ALIGNED_CLOUD) and not first else None,
                   snail=node.snail_trail() if fl & api.NODE_SNAIL_TRAIL else None, scan=node.prev_scan(), **extra)


@pytest.mark.gpu
def test_gpu_small_ring_bits_and_bounds(gpu_ctx):
    """The CPU case on the device: ring of 5000 with a draw of 2000 (wraps on the third solved frame, the write window split across the end), aligned cloud, snail
    trail, pose and quaternion after every one of 10 pushes."""
    from icet_amd import api
    kw = _map_maker_settings()
    node, twin = api.Node(gpu_ctx, **kw), api.Node(gpu_ctx, **_twin_settings(kw))
    h = _Held(kw, bit_exact=True)
    for k, s in enumerate(_drive(10)):
        _node_frame(h, node, twin, s, kw, first=(k == 0))
    assert node.map().shape == (5000, 3) and (h.window_writes >= 3).all() and h.n_rotating >= 5
    node.close(); twin.close()
    _report("gpu small ring", h.worst, h)
    assert _held(h.worst)


@pytest.mark.gpu
def test_gpu_ring_equal_to_the_draw(gpu_ctx):
    """map_capacity = map_downsample = 777 (no multiple of 64): every frame replaces the whole ring.  4 frames."""
    from icet_amd import api
    kw = _map_maker_settings(map_capacity=777, map_downsample=777)
    node, twin = api.Node(gpu_ctx, **kw), api.Node(gpu_ctx, **_twin_settings(kw))
    h = _Held(kw, bit_exact=True)
    for k, s in enumerate(_drive(4)):
        _node_frame(h, node, twin, s, kw, first=(k == 0))
    assert node.map().shape == (777, 3) and (h.window_writes == 3).all() and h.n_rotating >= 2
    node.close(); twin.close()
    _report("gpu ring = draw", h.worst, h)
    assert _held(h.worst)


@pytest.mark.gpu
def test_gpu_ring_second_trip_of_the_grid_stride_loop(gpu_ctx):
    """The ring kernels launch at most 2048 x 256 threads; a ring of 530 000 rows sends rows >= 524 288 through a second trip of the loop.  Three 64 x 2048 frames
    pushed a, b, c, a, b, c, a with runlen 2 and a draw of 110 000 fill the ring and wrap it within the six solved frames; the rows of the second trip are written
    through the window branch in one frame and re-expressed in place in another, and every row of every push is held to bits and bounds."""
    from icet_amd import api
    LAUNCHED = 2048 * 256
    abc = _drive(5, rings=64, steps=2048)[::2]                      # frames 0, 2, 4: two steps (a -> b, b -> c) or four (c -> a) between the frames of a pair, so every angle
    #                                                                 of every pair is at least 0.03 rad and two iterations from X0 = 0 leave it far above the 5 mrad asked below
    kw = dict(api.MAP_MAKER_NODE); kw.update(runlen=2, map_capacity=530000, map_downsample=110000, trans_thresh=0.0, rot_thresh=0.0)      # (no guard: X need not be small)
    kept = [len(_range_filter(s, kw["min_range"])) for s in abc]
    kw["map_downsample"] = min([kw["map_downsample"]] + kept)      # the draw is at most every frame's kept rows
    assert kw["map_capacity"] > LAUNCHED
    node, twin = api.Node(gpu_ctx, **kw), api.Node(gpu_ctx, **_twin_settings(kw))
    h = _Held(kw, bit_exact=True)
    for k in range(7):
        _node_frame(h, node, twin, abc[k % 3], kw, first=(k == 0))
        if k: assert len(node.prev_scan()) == kept[k % 3] >= kw["map_downsample"]
    assert len(node.map()) == 530000 and h.exact.ring.filled and h.n_rotating == 6
    # rows of the second trip: entered through the write window in one frame, re-expressed where they lie in at least one later frame
    assert (h.window_writes[LAUNCHED:] >= 1).all() and (h.live_writes[LAUNCHED:] >= 2).all()
    node.close(); twin.close()
    _report("gpu ring second trip", h.worst, h)
    assert _held(h.worst, ("map", "pose", "quat"))


@pytest.mark.gpu
def test_gpu_aligned_cloud_second_trip(gpu_ctx):
    """One pair of 128 x 4800 frames through the scan-registration node (no range filter, runlen 1): 614 400 rows, so the aligned cloud's rows >= 524 288 take the
    second trip of k_align_cloud's loop.  Two NaN rows, one in each trip, stay NaN; every other row is the restatement's bits and within the bound."""
    from icet_amd import api
    a, b = _drive(2, rings=128, steps=4800)
    far = len(b) - 1000
    assert far > 2048 * 256
    b = b.copy(); b[1000] = (np.nan, 1.0, 2.0); b[far] = (3.0, np.nan, -1.0)
    kw = dict(api.SCAN_REGISTRATION_NODE, runlen=1)
    node = api.Node(gpu_ctx, **kw)
    h = _Held(kw, bit_exact=True)
    _node_frame(h, node, None, a, kw, first=True)
    _node_frame(h, node, None, b, kw, first=False)
    al = node.aligned()
    assert len(node.prev_scan()) == len(b) > 524288                 # n_kept: nothing is filtered
    assert len(al) == len(b) and np.isnan(al[1000]).all() and np.isnan(al[far]).all() and np.isfinite(np.delete(al, (1000, far), axis=0)).all() and h.n_rotating == 1
    assert np.array_equal(tm.bits(node.prev_scan()), tm.bits(b))
    node.close()
    _report("gpu aligned cloud second trip", h.worst, h)
    assert _held(h.worst, ("aligned", "pose", "quat")) and h.worst["snail"] == 0      # (the trail's one old row is 0 * R^-1 - t: exact)


@pytest.mark.gpu
def test_gpu_group_launch_forms_bits_and_bounds(gpu_ctx):
    """k_group_map_add_scan / k_group_align_cloud: a group of 3 streams with the small ring's settings, drives through different scenes, stream 1 left out of the
    third call and stream 2 given an empty frame once; a twin group with the guard tripped beside it.  Every stream's map, aligned cloud, snail trail, pose and
    quaternion go through the small ring's checks after every call."""
    from icet_amd import api, lidar_sim as ls
    S, calls = 3, 7
    kw = _map_maker_settings()
    drives = [[t.to("cuda:0").contiguous() for t in ls.make_sequence(calls, scene_seed=3000 + 11 * s, noise_seed=5000 + 11 * s, motion=MOTION, rings=32, steps=1024)] for s in range(S)]
    empty = torch.zeros((3, 0), dtype=torch.float32, device="cuda:0")
    g, tw = api.NodeGroup(gpu_ctx, S, **kw), api.NodeGroup(gpu_ctx, S, **_twin_settings(kw))
    held = [_Held(kw, bit_exact=True) for _ in range(S)]
    pushed = [0] * S
    near_empty = set()
    for c in range(calls):
        frames = []
        for s in range(S):
            if c == 2 and s == 1: continue
            t = empty if (c == 4 and s == 2) else drives[s][c]
            if c in (4, 5) and s == 2: near_empty.add((c, s))      # the empty frame and the frame registered against it: X is whatever the solve makes of no rows
            n = int(t.shape[1])
            frames.append((s, t.data_ptr() if n else 0, n, n))
        torch.cuda.synchronize()
        rg, rt = g.push_device(frames), tw.push_device(frames)
        for (s, _, n, _), r, r2 in zip(frames, rg, rt):
            first = pushed[s] == 0
            held[s].frame(r, r2, node_map=g.map(s), twin_map=tw.map(s), aligned=g.aligned(s) if not first else None, snail=g.snail_trail(s), scan=g.prev_scan(s),
                          x_free=(c, s) in near_empty)
            pushed[s] += 1
    assert pushed == [calls, calls - 1, calls]
    g.close(); tw.close()
    for s in range(S):
        _report("gpu group, stream %d" % s, held[s].worst, held[s])
        assert _held(held[s].worst) and held[s].n_rotating >= 2
