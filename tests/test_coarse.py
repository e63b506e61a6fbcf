"""Coarse alignment of the keyframe store (include/icet_hip.h: icet_keyframe_store_enable_coarse / _coarse_grid_device / _coarse_align_device /
_close_coarse_device).  The rule is held to the NumPy model of tests/coarse_model.py: on the host through the header the kernels compile
(tests/cpp/test_coarse.cpp), on the GPU through the calls themselves, bit for bit; the registrations of the one-call query are held to the entries a caller
would otherwise chain by hand.  What the rule is FOR -- a start translation (and the right half turn) from which the solver converges -- is checked on
simulated revisits and on the CPU oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import appearance_model as am
import closure_model as cm
import coarse_model as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icet_keyframe_store_enable_coarse", "icet_keyframe_store_coarse_grid_device", "icet_keyframe_store_coarse_align_device",
               "icet_keyframe_store_close_coarse_device")
P0 = co.Params()
A0 = am.Params()
YAW_STEP = np.pi / 120
TOL_T, TOL_R = 0.02, 0.035                                              # the bounds of the oracle tests of test_loop_closure.py and test_appearance.py
START_T, START_R = 0.35, 0.09                                           # how far a coarse start may be from the true start pose
# the revisits of the RandomState(11) set from whose single coarse start the CPU oracle ends within TOL_T / TOL_R: test_oracle_converges_... asserts it
ORACLE_CONVERGING = [2001, 2002, 2003, 2005, 2006, 2007, 2009]


def test_coarse_entry_points_are_exported_and_refuse_a_null_store():
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    p = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    q = api.ClosureQuery(0.5, 4, 0, 1, float("inf"), 0, 0)
    se = api.KeyframeStore.coarse_search()
    assert (se.window, se.n_yaw, se.half_turn, se.min_score) == (12, 1, 1, 1) and se.yaw_step == np.float32(np.pi / 120)
    st = np.zeros(1, np.int64)
    assert lib.icet_keyframe_store_enable_coarse(None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_coarse_grid_device(None, 0, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_coarse_align_device(None, 1, None, None, 1, None, None, C.byref(se), None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_close_coarse_device(None, C.byref(p), 1, None, None, st.ctypes.data, C.byref(q), C.byref(se), None, None, None, None, None, None,
                                                       None) == api.ICET_ERR_BAD_ARG


def test_coarse_record_sizes_match_the_ctypes_mirrors(tmp_path):
    from icet_amd import api
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icet_hip.h"\nint main(void){ printf("%d %d %d %d %d %d %d %d %d\\n", (int)sizeof(icet_coarse_params), '
                   '(int)offsetof(icet_coarse_params, min_span), (int)offsetof(icet_coarse_params, reserved), (int)sizeof(icet_coarse_search), '
                   '(int)offsetof(icet_coarse_search, yaw_step), (int)offsetof(icet_coarse_search, min_score), (int)sizeof(icet_coarse_match), '
                   '(int)offsetof(icet_coarse_match, live_bits), (int)offsetof(icet_coarse_match, found)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
    assert got == [C.sizeof(api.CoarseParams), api.CoarseParams.min_span.offset, api.CoarseParams.reserved.offset, C.sizeof(api.CoarseSearch),
                   api.CoarseSearch.yaw_step.offset, api.CoarseSearch.min_score.offset, C.sizeof(api.CoarseMatch), api.CoarseMatch.live_bits.offset,
                   api.CoarseMatch.found.offset]
    assert got[0] == 32 and got[3] == 32 and got[6] == 32
    assert [api.COARSE_MATCH_DTYPE.fields[n][1] for n in ("live_bits", "found")] == [got[7], got[8]]


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    """tests/cpp/test_coarse.cpp: icet_coarse.h compiled for the host, nothing contracted."""
    exe = str(tmp_path_factory.mktemp("coarse") / "test_coarse")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_coarse.cpp"), "-o", exe])
    return exe


def _run(exe, mode, P, data, tmp):
    fin, fout = os.path.join(tmp, mode + ".in"), os.path.join(tmp, mode + ".out")
    cmd = [exe, mode] + P.args()
    if data is not None:
        open(fin, "wb").write(data if isinstance(data, bytes) else np.ascontiguousarray(data).tobytes())
        cmd.append(fin)
    subprocess.check_call(cmd + [fout])
    return open(fout, "rb").read()


PARAM_SETS = [co.Params(64, 0.5), co.Params(96, 0.4, -2.25, 7.75, 0.3), co.Params(), co.Params(512, 0.125, -5.0, 25.0, 1.0)]


def _edge_points(P, rs):
    """Points on and next to every cell edge, outside the grid, not finite, exact and signed zeros, z on, next to and outside the band."""
    half = P.G // 2
    e = (np.arange(-half - 2, half + 3) * np.float64(P.cell)).astype(np.float32)
    e = np.concatenate([e, np.nextafter(e, np.float32(1e9)), np.nextafter(e, np.float32(-1e9))])
    a = np.stack([e, rs.uniform(-1, 1, e.size) * half * float(P.cell), rs.uniform(-5, 15, e.size)], 1)
    b = a[:, [1, 0, 2]]
    zl, zh = float(P.z_lo), float(P.z_hi)
    special = np.array([(0, 0, 0), (-0.0, 0.0, 1), (0, -0.0, -0.0), (0, 1, 0), (-0.0, 1, 0), (1, 0, 0), (1, -0.0, 0), (1e-30, 1e-30, 0), (1e-20, 0, 0),
                        (np.nan, 1, 1), (1, np.nan, 1), (1, 1, np.nan), (np.inf, 1, 1), (1, -np.inf, 1), (1, 1, np.inf), (1, 1, -np.inf), (1e25, 1, 0), (1, -1e25, 0), (3e38, 3e38, 0),
                        (2, 2, zl), (2, 2, zh), (2, 2, np.nextafter(P.z_lo, np.float32(-100))), (2, 2, np.nextafter(P.z_hi, np.float32(100))), (2, 2, -1e9), (2, 2, 1e9),
                        (2, 2, np.nextafter(P.z_hi, np.float32(-100))), (2, 2, np.nextafter(P.z_lo, np.float32(100)))], np.float32)
    return np.concatenate([a, b, special]).astype(np.float32)


def _structured_points(P, rs, n_cells=300, ground=3000):
    """A small scene: columns of points over random cells (some spanning, some just below the minimum span), and flat ground."""
    half = P.G // 2 * float(P.cell)
    pts = []
    for _ in range(n_cells):
        cx, cy = rs.uniform(-0.9, 0.9, 2) * half
        span = rs.choice([0.0, 0.5, 0.9, 1.0, 1.1, 3.0]) * float(P.min_span)
        z0 = rs.uniform(float(P.z_lo) - 1, float(P.z_hi) - 2)
        k = rs.randint(1, 6)
        pts.append(np.stack([cx + rs.uniform(-0.4, 0.4, k) * float(P.cell), cy + rs.uniform(-0.4, 0.4, k) * float(P.cell), z0 + np.linspace(0, span, k)], 1))
    g = np.stack([rs.uniform(-1.1, 1.1, ground) * half, rs.uniform(-1.1, 1.1, ground) * half, -1.8 + rs.normal(0, 0.02, ground)], 1)
    return np.concatenate(pts + [g]).astype(np.float32)


def test_header_constants_cells_codes_structure_and_grids_equal_the_model(rule_exe, tmp_path):
    assert subprocess.check_output([rule_exe, "self"]).strip().endswith(b"self ok")
    rs = np.random.RandomState(21)
    plain = 0
    for P in PARAM_SETS:
        k = _run(rule_exe, "consts", P, None, str(tmp_path))
        assert k == np.array([P.kc, P.kz], np.float32).tobytes() + np.array([P.span_codes], np.int32).tobytes(), P.args()
        half = P.G // 2 * float(P.cell)
        rnd = np.concatenate([rs.uniform(-1.2, 1.2, (40000, 2)) * half, rs.uniform(float(P.z_lo) - 2, float(P.z_hi) + 2, (40000, 1))], 1).astype(np.float32)
        pts = np.concatenate([rnd, _edge_points(P, rs), _structured_points(P, rs)])
        got = np.frombuffer(_run(rule_exe, "points", P, pts, str(tmp_path)), np.int32).reshape(-1, 5)
        ok, ix, iy, q = co.count_points(P, pts)
        st = co.structure(P, pts)
        want = np.stack([ok.astype(np.int64), ix, iy, q, st.astype(np.int64)], 1)
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (P.args(), pts[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert ok.sum() > 20000 and (~ok).sum() > 1000 and st.sum() > 100
        plain += int((ok & ~st).sum())
        assert (ix[ok] < P.G).all() and (iy[ok] < P.G).all() and (q[ok] >= 0).all() and (q[ok] <= 254).all()
        assert set(np.unique(ix[ok])) == set(range(P.G)) and set(np.unique(iy[ok])) == set(range(P.G))
        grid = np.frombuffer(_run(rule_exe, "grid", P, pts, str(tmp_path)), np.uint32).reshape(P.G, P.W)
        want_grid = co.words(co.keyframe_grid(P, pts))
        assert grid.tobytes() == want_grid.tobytes() and want_grid.any()
        assert co.unwords(want_grid).tobytes() == co.keyframe_grid(P, pts).tobytes()
    assert plain > 10000                                                # counting points that are no structure points occur, too
    # the cell of an edge is the upper one; the first coordinate outside is G / 2 cells away; exact zeros do not count; z outside the band takes the end codes
    ok, ix, iy, q = co.count_points(P0, np.array([(0.25, -0.25, 0), (-32.0, 31.99, 0), (32.0, 0.1, 0), (0.1, -32.01, 0), (0, 0, 5), (-0.0, 0.0, 5), (2, 2, -100), (2, 2, 100)], np.float32))
    assert list(ok) == [True, True, False, False, False, False, True, True] and (ix[0], iy[0]) == (129, 127) and (ix[1], iy[1]) == (0, 255) and q[6] == 0 and q[7] in (253, 254)
    assert P0.span_codes == 9 and float(P0.kc) == 4.0
    # flat ground does not span whatever the sensor height; a wall does
    for h in (-1.8, -0.3, 2.0):
        flat = np.stack([rs.uniform(-20, 20, 5000), rs.uniform(-20, 20, 5000), h + rs.normal(0, 0.02, 5000)], 1).astype(np.float32)
        assert not co.keyframe_grid(P0, flat).any()
    wall = np.stack([np.full(200, 5.1), rs.uniform(-3, 3, 200), rs.uniform(-1.8, 1.0, 200)], 1).astype(np.float32)
    g = co.keyframe_grid(P0, wall)
    assert g.any() and set(np.nonzero(g)[0]) == {148}


def _pose_header(X0, step, ints):
    return np.asarray(X0, np.float32).tobytes() + np.array([step], np.float32).tobytes() + np.array(ints, np.int32).tobytes()


def _moved(pts, X, rs, sigma=0.01):
    """The scan a sensor moved by X (q = R(X)^T (p + X_t), so p = R(X) q - X_t) would see of the points q, with a little noise."""
    R = cm.euler_R(*[np.float64(v) for v in X[3:]])
    p = pts.astype(np.float64) @ R.T - np.asarray(X[:3], np.float64)
    return (p + rs.normal(0, sigma, p.shape)).astype(np.float32)


SEARCH_CASES = [  # (P, X_true, X0 base, window, Y, half_turn, min_score)
    (co.Params(64, 0.5), (1.5, -1.0, 0.0, 0.0, 0.0, 0.3), (0, 0, 0, 0, 0, 0.29), 12, 1, 1, 1),
    (co.Params(64, 0.5), (4.0, 7.5, 0.1, 0.0, 0.0, -0.2), (0.1, 0.2, 0, 0.01, -0.02, -0.21), 32, 0, 0, 1),
    (co.Params(96, 0.4, -2.25, 7.75, 0.3), (-2.0, 3.0, 0.0, 0.02, -0.01, 2.0), (0, 0, 0, 0.02, -0.01, 2.0 - np.pi), 12, 1, 1, 1),
    (co.Params(96, 0.4, -2.25, 7.75, 0.3), (0.1, 0.1, 0.0, 0.0, 0.0, 0.1), (0, 0, 0, 0, 0, 0.1), 0, 0, 0, 1),
    (co.Params(), (2.0, -1.5, 0.0, 0.0, 0.0, -0.4), (0, 0, 0, 0, 0, -0.41), 12, 1, 1, 1),
    (co.Params(), (1.0, 0.5, 0.0, 0.0, 0.0, 0.2), (0, 0, 0, 0, 0, 0.2), 12, 2, 0, 10 ** 6),       # min_score out of reach: found = 0
]


def test_header_transforms_scores_keys_and_start_poses_equal_the_model(rule_exe, tmp_path):
    rs = np.random.RandomState(22)
    seen_f1 = seen_not_found = 0
    for n, (P, Xt, X0, window, Y, half, min_score) in enumerate(SEARCH_CASES):
        kf = _structured_points(P, rs, 250, 2000)
        live = np.concatenate([_moved(kf, Xt, rs), _edge_points(P, rs)[::7]])
        step = np.float32(0.02)
        key = co.keyframe_grid(P, kf)
        # every hypothesis: the float32 rows of M and the live grid, bit for bit
        for h in range(co.n_hypotheses(Y, half)):
            y, f = co.hypothesis_of(h, Y)
            out = _run(rule_exe, "live", P, _pose_header(X0, step, [y, f]) + live.tobytes(), str(tmp_path))
            M = co.hypothesis_rotation(X0, y, f, step).T.astype(np.float32)
            assert out[:24] == M[:2].tobytes(), (n, h)
            lg = co.live_grid(P, live, X0, y, f, step)
            assert out[24:] == co.words(lg).tobytes(), (n, h)
            if h == 0:                                                  # every shift's score and the hypothesis's best key
                sh = _run(rule_exe, "shifts", P, np.array([window, h], np.int32).tobytes() + co.words(lg).tobytes() + co.words(key).tobytes(), str(tmp_path))
                S = co.scores(lg, key, window)
                assert sh[:-8] == S.astype(np.uint32).tobytes(), n
                k, s, a, b = co.best_shift(S, window, h)
                assert int(np.frombuffer(sh[-8:], np.uint64)[0]) == k == co.shift_key(s, a, b, h)
        for has_key in (1, 0):
            out = _run(rule_exe, "search", P, _pose_header(X0, step, [window, Y, half, min_score, has_key]) + co.words(key).tobytes() + live.tobytes(), str(tmp_path))
            rec = np.frombuffer(out[:32], np.int32); x0 = np.frombuffer(out[32:56], np.float32); best = int(np.frombuffer(out[56:], np.uint64)[0])
            m = co.search(P, live, X0, key if has_key else None, window, Y, step, half, min_score)
            assert list(rec) == [m["score"], m["a"], m["b"], m["h"], m["live_bits"], m["key_bits"], m["found"], 0], (n, rec, m)
            assert x0.tobytes() == m["x0"].tobytes(), (n, x0, m["x0"])
            assert best == (co.shift_key(m["score"], m["a"], m["b"], m["h"]) if has_key else 0)
            if not has_key or min_score > 1000:
                assert m["found"] == 0 and x0.tobytes() == np.asarray(X0, np.float32).tobytes()
                seen_not_found += 1
                continue
            # what the rule is for: the start is within a cell or so of the truth, and the half turn is recognised
            y, f = co.hypothesis_of(m["h"], Y)
            seen_f1 += f
            err_t = np.abs(m["x0"][:2] - np.asarray(Xt[:2], np.float32)).max()
            err_r = abs((float(m["x0"][5]) - Xt[5] + np.pi) % (2 * np.pi) - np.pi)
            print("case %d: %s -> start %s, score %d of %d live bits" % (n, m, m["x0"], m["score"], m["live_bits"]))
            assert m["found"] == 1 and 0 < m["score"] <= min(m["live_bits"], m["key_bits"])
            # (the shift is whole cells in a frame turned by up to half a yaw step: half a cell per axis, and as much again for the turn and the noise; the yaw is
            # one of the hypotheses, a step of 0.02 apart around a base 0.01 off -- the base itself, 0.01 off, where Y = 0)
            assert err_t <= 1.5 * float(P.cell) and err_r <= 0.03, (n, err_t, err_r)
            if window == 0:
                assert (m["a"], m["b"]) == (0, 0) and x0.tobytes() == np.asarray(X0, np.float32).tobytes()      # nothing to search: the base start itself
    assert seen_f1 >= 1 and seen_not_found >= len(SEARCH_CASES) + 1


def _shifted(g, a, b):
    """The grid g moved by (a, b) cells: bit (i + a, j + b) of the result is bit (i, j) of g; what leaves the grid is dropped."""
    G = g.shape[0]
    out = np.zeros_like(g)
    i0, i1, j0, j1 = max(0, -a), min(G, G - a), max(0, -b), min(G, G - b)
    out[i0 + a:i1 + a, j0 + b:j1 + b] = g[i0:i1, j0:j1]
    return out


def test_known_shifts_win_exactly(rule_exe, tmp_path):
    rs = np.random.RandomState(23)
    for P in (co.Params(64, 0.5), co.Params(96, 0.4)):
        live = rs.uniform(size=(P.G, P.G)) < 0.05
        for a, b in ((0, 0), (3, -5), (-12, 12), (1, 31), (-1, -31), (2, 32), (-2, -32), (32, -32), (-32, 31), (0, 32), (17, 0)):
            key = _shifted(live, a, b)
            inside = int(key.sum())
            S = co.scores(live, key, 32)
            k, s, wa, wb = co.best_shift(S, 32, 0)
            assert (s, wa, wb) == (inside, a, b) and inside < live.sum() + (a == 0 and b == 0)
            sh = _run(rule_exe, "shifts", P, np.array([32, 0], np.int32).tobytes() + co.words(live).tobytes() + co.words(key).tobytes(), str(tmp_path))
            assert sh[:-8] == S.astype(np.uint32).tobytes() and int(np.frombuffer(sh[-8:], np.uint64)[0]) == k == co.shift_key(inside, a, b, 0)
        # two equal maxima: the smaller shift wins; at equal length the smaller a, then the smaller b
        one = np.zeros((P.G, P.G), bool); one[30, 40] = True
        for cells, want in (([(30 + 2, 40), (30 - 3, 40)], (2, 0)), ([(30 + 2, 40), (30 - 2, 40)], (-2, 0)), ([(30, 40 + 5), (30, 40 - 5)], (0, -5)),
                            ([(30 + 1, 40 + 2), (30 + 2, 40 + 1), (30 - 1, 40 + 2)], (-1, 2)), ([(30 + 1, 40 - 2), (30 + 1, 40 + 2)], (1, -2))):
            key = np.zeros((P.G, P.G), bool)
            for c in cells:
                key[c] = True
            k, s, wa, wb = co.best_shift(co.scores(one, key, 12), 12, 0)
            assert (s, wa, wb) == (1,) + want
            sh = _run(rule_exe, "shifts", P, np.array([12, 0], np.int32).tobytes() + co.words(one).tobytes() + co.words(key).tobytes(), str(tmp_path))
            assert int(np.frombuffer(sh[-8:], np.uint64)[0]) == k
        # between hypotheses the smaller h wins an equal score and shift, and a larger score wins whatever the rest
        assert co.shift_key(7, 1, 1, 2) > co.shift_key(7, 1, 1, 3) and co.shift_key(8, 32, 32, 33) > co.shift_key(7, 0, 0, 0)
        # an empty grid on either side: no score, found = 0, the start stays X0
        pts = _structured_points(P, rs, 50, 500)
        X0 = np.array([0.5, -0.25, 0, 0, 0, 1.0], np.float32)
        for key, scan in ((np.zeros((P.G, P.G), bool), pts), (co.keyframe_grid(P, pts), np.zeros((10, 3), np.float32))):
            m = co.search(P, scan, X0, key, 12, 1, 0.02, True)
            assert (m["score"], m["a"], m["b"], m["h"], m["found"]) == (0, 0, 0, 0, 0) and m["x0"].tobytes() == X0.tobytes()
            out = _run(rule_exe, "search", P, _pose_header(X0, np.float32(0.02), [12, 1, 1, 1, 1]) + co.words(key).tobytes() + scan.tobytes(), str(tmp_path))
            assert list(np.frombuffer(out[:32], np.int32)) == [0, 0, 0, 0, m["live_bits"], m["key_bits"], 0, 0] and out[32:56] == X0.tobytes()


def _scan(scene, T, seed, **kw):
    from icet_amd import lidar_sim as ls
    return np.ascontiguousarray(ls.make_scan(scene, (T[:3, 3].astype(np.float64), T[:3, :3].astype(np.float64)), seed, **kw).numpy().T)


def _wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def _revisits(seed, r_lo, r_hi, dyaw_max):
    """Twelve scenes (lidar_sim.make_scene(2000 .. 2011)), one keyframe each at a random yaw, each revisited r_lo .. r_hi metres away at a yaw difference of up to
    +-dyaw_max.  Per scene: the two scans, the true start pose, the yaw the appearance search gives and the coarse search's result from it."""
    from icet_amd import lidar_sim as ls
    rs = np.random.RandomState(seed)
    out = []
    for k in range(12):
        scene = ls.make_scene(2000 + k)
        yaw = rs.uniform(-np.pi, np.pi)
        r, phi, dyaw = rs.uniform(r_lo, r_hi), rs.uniform(-np.pi, np.pi), rs.uniform(-dyaw_max, dyaw_max)
        Tk = cm.pose_yaw((0.0, 0.0, 0.0), yaw); Tl = cm.pose_yaw((r * np.cos(phi), r * np.sin(phi), 0.0), yaw + dyaw)
        kf, live = _scan(scene, Tk, 300 + k), _scan(scene, Tl, 400 + k)
        Dq, wq = am.descriptor(A0, live); Dk, wk = am.descriptor(A0, kf)
        app_yaw = am.shift_yaw(am.distance(Dq, wq, Dk, wk)[1], A0.A)
        X0 = np.array([0, 0, 0, 0, 0, app_yaw], np.float32)
        m = co.search(P0, live, X0, co.keyframe_grid(P0, kf), 12, 1, YAW_STEP, True)
        out.append(dict(scene=2000 + k, kf=kf, live=live, truth=cm.start_pose64(Tl, Tk), app_yaw=app_yaw, X0=X0, m=m, r=r, dyaw=dyaw))
    return out


@pytest.fixture(scope="module")
def revisits_11():
    return _revisits(11, 0.5, 2.5, 0.6)


def _check_starts(revs):
    worst_t = worst_r = 0.0
    for e in revs:
        m = e["m"]
        dt = float(np.hypot(*(m["x0"][:2].astype(np.float64) - e["truth"][:2])))
        dr = abs(_wrap(float(m["x0"][5]) - e["truth"][5]))
        print("scene %d: %.2f m, %+.2f rad away; appearance yaw off by %.3f; winner S %d a %d b %d h %d (live %d, keyframe %d bits); start off by %.3f m %.3f rad"
              % (e["scene"], e["r"], e["dyaw"], abs(_wrap(float(e["app_yaw"]) - e["truth"][5])), m["score"], m["a"], m["b"], m["h"], m["live_bits"], m["key_bits"], dt, dr))
        assert m["found"] == 1 and np.abs(m["x0"][[2, 3, 4]]).max() == 0
        assert dt <= START_T and dr <= START_R, (e["scene"], dt, dr)
        worst_t, worst_r = max(worst_t, dt), max(worst_r, dr)
    print("worst start error %.3f m, %.3f rad" % (worst_t, worst_r))


def test_twelve_revisits_up_to_two_and_a_half_metres_start_close_to_the_truth(revisits_11):
    """RandomState(11): 0.5 - 2.5 m, +-0.6 rad.  Every coarse start is within 0.35 m and 0.09 rad of closure_model.start_pose64 of the true poses."""
    _check_starts(revisits_11)


def test_twelve_revisits_up_to_three_metres_and_the_half_turns():
    """RandomState(5): 0 - 3 m, +-1.2 rad.  The same bounds; on scenes 2000, 2009 and 2010 the appearance yaw is a half turn off and the half-turned hypothesis wins."""
    revs = _revisits(5, 0.0, 3.0, 1.2)
    _check_starts(revs)
    half = [e["scene"] for e in revs if abs(_wrap(float(e["app_yaw"]) - e["truth"][5])) > 2.5]
    assert half == [2000, 2009, 2010]
    for e in revs:
        assert co.hypothesis_of(e["m"]["h"], 1)[1] == (1 if e["scene"] in half else 0), e["scene"]


def _oracle_ok(e, x0):
    from oracle import pyoracle as po
    r = po.solve(e["kf"], e["live"], x0=np.asarray(x0, np.float32), runlen=7, bins_phi=24, bins_theta=75)
    dt, dr = np.abs(r["X"][:3] - e["truth"][:3]).max(), np.abs(_wrap(r["X"][3:] - e["truth"][3:])).max()
    return bool(dt <= TOL_T and dr <= TOL_R), float(dt), float(dr)


def test_oracle_converges_from_the_single_coarse_start_more_often_than_from_the_lattice(revisits_11):
    """End to end on the CPU oracle (runlen 7, 75 x 24): from ONE coarse start at least 6 of the 12 revisits end within 0.02 m / 0.035 rad of the truth -- the pinned
    list --, strictly more than from the 3 x 3 lattice of +-0.3 m around the appearance yaw alone (9 starts each)."""
    from icet_amd import api
    coarse, lattice = [], []
    for e in revisits_11:
        ok, dt, dr = _oracle_ok(e, e["m"]["x0"])
        print("scene %d from the coarse start: |dt| %.4f m |dr| %.4f rad" % (e["scene"], dt, dr))
        if ok:
            coarse.append(e["scene"])
        if any(_oracle_ok(e, e["X0"] + off)[0] for off in api.LATTICE_STARTS):
            lattice.append(e["scene"])
    print("converging from the coarse start: %s; from the lattice on the appearance yaw: %s" % (coarse, lattice))
    assert len(coarse) >= 6 and len(coarse) > len(lattice)
    assert coarse == ORACLE_CONVERGING


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

DEV = torch.device("cuda", 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).to(DEV)


def _desc(t, n=None):
    return (t.data_ptr(), t.shape[1] if n is None else int(n), t.shape[1])


def _grids(st, tensors, P, rows=None, ns=None):
    n = len(tensors)
    g = torch.full((n, P.G, P.W), 0x55555555, dtype=torch.int32, device=DEV)
    rows_t = torch.tensor(rows, dtype=torch.int32, device=DEV) if rows is not None else None
    torch.cuda.synchronize()
    st.coarse_grid_device([_desc(t, None if ns is None else ns[i]) for i, t in enumerate(tensors)], g.data_ptr(), rows_t.data_ptr() if rows_t is not None else None)
    st._ctx.sync()
    return g.cpu().numpy().view(np.uint32)


def _same_grid(got, scan, P):
    return got.tobytes() == co.words(co.keyframe_grid(P, scan)).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("P", PARAM_SETS, ids=lambda p: "G%d" % p.G)
def test_grids_equal_the_model_bit_for_bit(frames, sample_pc, P):
    import icet_amd
    import param_sweep
    from icet_amd import lidar_sim as ls
    rng = np.random.default_rng(8)
    rs = np.random.RandomState(24)
    sim = _scan(ls.make_scene(2003), cm.pose_yaw((0.0, 0.0, 0.0), 0.4), 77, rings=16, steps=512)
    scans = [sim, frames[0], sample_pc[0], sample_pc[1], np.concatenate([_structured_points(P, rs), _edge_points(P, rs)])]
    assert (np.abs(sample_pc[0]).sum(1) == 0).sum() > 1000              # the real pair carries thousands of exact-zero rows
    for k in range(3):
        o = param_sweep.spoil(rng, scans[k])[0]
        o[rng.choice(o.shape[0], 40, replace=False), rng.integers(0, 3, 40)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), 40)
        scans.append(o)
    scans += [np.zeros((0, 3), np.float32), np.zeros((50, 3), np.float32), sim[:1], sim[:301]]
    ctx = icet_amd.Context(0)
    st = icet_amd.KeyframeStore(ctx, 60)
    st.enable_coarse(P.G, float(P.cell), float(P.z_lo), float(P.z_hi), float(P.min_span))
    t = [_dev(s) for s in scans]
    g = _grids(st, t, P)                                                # coarse_grid_device, all in one call
    for i, s in enumerate(scans):
        assert _same_grid(g[i], s, P), i
    assert g[:8].any(axis=(1, 2)).all() and not g[8].any() and not g[9].any()
    # put_device: the same words through debug_fetch, whatever the batch: alone, and in one batch of unequal lengths into other slots
    big = [i for i, s in enumerate(scans) if s.shape[0] > 0]
    for i in big[:3]:
        st.put_device([i], [_desc(t[i])])
    st.put_device([30 + i for i in big], [_desc(t[i]) for i in big])
    for i in big:
        for slot in ([i] if i in big[:3] else []) + [30 + i]:
            assert _same_grid(st.debug_fetch(slot, "grid"), scans[i], P), (i, slot)
    # d_rows shorter than n: the device-side count cuts the scan; a count above n or below 0 is clamped
    rows = [1000, 0, 10 ** 9, -5, 333, 1]
    want_n = [min(max(r, 0), scans[i].shape[0]) for i, r in enumerate(rows)]
    g = _grids(st, t[:6], P, rows=rows)
    for i in range(6):
        assert _same_grid(g[i], scans[i][:want_n[i]], P), i
    rows_t = torch.tensor(rows[:3], dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st.put_device([50, 51, 52], [_desc(x) for x in t[:3]], rows_t.data_ptr())
    for i in range(3):
        assert _same_grid(st.debug_fetch(50 + i, "grid"), scans[i][:want_n[i]], P), i
    # a padded leading dimension with NaN in the padding (n < ld; ld not a multiple of 4)
    padded = []
    for s in scans[:3]:
        ld = s.shape[0] + 37 + ((s.shape[0] + 37) % 4 == 0)
        buf = torch.full((3, ld), float("nan"), dtype=torch.float32, device=DEV)
        buf[:, :s.shape[0]] = torch.from_numpy(np.ascontiguousarray(s.T)).to(DEV)
        assert buf.shape[1] % 4
        padded.append(buf)
    g = _grids(st, padded, P, ns=[s.shape[0] for s in scans[:3]])
    for i in range(3):
        assert _same_grid(g[i], scans[i], P), i
    # more scans than one structure pass takes, the same scan alone and among the others
    g20 = _grids(st, [t[(i * 5) % 8] for i in range(20)], P)
    g1 = _grids(st, [t[4]], P)
    assert all(_same_grid(g20[i], scans[(i * 5) % 8], P) for i in range(20)) and g20[4].tobytes() == g1[0].tobytes()
    st.close(); ctx.close()


KF_SLOTS = [3, 0, 9, 5, 12, 7, 1, 14]                                   # the drive of tests/test_loop_closure.py and tests/test_appearance.py
DISTRACTOR_SLOTS = [2, 4, 6, 8, 10, 11, 13, 15]
NEAR = [1, 3, 5, 7]


def _make_drive(n_distractors, **kw):
    """The drive of tests/test_appearance.py: 8 keyframes 1.5 m apart in scene 2000, 4 revisits 0.3 - 0.6 m and 0.2 - 0.5 rad of yaw from their nearest keyframe,
    keyframes of scenes 2001 ... as distractors -- in a store of 40 slots with coarse alignment and appearance enabled.  Slots 30 and 31 were put before enabling."""
    import icet_amd
    from icet_amd import lidar_sim as ls
    scene = ls.make_scene(2000)
    true_kf = [cm.pose_yaw((-5.0 + 1.5 * k, -1.0 + 0.1 * k, 0.0), 0.05 * k) for k in range(8)]
    off = [(0.35, 0.20, 0.30), (-0.30, 0.30, 0.45), (0.25, -0.35, -0.25), (0.40, 0.10, 0.20)]
    live_T = [cm.pose_yaw((true_kf[k][0, 3] + o[0], true_kf[k][1, 3] + o[1], 0.0), 0.05 * k + o[2]) for k, o in zip(NEAR, off)]
    kf = [_scan(scene, T, 100 + k, **kw) for k, T in enumerate(true_kf)]
    live = [_scan(scene, T, 200 + i, **kw) for i, T in enumerate(live_T)]
    distractors = [_scan(ls.make_scene(2001 + k), cm.pose_yaw((0.0, 0.0, 0.0), 0.0), 500 + k, **kw) for k in range(n_distractors)]
    ctx = icet_amd.Context(0)
    st = icet_amd.KeyframeStore(ctx, 40)
    st.put([30, 31], [kf[1], kf[3]])
    st.enable_coarse()
    st.enable_appearance()
    slots, scans = KF_SLOTS + DISTRACTOR_SLOTS[:n_distractors], kf + distractors
    st.put(slots, scans)
    book = {s: co.keyframe_grid(P0, sc) for s, sc in zip(slots, scans)}
    poses = {KF_SLOTS[k]: T for k, T in enumerate(true_kf)}
    st.set_pose(KF_SLOTS, np.stack(true_kf), [10 * k for k in range(8)])
    d = dict(ctx=ctx, st=st, book=book, kf=kf, live=live, live_T=live_T, distractors=distractors, poses=poses, dev=[_dev(s) for s in live],
             truth=np.stack([cm.start_pose(live_T[i], true_kf[k]) for i, k in enumerate(NEAR)]), near=[KF_SLOTS[k] for k in NEAR])
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="module")
def drive():
    """The drive at 16 x 512 rays, where no registration has to find voxels: the grids and the search against the model."""
    d = _make_drive(8, rings=16, steps=512)
    yield d
    d["st"].close(); d["ctx"].close()


@pytest.fixture(scope="module")
def drive_full():
    """The drive at the full 64 x 2048 rays (the 75 x 24 voxels of a registration need the points), with 4 distractors."""
    d = _make_drive(4)
    yield d
    d["st"].close(); d["ctx"].close()


def _align(d, qs, cand, base, se, rows=None):
    from icet_amd import api
    Q, K = cand.shape
    dc = torch.from_numpy(np.ascontiguousarray(cand, np.int32)).to(DEV); db = torch.from_numpy(np.ascontiguousarray(base, np.float32)).to(DEV)
    x0 = torch.full((Q, K, 6), float("nan"), dtype=torch.float32, device=DEV)
    m = torch.full((Q, K, 32), 0x77, dtype=torch.uint8, device=DEV)
    rows_t = torch.tensor(rows, dtype=torch.int32, device=DEV) if rows is not None else None
    torch.cuda.synchronize()
    d["st"].coarse_align_device([_desc(d["dev"][q]) for q in qs], K, dc.data_ptr(), db.data_ptr(), se, x0.data_ptr(), m.data_ptr(), rows_t.data_ptr() if rows_t is not None else None)
    d["ctx"].sync()
    return x0.cpu().numpy(), np.frombuffer(m.cpu().numpy().tobytes(), api.COARSE_MATCH_DTYPE).reshape(Q, K)


def _check_align(d, qs, cand, base, se, rows=None):
    x0, m = _align(d, qs, cand, base, se, rows)
    for i, q in enumerate(qs):
        scan = d["live"][q] if rows is None else d["live"][q][:rows[i]]
        for k in range(cand.shape[1]):
            slot = int(cand[i, k])
            if slot < 0:
                assert m[i, k].tobytes() == bytes(32) and x0[i, k].tobytes() == bytes(24)
                continue
            w = co.search(P0, scan, base[i, k], d["book"].get(slot), se.window, se.n_yaw, se.yaw_step, se.half_turn, se.min_score)
            got = tuple(int(m[i, k][n]) for n in ("score", "a", "b", "h", "live_bits", "key_bits", "found", "reserved"))
            assert got == (w["score"], w["a"], w["b"], w["h"], w["live_bits"], w["key_bits"], w["found"], 0), (q, slot, got, w)
            assert x0[i, k].tobytes() == w["x0"].tobytes(), (q, slot, x0[i, k], w["x0"])
    return x0, m


@pytest.mark.gpu
def test_align_equals_the_model_exactly(drive):
    from icet_amd import api
    d = drive
    S = api.KeyframeStore.coarse_search
    rs = np.random.RandomState(25)
    yaw = lambda q: np.array([0, 0, 0, 0, 0, d["truth"][q, 5]], np.float32)
    # Q = 1, K = 16 with -1 candidates and a slot put before enable; Y = 1 with the half turn; window 12
    cand = np.array([[d["near"][0], 30, -1, 2, 4, 6, 0, 9, -1, 5, 12, 7, 1, 14, 8, -1]], np.int32)
    base = np.tile(yaw(0), (1, 16, 1)); base[0, 3] += np.float32([0.2, -0.1, 0, 0, 0, np.pi])       # one base start a half turn off
    x0, m = _check_align(d, [0], cand, base, S(12, 1, YAW_STEP, True))
    assert m[0, 0]["found"] == 1 and m[0, 1]["found"] == 0 and x0[0, 1].tobytes() == base[0, 1].tobytes() and m[0, 1].tobytes() == bytes(32)
    assert np.abs(x0[0, 0, :2] - d["truth"][0, :2]).max() <= START_T and m[0, 0]["score"] > m[0, 4]["score"]
    # Q = 4, K = 1: every revisit against its nearest keyframe, from the yaw alone; the start lands within a cell or so of the truth
    near = np.array(d["near"], np.int32).reshape(4, 1)
    base4 = np.stack([yaw(q) for q in range(4)]).reshape(4, 1, 6)
    for se in (S(12, 0, YAW_STEP, False), S(12, 1, YAW_STEP, False), S(0, 0, YAW_STEP, False), S(32, 0, YAW_STEP, True), S(12, 1, YAW_STEP, True, min_score=10 ** 6)):
        x0, m = _check_align(d, [0, 1, 2, 3], near, base4, se)
        if se.window == 0:
            assert x0.tobytes() == base4.tobytes() and (m["found"] == 1).all()      # nothing to search: the base start comes back unchanged
        elif se.min_score > 1000:
            assert x0.tobytes() == base4.tobytes() and (m["found"] == 0).all() and (m["score"] > 0).all()
        else:
            assert np.abs(x0[:, 0, :2] - d["truth"][:, :2]).max() <= START_T, (x0[:, 0], d["truth"])
    # base starts with roll and pitch, and translations
    base_rp = base4 + rs.uniform(-1, 1, (4, 1, 6)).astype(np.float32) * np.float32([0.3, 0.3, 0.1, 0.03, 0.03, 0.02])
    _check_align(d, [0, 1, 2, 3], near, base_rp, S(12, 1, YAW_STEP, True))
    # d_rows shorter than n
    _check_align(d, [1, 2], near[1:3], base4[1:3], S(12, 0, YAW_STEP, False), rows=[2000, 3001])
    # two consecutive calls of one shape with other scans, nothing waited for in between
    se = S(12, 0, YAW_STEP, False)
    outs = []
    torch.cuda.synchronize()
    bufs = [(torch.from_numpy(near[q:q + 1]).to(DEV), torch.from_numpy(base4[q:q + 1]).to(DEV), torch.zeros((1, 1, 6), dtype=torch.float32, device=DEV),
             torch.zeros((1, 1, 32), dtype=torch.uint8, device=DEV)) for q in (0, 2, 0)]
    torch.cuda.synchronize()
    for (c, b, x, mm), q in zip(bufs, (0, 2, 0)):
        d["st"].coarse_align_device([_desc(d["dev"][q])], 1, c.data_ptr(), b.data_ptr(), se, x.data_ptr(), mm.data_ptr())
    d["ctx"].sync()
    for (c, b, x, mm), q in zip(bufs, (0, 2, 0)):
        w = co.search(P0, d["live"][q], base4[q, 0], d["book"][d["near"][q]], 12, 0, se.yaw_step, False)
        assert x.cpu().numpy().tobytes() == w["x0"].tobytes() and int(np.frombuffer(mm.cpu().numpy().tobytes(), api.COARSE_MATCH_DTYPE)[0]["score"]) == w["score"]
        outs.append(x.cpu().numpy().tobytes())
    assert outs[0] == outs[2] != outs[1]
    # the host wrapper gives the same
    x0h, mh = d["st"].coarse_align([d["live"][q] for q in range(4)], near, base4, 12, 1, YAW_STEP, True)
    x0d, md = _align(d, [0, 1, 2, 3], near, base4, S(12, 1, YAW_STEP, True))
    assert x0h.tobytes() == x0d.tobytes() and mh.tobytes() == md.tobytes()


def _recs(t):
    from icet_amd import api
    return np.frombuffer(t.cpu().numpy().tobytes(), api.CLOSURE_DTYPE).copy()


def _scores(t):
    from icet_amd import api
    return np.frombuffer(t.cpu().numpy().tobytes(), api.SCORE_DTYPE).copy()


def _close_coarse(d, qs, K, S, se, by_pose, radius, outputs=True, starts=None, runlen=7):
    from icet_amd import api
    st = d["st"]
    Q, R = len(qs), len(qs) * K * S
    rec = torch.zeros((Q, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    cand = torch.full((Q, K), -7, dtype=torch.int32, device=DEV)
    x0 = torch.full((R, 6), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((R, 48), float("nan"), dtype=torch.float32, device=DEV)
    sc = torch.zeros((R, 8), dtype=torch.int32, device=DEV)
    m = torch.full((Q * K, 32), 0x77, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    query = api.ClosureQuery(float(radius), K, 0, S, float("inf"), 0, 0)
    ptr = (lambda t: t.data_ptr()) if outputs else (lambda t: None)
    poses = np.stack([d["live_T"][q] for q in qs]) if by_pose else None
    stamps = [1000 + q for q in qs] if by_pose else None
    st.close_coarse_device([_desc(d["dev"][q]) for q in qs], poses, stamps, st._params(runlen, 0), query, se, rec.data_ptr(),
                           api.LATTICE_STARTS[:S] if starts is None else starts, ptr(cand), ptr(x0), ptr(out), ptr(sc), ptr(m))
    d["ctx"].sync()
    return dict(rec=_recs(rec), cand=cand.cpu().numpy(), x0=x0.cpu().numpy(), out=out.cpu().numpy(), score=_scores(sc),
                match=np.frombuffer(m.cpu().numpy().tobytes(), api.COARSE_MATCH_DTYPE).reshape(Q, K))


@pytest.mark.gpu
@pytest.mark.parametrize("by_pose", [True, False], ids=["pose", "appearance"])
def test_close_coarse_carries_the_bits_of_the_manual_path(drive_full, by_pose):
    """close_coarse_device against what a caller would chain by hand: the existing candidates call, coarse_align_device, register_scored_device,
    icet_select_best_device, the host gate -- and, with nothing to search, against the existing one-call query itself."""
    from icet_amd import api
    d = drive_full
    st, ctx = d["st"], d["ctx"]
    qs, K, S = [0, 1, 2, 3], 5, 2
    radius = 2.0 if by_pose else np.inf                                 # (by pose: one or two keyframes in reach, so -1 candidates and padding registrations)
    se = api.KeyframeStore.coarse_search(12, 1, YAW_STEP, True)
    res = _close_coarse(d, qs, K, S, se, by_pose, radius)
    # 1 the candidates and base starts of the existing calls
    if by_pose:
        cand, base = st.candidates(np.stack([d["live_T"][q] for q in qs]), [1000 + q for q in qs], radius, K)
        dist = shift = None
    else:
        cand, dist, shift, base = st.candidates_by_appearance([d["live"][q] for q in qs], K, radius)
    assert np.array_equal(res["cand"], cand) and (cand >= 0).any()
    if by_pose:
        assert (cand < 0).any()
    # 2 coarse_align_device on them
    x0c, match = _align(d, qs, cand, base, se)
    assert res["match"].tobytes() == match.tobytes()
    want_x0 = np.zeros((len(qs) * K * S, 6), np.float32)
    for i in range(len(qs)):
        for k in range(K):
            for s in range(S):
                if cand[i, k] >= 0:
                    want_x0[(i * K + k) * S + s] = x0c[i, k] + api.LATTICE_STARTS[s]
    assert res["x0"].tobytes() == want_x0.tobytes()
    # 3 the registrations, 4 the best of each query
    live = [r for r in range(len(qs) * K * S) if cand.reshape(-1)[r // S] >= 0]
    slots = [int(cand.reshape(-1)[r // S]) for r in live]
    descs = [_desc(d["dev"][qs[r // (K * S)]]) for r in live]
    xl = torch.from_numpy(want_x0[live]).to(DEV)
    out2 = torch.zeros((len(live), 48), dtype=torch.float32, device=DEV); sc2 = torch.zeros((len(live), 8), dtype=torch.int32, device=DEV)
    best = torch.full((len(qs),), -9, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st.register_scored_device(slots, descs, st._params(7, 0), out2.data_ptr(), sc2.data_ptr(), xl.data_ptr())
    ctx.select_best_device(np.array([r // (K * S) for r in live], np.int32), len(qs), sc2.data_ptr(), best.data_ptr())
    ctx.sync()
    out2, sc2, best = out2.cpu().numpy(), _scores(sc2), best.cpu().numpy()
    assert np.array_equal(out2.view(np.uint32), res["out"][live].view(np.uint32)) and sc2.tobytes() == res["score"][live].tobytes()
    # 5 the records
    want = np.zeros(len(qs), api.CLOSURE_DTYPE)
    for i in range(len(qs)):
        want[i]["n_candidates"] = int((cand[i] >= 0).sum())
        b = int(best[i])
        assert b >= 0
        r = live[b]; k = (r // S) % K
        slot = int(cand[i, k])
        want[i]["slot"] = slot; want[i]["reg"] = r; want[i]["accepted"] = 1
        want[i]["stamp"] = st.debug_fetch(slot, "stamp")
        if by_pose:
            want[i]["d2"] = cm.dist2(d["live_T"][qs[i]][:3, 3], d["poses"][slot][:3, 3].reshape(1, 3))[0]
        else:
            want[i]["d2"] = dist[i, k]; want[i]["reserved0"] = shift[i, k]
        want[i]["x0"] = want_x0[r]; want[i]["out"] = out2[b]; want[i]["score"] = sc2[b]
        mk = match[i, k]
        want[i]["reserved1"] = (mk["score"], co.shift_code(int(mk["a"]), int(mk["b"]), int(mk["h"])))
    rec = res["rec"]
    assert rec.tobytes() == want.tobytes(), [(n, rec[n], want[n]) for n in rec.dtype.names if rec[n].tobytes() != want[n].tobytes()]
    assert (rec["reserved1"][:, 0] > 0).all()
    # the same records when the store uses buffers of its own
    assert _close_coarse(d, qs, K, S, se, by_pose, radius, outputs=False)["rec"].tobytes() == rec.tobytes()
    # nothing to search (window 0, Y = 0, no half turn): the base start comes back unchanged and the registrations are the existing call's, bit for bit
    none = api.KeyframeStore.coarse_search(0, 0, YAW_STEP, False)
    r0 = _close_coarse(d, qs, K, S, none, by_pose, radius)
    R = len(qs) * K * S
    rec_t = torch.zeros((len(qs), api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    c_t = torch.full((len(qs), K), -7, dtype=torch.int32, device=DEV); x_t = torch.full((R, 6), float("nan"), dtype=torch.float32, device=DEV)
    o_t = torch.full((R, 48), float("nan"), dtype=torch.float32, device=DEV); s_t = torch.zeros((R, 8), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    query = api.ClosureQuery(float(radius), K, 0, S, float("inf"), 0, 0)
    sd = [_desc(d["dev"][q]) for q in qs]
    if by_pose:
        st.close_device(sd, np.stack([d["live_T"][q] for q in qs]), [1000 + q for q in qs], st._params(7, 0), query, rec_t.data_ptr(), api.LATTICE_STARTS[:S],
                        c_t.data_ptr(), x_t.data_ptr(), o_t.data_ptr(), s_t.data_ptr())
    else:
        st.close_appearance_device(sd, None, st._params(7, 0), query, rec_t.data_ptr(), api.LATTICE_STARTS[:S], c_t.data_ptr(), x_t.data_ptr(), o_t.data_ptr(), s_t.data_ptr())
    ctx.sync()
    assert np.array_equal(r0["cand"], c_t.cpu().numpy()) and r0["x0"].tobytes() == x_t.cpu().numpy().tobytes()
    assert r0["out"].tobytes() == o_t.cpu().numpy().tobytes() and r0["score"].tobytes() == _scores(s_t).tobytes()
    old = _recs(rec_t)
    assert (old["reserved1"] == 0).all()                                # the existing calls keep these words zero
    new = r0["rec"].copy()
    assert (new["reserved1"][:, 0] > 0).all() and (new["reserved1"][:, 1] == co.shift_code(0, 0, 0)).all()
    new["reserved1"] = 0
    assert new.tobytes() == old.tobytes()


@pytest.mark.gpu
def test_pinned_revisits_close_on_the_device_from_a_single_coarse_start(revisits_11):
    """The revisits the CPU oracle converges on, through find_closures_coarse at S = 1 with candidates by appearance among all twelve keyframes: each ends within
    0.02 m / 0.035 rad of the truth, with the right slot."""
    import icet_amd
    ctx = icet_amd.Context(0)
    st = icet_amd.KeyframeStore(ctx, 12)
    st.enable_appearance(); st.enable_coarse()
    st.put(list(range(12)), [e["kf"] for e in revisits_11])
    pinned = [e for e in revisits_11 if e["scene"] in ORACLE_CONVERGING]
    got = st.find_closures_coarse([e["live"] for e in pinned], 7, 4)
    for e, g in zip(pinned, got):
        dt, dr = np.abs(g["X"][:3] - e["truth"][:3]).max(), np.abs(_wrap(g["X"][3:] - e["truth"][3:])).max()
        print("scene %d: slot %s, coarse %s, start %s: |dt| %.4f m |dr| %.4f rad" % (e["scene"], g["slot"], g["coarse"], g["x0"], dt, dr))
        assert g["slot"] == e["scene"] - 2000 and g["accepted"]
        assert g["coarse"] == dict(score=e["m"]["score"], a=e["m"]["a"], b=e["m"]["b"], h=e["m"]["h"]) and g["x0"].tobytes() == (e["m"]["x0"] + np.float32(0)).tobytes()      # (start 0 is fl(X0_coarse + 0))
        assert dt <= TOL_T and dr <= TOL_R, (e["scene"], dt, dr)
    st.close(); ctx.close()


@pytest.mark.gpu
def test_nothing_else_moves_and_refusals(drive, drive_full, frames):
    import icet_amd
    from icet_amd import api
    from test_keyframe_store import _bytes, _same_bytes
    d = drive
    st, ctx = d["st"], d["ctx"]
    prm = st._params(7, 0)
    watched = KF_SLOTS + [30]
    S = api.KeyframeStore.coarse_search

    def parked():
        out = torch.zeros((1, 48), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        ctx.register_device([_desc(d["dev"][1])], prm, out.data_ptr())
        ctx.sync()
        return out.cpu().numpy()

    def state():
        return [(_bytes(st, s), st.debug_fetch(s, "pose"), st.debug_fetch(s, "stamp"),
                 (st.debug_fetch(s, "descriptor"), st.debug_fetch(s, "weights"), st.debug_fetch(s, "grid")) if s != 30 else None) for s in watched]

    def same(x, y):
        return all(_same_bytes(p[0], q[0]) and p[1].tobytes() == q[1].tobytes() and p[2] == q[2] and
                   (p[3] is None or all(u.tobytes() == v.tobytes() for u, v in zip(p[3], q[3]))) for p, q in zip(x, y))

    with pytest.raises(icet_amd.IcetError) as e:                        # a slot put before enable has no grid
        st.debug_fetch(30, "grid")
    assert e.value.status == api.ICET_ERR_BAD_ARG
    kf2 = _dev(d["kf"][2])
    torch.cuda.synchronize()
    ctx.keyframe_device([_desc(kf2)], prm)
    before, out_before = state(), parked()
    assert np.isfinite(out_before).all()
    for s, k in zip(KF_SLOTS, range(8)):
        assert st.debug_fetch(s, "grid").tobytes() == co.words(d["book"][s]).tobytes()
    # the new calls, whole solves and another store's calls leave everything as it was
    near = np.array(d["near"], np.int32).reshape(4, 1)
    base = np.zeros((4, 1, 6), np.float32); base[:, 0, 5] = d["truth"][:, 5]
    _align(d, [0, 1, 2, 3], near, base, S())
    _close_coarse(d, [0, 1], 4, 2, S(), True, 2.0)
    _close_coarse(d, [2], 3, 1, S(), False, np.inf, outputs=False)
    st.coarse_grid([frames[0]])
    assert same(before, state()) and parked().tobytes() == out_before.tobytes()
    ctx.solve(frames[0], frames[1], 3, np.zeros(6, np.float32), 24, 75)
    st2 = icet_amd.KeyframeStore(ctx, 8)
    st2.enable_coarse(64, 0.5)
    st2.put([1, 2], [d["live"][0], d["live"][1]])
    st2.coarse_align([d["live"][2]], [[1]], np.zeros((1, 1, 6), np.float32))
    st2.close()
    st.put([33], [d["live"][3]])                                        # a put into another slot
    ctx.keyframe_device([_desc(kf2)], prm)
    assert same(before, state()) and parked().tobytes() == out_before.tobytes()
    assert st.debug_fetch(33, "grid").tobytes() == co.words(co.keyframe_grid(P0, d["live"][3])).tobytes()
    # reserve carries the grids over; a slot beyond the old capacity gets one; a put replaces exactly its own slot's grid
    st.reserve(64)
    assert same(before, state())
    st.put([50], [d["live"][2]])
    assert st.debug_fetch(50, "grid").tobytes() == co.words(co.keyframe_grid(P0, d["live"][2])).tobytes()
    st.put([50], [d["kf"][5]])
    assert st.debug_fetch(50, "grid").tobytes() == co.words(co.keyframe_grid(P0, d["kf"][5])).tobytes()
    assert st.debug_fetch(33, "grid").tobytes() == co.words(co.keyframe_grid(P0, d["live"][3])).tobytes()
    d["book"][50] = co.keyframe_grid(P0, d["kf"][5]); d["book"][33] = co.keyframe_grid(P0, d["live"][3])
    x0, m = _check_align(d, [2], np.array([[50, 33]], np.int32), np.zeros((1, 2, 6), np.float32), S(12, 0, YAW_STEP, False))
    ctx.keyframe_device([_desc(kf2)], prm)
    assert same(before, state())
    # refused calls change nothing
    out_before = parked()
    bad_search = [S(33), S(-1), S(12, 9), S(12, -1), S(12, 1, YAW_STEP, True, 0), S(12, 1, float("nan"))]
    r = S(); r.reserved[1] = 1; bad_search.append(r)
    h = S(); h.half_turn = 2; bad_search.append(h)
    for se in bad_search:
        for call in (lambda: _align(d, [0], near[:1], base[:1], se), lambda: _close_coarse(d, [0], 2, 1, se, False, np.inf)):
            with pytest.raises(icet_amd.IcetError) as e:
                call()
            assert e.value.status == api.ICET_ERR_BAD_ARG
    for se in (S(32, 8), S(0, 0)):                                      # the limits themselves are accepted
        _align(d, [0], near[:1], base[:1], se)
    for kw in (dict(K=33), dict(K=0), dict(S=17), dict(S=0)):
        args = dict(K=2, S=1); args.update(kw)
        with pytest.raises(icet_amd.IcetError) as e:
            _close_coarse(d, [0], args["K"], args["S"], S(), True, 2.0, starts=np.zeros((args["S"], 6), np.float32))
        assert e.value.status == api.ICET_ERR_BAD_ARG
    dc = torch.zeros((1, 33), dtype=torch.int32, device=DEV); db = torch.zeros((1, 33, 6), dtype=torch.float32, device=DEV)
    for K, cp, bp, scans in ((33, dc.data_ptr(), db.data_ptr(), [_desc(d["dev"][0])]), (0, dc.data_ptr(), db.data_ptr(), [_desc(d["dev"][0])]),
                             (1, None, db.data_ptr(), [_desc(d["dev"][0])]), (1, dc.data_ptr(), None, [_desc(d["dev"][0])]),
                             (1, dc.data_ptr(), db.data_ptr(), [(d["dev"][0].data_ptr(), 10, 5)]), (1, dc.data_ptr(), db.data_ptr(), [])):
        with pytest.raises(icet_amd.IcetError) as e:
            st.coarse_align_device(scans, K, cp, bp, S())
        assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError) as e:                        # a NULL grid buffer
        st.coarse_grid_device([_desc(d["dev"][0])], None)
    assert e.value.status == api.ICET_ERR_BAD_ARG
    rec = torch.zeros((1, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    q1 = api.ClosureQuery(1.0, 4, 0, 1, float("inf"), 0, 0)
    with pytest.raises(icet_amd.IcetError) as e:                        # another grid than the store's
        st.close_coarse_device([_desc(d["dev"][0])], None, None, api.Params(7, 20, 75, 25, 0.1, 0.1, 0), q1, S(), rec.data_ptr())
    assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError) as e:                        # enabling twice
        st.enable_coarse()
    assert e.value.status == api.ICET_ERR_BAD_ARG
    st3 = icet_amd.KeyframeStore(ctx, 4)
    st3.enable_appearance()
    full = drive_full
    st3.put([0, 1], [full["kf"][0], full["live"][0]])
    for kw in (dict(cells=32), dict(cells=544), dict(cells=100), dict(cells=0), dict(cell=0.0), dict(cell=-0.25), dict(cell=float("nan")), dict(z_lo=1.0, z_hi=1.0),
               dict(z_lo=2.0, z_hi=1.0), dict(min_span=0.0)):
        with pytest.raises(icet_amd.IcetError) as e:
            st3.enable_coarse(**kw)
        assert e.value.status == api.ICET_ERR_BAD_ARG and st3.coarse is None
    cp = api.CoarseParams(256, 0.25, -3.0, 12.0, 0.5, (C.c_int32 * 3)(0, 0, 7))
    assert api.load_library().icet_keyframe_store_enable_coarse(st3._h, C.byref(cp)) == api.ICET_ERR_BAD_ARG      # a nonzero reserved word
    # a store without enable_coarse refuses the new calls, and its existing queries return what they did
    for call in (lambda: st3.coarse_grid_device([_desc(d["dev"][0])], dc.data_ptr()), lambda: st3.coarse_align_device([_desc(d["dev"][0])], 1, dc.data_ptr(), db.data_ptr(), S()),
                 lambda: st3.close_coarse_device([_desc(d["dev"][0])], None, None, prm, q1, S(), rec.data_ptr())):
        with pytest.raises(icet_amd.IcetError) as e:
            call()
        assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError):
        st3.debug_fetch(0, "grid")
    a1 = st3.find_closures_by_appearance([full["live"][0]], 7, 2, starts=api.LATTICE_STARTS[:2])
    st4 = icet_amd.KeyframeStore(ctx, 4)
    st4.enable_appearance(); st4.enable_coarse(64, 0.5)
    st4.put([0, 1], [full["kf"][0], full["live"][0]])
    a2 = st4.find_closures_by_appearance([full["live"][0]], 7, 2, starts=api.LATTICE_STARTS[:2])
    assert a1[0]["slot"] == a2[0]["slot"] == 1 and a1[0]["X"].tobytes() == a2[0]["X"].tobytes() and a1[0]["score"] == a2[0]["score"]
    for s in (0, 1):                                                    # the keyframe tables are the bytes they are without coarse alignment
        assert _same_bytes(_bytes(st3, s), _bytes(st4, s))
    st3.close(); st4.close()
    ctx.set_option("keep", 1)
    try:
        with pytest.raises(icet_amd.IcetError) as e:
            _close_coarse(d, [0], 2, 1, S(), True, 2.0)
        assert e.value.status == api.ICET_ERR_UNSUPPORTED
    finally:
        ctx.set_option("keep", 0)
    ctx.keyframe_device([_desc(kf2)], prm)
    assert same(before, state()) and parked().tobytes() == out_before.tobytes()
