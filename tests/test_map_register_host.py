"""CPU tests of the registration against a shaped voxel map (include/icet_hip.h icet_voxel_map_register_*): the header the kernels compile
(icet_amd/csrc/icet_map_register.h), built with g++ into a stand-alone program (tests/cpp/test_map_register_rule.cpp), equals the NumPy model
(tests/map_register_model.py) bit for bit on row terms, Gaussian records, damped solves and retractions, and on a whole call run on the CPU; the same program is
clean under the address and undefined-behaviour sanitizers; the entry points are exported and refuse NULL; both structs have the size and offsets of their
ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_model as mm
import map_register_cases as cs
import map_register_model as rm
import map_shape_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icet_voxel_map_register_device", "icet_voxel_map_register_posed_device", "icet_debug_voxel_map_register_terms")
SRC = os.path.join(ROOT, "tests", "cpp", "test_map_register_rule.cpp")


@pytest.fixture(scope="module")
def rule_prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_register_rule") / "test_map_register_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", SRC, "-o", exe])
    return exe


def _b32(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def _b64(v):
    return "%016x" % int(np.float64(v).view(np.uint64))


def _run(exe, mode, text, tmp_path):
    f = tmp_path / (mode + ".txt")
    f.write_text(text)
    return subprocess.check_output([exe, mode, str(f)]).decode().split("\n")[:-1]


# ---- row terms ------------------------------------------------------------------------------------------------------------------------------------------------------

def _rows_text(G, rows, poses, scale, mn, mx):
    lines = ["%s %s %s %s %d %d" % (_b32(G.cell), _b32(mn), _b32(mx), _b64(scale), G.key.shape[0], len(rows))]
    for k, mu, W in zip(G.key, G.mu, G.W):
        lines.append("%d %s" % (int(k), " ".join(_b64(v) for v in list(mu) + list(W))))
    for p, (R, t) in zip(rows, poses):
        lines.append(" ".join([_b64(v) for v in list(R.reshape(9)) + list(t)] + [_b32(v) for v in p]))
    return "\n".join(lines) + "\n"


def _rows_case(exe, tmp_path, G, rows, poses, scale=11.3449, mn=0.0, mx=0.0):
    """rows (N x 3 float32), poses (N float64 (R, t)): the program's record per row against the model's.  Returns the classes and the matched flags."""
    rows = np.asarray(rows, np.float32).reshape(-1, 3)
    got = _run(exe, "rows", _rows_text(G, rows, poses, scale, mn, mx), tmp_path)
    assert len(got) == rows.shape[0]
    cls, matched = [], []
    for i, line in enumerate(got):
        tm = rm.row_terms(rows[i:i + 1], poses[i][0], poses[i][1], G, scale, mn, mx)
        want = [str(int(tm["cls"][0])), str(int(tm["key"][0])), str(int(tm["matched"][0]))] + [_b64(tm[k][0]) for k in ("s", "omega", "rho")] + [_b64(v) for v in tm["v"][0]]
        assert line.split() == want, (i, rows[i], poses[i])
        cls.append(int(tm["cls"][0])); matched.append(bool(tm["matched"][0]))
    return np.array(cls), np.array(matched)


@pytest.mark.parametrize("cell", [0.1, 0.5])
def test_header_equals_the_model_on_row_terms(rule_prog, tmp_path, cell):
    m = cs.model_map(cell)
    rows, poses = [], []
    for r, T, _ in mm.edge_rows(cell):                                 # the map rule's edge table: its rows join the map, so that most of them match a cell
        m.add([r] * 6, [T] * 6)
    G = rm.Gaussians(m, min_points=5)
    for r, T, _ in mm.edge_rows(cell):
        for p in r:
            rows.append(p); poses.append(rm.pose64(T))
    cls, matched = _rows_case(rule_prog, tmp_path, G, rows, poses)
    assert matched.sum() >= 16 and set(cls) == {mm.KEPT, mm.NONFINITE, mm.RANGE, mm.OUTSIDE}
    r, want = mm.range_rows()
    cls, _ = _rows_case(rule_prog, tmp_path, G, r, [rm.pose64(mm.pose())] * len(r), mn=5.0, mx=13.0)
    assert list(cls) == want
    rs = np.random.RandomState(41)
    ext = np.array([18.0, 18.0, 4.0]) * cell
    rows, poses = [], []
    for _ in range(2000):                                             # random rows at random poses, the poses in double (a pose after a step is no float32)
        T = mm.pose(t=rs.randn(3) * cell, r=rs.randn(3) * [0.05, 0.05, 3.0]).astype(np.float64)
        R = T[:3, :3] + rs.randn(3, 3) * 1e-9; t = T[:3, 3] + rs.randn(3) * 1e-9
        w = rs.rand(3) * ext - ext / 2
        rows.append(((w - t) @ R).astype(np.float32)); poses.append((R, t))
    cls, matched = _rows_case(rule_prog, tmp_path, G, rows, poses)
    assert (cls == mm.KEPT).all() and 800 < matched.sum() < 2000
    rows = cs.term_rows(cell, 300)
    cls, matched = _rows_case(rule_prog, tmp_path, G, rows, [rm.pose64(cs.POSE)] * 300, mn=0.05, mx=30.0)
    assert set(cls) == {mm.KEPT, mm.NONFINITE, mm.RANGE}
    cls, matched = _rows_case(rule_prog, tmp_path, G, rows, [rm.pose64(cs.POSE)] * 300)
    assert mm.OUTSIDE in cls and not matched[:4].any()                # the empty cell, the cell below min_points, the emptied and the negative-count cell


# ---- Gaussian records ---------------------------------------------------------------------------------------------------------------------------------------------

def _gauss_cases():
    """(cell, sigma_min, min_points, key, n, sums, words): cells of real rows, n = 1, n below min_points, counts up to 2^32 - 1, words of a half-removed cell, an
    emptied and a negative-count entry, and a singular C' (sigma_min so small that its square is 0, on a cell of one row)."""
    rs = np.random.RandomState(42)
    cases = []
    for cell in (0.1, 0.5, 0.37):
        m = cs.model_map(cell)
        for sigma, mp in ((0.02, 5), (0.005, 1)):
            cases += [(cell, sigma, mp, k, m.cells[k][0], [v & sm.MASK for v in m.cells[k][1:4]], m.words(k)) for k in sorted(m.mom)[:250]]
        key = int(mm.classify(np.array([[3.3 * cell, -2.2 * cell, 1.1 * cell]], np.float32), mm.pose(), cell)[1][0])
        for q in ([0, 0, 0], [1 << 16, 5 << 16, 65535 << 16], [(1 << 32) - 1] * 3):
            h = [v >> 16 for v in q]
            w = h + [h[a] * h[b] for a, b in sm.PAIRS]
            cases.append((cell, 0.02, 1, key, 1, q, w))                # one row: W = I / sigma_min^2
            cases.append((cell, 0.02, 5, key, 1, q, w))                # below min_points
            cases.append((cell, 1e-200, 1, key, 1, q, w))              # C' = 0: singular
        for n in (4, 5, 1000, (1 << 31) + 12345, (1 << 32) - 1):
            for _ in range(8):                                        # n rows spread over a few offsets: exact integer sums and words of any size
                qs = rs.randint(0, 1 << 32, size=(4, 3), dtype=np.int64); qs[0] = [(1 << 32) - 1, 0, (1 << 32) - 1]
                cnt = [n // 4 + (1 if j < n % 4 else 0) for j in range(4)]
                hs = qs >> 16
                sums = [sum(c * int(q[a]) for c, q in zip(cnt, qs)) & sm.MASK for a in range(3)]
                w = [sum(c * int(h[a]) for c, h in zip(cnt, hs)) for a in range(3)]
                w += [sum(c * int(h[a]) * int(h[b]) for c, h in zip(cnt, hs)) & sm.MASK for a, b in sm.PAIRS]
                cases.append((cell, 0.02, 5, key, n, sums, w))
        cases.append((cell, 0.02, 5, key, 5, [(-7) & sm.MASK, 3, 9], [(-7) & sm.MASK, 3, 9, (-50) & sm.MASK, 4, 5, 6, 7, 8]))      # half removed: words read as uint64
        cases.append((cell, 0.02, 1, key, 0, [0, 0, 0], [0] * 9))     # emptied
        cases.append((cell, 0.02, 1, key, -2, [(-5) & sm.MASK] * 3, [(-5) & sm.MASK] * 9))      # negative
        cases.append((cell, 0.02, 0, key, 0, [0, 0, 0], [0] * 9))     # min_points 0 means 1
    return cases


def _gauss_text(cases):
    return "".join("%s %s %d %d %d %s\n" % (_b32(c), _b64(s), mp, k, n, " ".join(str(int(v)) for v in list(sums) + list(w))) for c, s, mp, k, n, sums, w in cases)


def test_gaussian_records_equal_the_model_bit_for_bit(rule_prog, tmp_path):
    cases = _gauss_cases()
    got = _run(rule_prog, "gauss", _gauss_text(cases), tmp_path)
    assert len(got) == len(cases) > 1000
    usable = 0
    for line, (cell, sigma, mp, key, n, sums, w) in zip(got, cases):
        g = rm.gauss(key, n, sums, w, cell, sigma, mp)
        want = ["0"] + [_b64(0.0)] * 9 if g is None else ["1"] + [_b64(v) for v in g[0] + g[1]]
        assert line.split() == want, (cell, sigma, mp, key, n, sums, w)
        usable += g is not None
        if n < max(1, mp) or sigma == 1e-200:
            assert g is None
        elif sums[0] != (-7) & sm.MASK:                                # (the half-removed cell's words are no covariance: either way, as the model says)
            assert g is not None
        if g is not None and n == 1:
            s2 = sigma * sigma
            assert g[1][1] == 0 and g[1][2] == 0 and g[1][4] == 0 and all(abs(g[1][j] * s2 - 1.0) < 1e-15 for j in (0, 3, 5))
    assert 500 < usable < len(cases)


# ---- damped solves and retractions ----------------------------------------------------------------------------------------------------------------------------------

def _solve_cases():
    """(H21, g, lambda, R, t): sums of real rows, and the edges -- a zero diagonal, a failed pivot, om . om just below and just above 1, a NaN in H, in g, an infinite
    step."""
    rs = np.random.RandomState(43)
    G = rm.Gaussians(cs.model_map(0.5))
    cases = []
    for i in range(300):
        T = mm.pose(t=rs.randn(3) * 0.3, r=rs.randn(3) * [0.03, 0.03, 1.0])
        R, t = rm.pose64(T)
        rows = cs.term_rows(0.5, 200, pose=T, seed=100 + i)
        tot, _, _ = rm.totals(rm.row_terms(rows, R, t, G), "forward")
        cases.append((tot[7:], tot[1:7] * 10.0 ** rs.randint(-3, 2), 10.0 ** rs.randint(-9, 3), R + rs.randn(3, 3) * 1e-9, t))
    H0, g0, _, R0, t0 = cases[0]
    eye = np.array([1.0 if i == j else 0.0 for i, j in rm.TRI])
    z = H0.copy(); z[0] = 0.0
    cases.append((z, g0, 1e-3, R0, t0))                                # a zero diagonal
    z = H0.copy(); z[rm.TRI.index((1, 1))] = -1.0
    cases.append((z, g0, 1e-3, R0, t0))                                # a negative pivot
    z = eye.copy(); z[rm.TRI.index((0, 1))] = 1.0                      # singular: the second pivot is exactly 0
    cases.append((z, g0, 0.0, R0, t0))
    for u in (1.0 - 2.0 ** -52, 1.0, 1.0 + 2.0 ** -51, 0.999, 1.001, 4.0):      # H = I, lambda = 0: delta = -g exactly
        om = np.array([0.6, 0.0, 0.8]) * np.sqrt(u)
        cases.append((eye, np.concatenate([[0.1, -0.2, 0.3], -om]), 0.0, R0, t0))
    z = H0.copy(); z[5] = np.nan
    cases.append((z, g0, 1e-3, R0, t0))
    z = g0.copy(); z[2] = np.nan
    cases.append((H0, z, 1e-3, R0, t0))
    z = g0.copy(); z[4] = np.inf
    cases.append((H0, z, 1e-3, R0, t0))
    cases.append((eye * 1e-300, np.ones(6) * 1e300, 0.0, R0, t0))      # an overflowing step
    return cases


def test_solves_and_retractions_equal_the_model_bit_for_bit(rule_prog, tmp_path):
    cases = _solve_cases()
    text = "".join(" ".join(_b64(v) for v in list(H) + list(g) + [lam] + list(np.asarray(R).reshape(9)) + list(t)) + "\n" for H, g, lam, R, t in cases)
    got = _run(rule_prog, "solve", text, tmp_path)
    assert len(got) == len(cases) > 300
    solved = stepped = 0
    for line, (H, g, lam, R, t) in zip(got, cases):
        d = rm.solve_damped(H, g, lam)
        q = rm.retract(R, t, d) if d is not None else None
        Q = (np.asarray(R, np.float64), np.asarray(t, np.float64)) if q is None else q
        want = [str(int(d is not None))] + [_b64(v) for v in (d if d is not None else [0.0] * 6)] + [str(int(q is not None))]
        want += [_b64(v) for v in list(Q[0].reshape(9)) + list(Q[1])] + ["1"]      # (the last word: the rule's E is pose_from_twist's, bit for bit)
        assert line.split() == want, (H, g, lam)
        solved += d is not None; stepped += q is not None
    assert solved >= 300 and 300 <= stepped < solved and solved < len(cases)
    # the edges, by name: om . om just below 1 steps, just above does not
    flags = [(ln.split()[0], ln.split()[7]) for ln in got[303:309]]
    assert flags == [("1", "1"), ("1", "1"), ("1", "0"), ("1", "1"), ("1", "0"), ("1", "0")]


# ---- a whole call on the CPU ----------------------------------------------------------------------------------------------------------------------------------------

def _loop_text(m, queries, P):
    keys = sorted(m.cells)
    lines = ["%s %s %s %s %d %d %d %d %d" % (_b32(m.cell), _b32(P["min_range"]), _b32(P["max_range"]),
                                            " ".join(_b64(P[k]) for k in ("sigma_min", "scale", "tol_t", "tol_r", "lambda0")), P["min_points"], P["min_matched"],
                                            P["max_iters"], len(keys), len(queries))]
    for k in keys:
        e = m.cells[k]
        lines.append("%d %d %s" % (k, e[0], " ".join(str(int(v) & sm.MASK) for v in list(e[1:4]) + (m.words(k) if k in m.mom else [0] * 9))))
    for scan, T in queries:
        scan = np.asarray(scan, np.float32).reshape(-1, 3)
        lines.append(" ".join(_b32(v) for v in np.asarray(T, np.float32).reshape(16)) + " %d" % scan.shape[0])
        lines += [" ".join(_b32(v) for v in p) for p in scan]
    return "\n".join(lines) + "\n"


def _loop_queries():
    """A small scene: the slab map at cell 0.5 with its special cells; scans of 2500 rows (two chunks) from perturbed poses, one scan of no row, one pose 1 km
    away, one pose with a NaN."""
    T = cs.POSE
    rows = cs.term_rows(0.5, 2500, pose=T)
    Tn = T.copy(); Tn[1, 3] = np.nan
    return [(rows, mm.pose(t=(0.37 + 0.1, -0.21 - 0.05, 0.11 + 0.05), r=(0.02, -0.015, 0.42))), (rows, T), (rows[:0], T), (rows, mm.pose(t=(1000.0, 0, 0))), (rows, Tn),
            (rows[:300], mm.pose(t=(0.30, -0.15, 0.10), r=(0.02, -0.015, 0.38)))]


def _check_loop(exe, tmp_path, P):
    m = cs.model_map(0.5)
    G = rm.Gaussians(m, P["sigma_min"], P["min_points"])
    queries = _loop_queries()
    got = _run(exe, "loop", _loop_text(m, queries, P), tmp_path)
    assert len(got) == len(queries)
    recs = []
    for line, (scan, T) in zip(got, queries):
        r = rm.register(scan, T, G, order="chunks", **P)
        want = [str(r[k]) for k in ("status", "iterations", "accepted", "rows_scored", "rows_matched")] + [_b32(v) for v in r["pose"].reshape(16)]
        want += [_b64(r[k]) for k in ("cost", "cost_start", "lambda")] + [_b64(v) for v in list(r["g"]) + list(r["info"])]
        assert line.split() == want, (T, r)
        recs.append(r)
    return recs


def test_the_whole_loop_on_the_cpu_equals_the_model_bit_for_bit(rule_prog, tmp_path):
    recs = _check_loop(rule_prog, tmp_path, rm.params(max_iters=30))
    assert [r["status"] for r in recs[2:5]] == [rm.NO_OVERLAP, rm.NO_OVERLAP, rm.BAD_POSE]
    assert recs[0]["accepted"] >= 3 and recs[0]["cost"] < recs[0]["cost_start"] and recs[0]["status"] in (rm.CONVERGED, rm.STALLED, rm.ITERATION_CAP)
    assert recs[3]["cost"] == rm.DEFAULTS["scale"] * recs[3]["rows_scored"] and recs[3]["rows_matched"] == 0
    recs = _check_loop(rule_prog, tmp_path, rm.params(max_iters=0, min_matched=10))
    assert all(r["iterations"] == 0 and r["status"] in (rm.ITERATION_CAP, rm.NO_OVERLAP, rm.BAD_POSE) for r in recs)


def test_the_program_is_clean_under_the_address_and_undefined_sanitizers(tmp_path):
    """The stand-alone program alone, built with -fsanitize=address,undefined: the whole loop against exact-size buffers, the extreme tables, the edge solves."""
    exe = str(tmp_path / "test_map_register_rule_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe],
                       stderr=subprocess.PIPE)
    if r.returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime: " + r.stderr.decode()[-200:])
    _check_loop(exe, tmp_path, rm.params(max_iters=6))
    cases = [c for c in _gauss_cases() if c[4] > 1000 or c[4] <= 1][:200]
    assert len(_run(exe, "gauss", _gauss_text(cases), tmp_path)) == len(cases)
    cases = _solve_cases()[295:]
    text = "".join(" ".join(_b64(v) for v in list(H) + list(g) + [lam] + list(np.asarray(R).reshape(9)) + list(t)) + "\n" for H, g, lam, R, t in cases)
    assert len(_run(exe, "solve", text, tmp_path)) == len(cases)
    rows = cs.term_rows(0.1, 64)
    G = rm.Gaussians(cs.model_map(0.1))
    _rows_case(exe, tmp_path, G, rows, [rm.pose64(cs.POSE)] * 64)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_register_entry_points_are_exported_and_refuse_null():
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    sc = api.DevScan(0, 0, 0)
    pose = np.eye(4, dtype=np.float32)
    assert lib.icet_voxel_map_register_device(None, 1, C.byref(sc), pose.ctypes.data, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_register_posed_device(None, 1, C.byref(sc), None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_debug_voxel_map_register_terms(None, C.byref(sc), pose.ctypes.data, None, None) == api.ICET_ERR_BAD_ARG


def test_register_structs_size_and_offsets_match_the_ctypes_mirrors(tmp_path):
    from icet_amd import api
    pf = ("min_range", "max_range", "sigma_min", "scale", "tol_t", "tol_r", "lambda0", "min_points", "min_matched", "max_iters", "flags", "reserved")
    rf = ("pose", "info", "g", "cost", "cost_start", "lambda", "rows_scored", "rows_matched", "iterations", "accepted", "status", "reserved")
    tf = ("key", "cls", "matched", "s", "omega", "rho", "g", "H")
    src = tmp_path / "sizes.c"
    body = 'printf("%d", (int)sizeof(icet_voxel_map_register_params));\n' + "".join('printf(" %%d", (int)offsetof(icet_voxel_map_register_params, %s));\n' % f for f in pf)
    body += 'printf("\\n%d", (int)sizeof(icet_voxel_map_registration));\n' + "".join('printf(" %%d", (int)offsetof(icet_voxel_map_registration, %s));\n' % f for f in rf)
    body += 'printf("\\n%d", (int)sizeof(icet_voxel_map_register_term));\n' + "".join('printf(" %%d", (int)offsetof(icet_voxel_map_register_term, %s));\n' % f for f in tf)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icet_hip.h"\nint main(void){\n' + body + 'printf("\\n"); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    got = [[int(v) for v in ln.split()] for ln in subprocess.check_output([str(tmp_path / "sizes")]).decode().split("\n") if ln]
    assert got[0] == [C.sizeof(api.MapRegisterParams)] + [getattr(api.MapRegisterParams, f).offset for f in pf]
    assert got[0] == [72, 0, 4, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64]
    assert got[1] == [C.sizeof(api.MapRegistration)] + [getattr(api.MapRegistration, "lambda_" if f == "lambda" else f).offset for f in rf]
    assert got[1] == [api.MAP_REGISTRATION_DTYPE.itemsize] + [api.MAP_REGISTRATION_DTYPE.fields[f][1] for f in rf]
    assert got[1] == [328, 0, 64, 232, 280, 288, 296, 304, 308, 312, 316, 320, 324] and got[1][0] % 8 == 0
    assert got[2] == [api.MAP_REGISTER_TERM_DTYPE.itemsize] + [api.MAP_REGISTER_TERM_DTYPE.fields[f][1] for f in tf]
    assert got[2] == [256, 0, 8, 12, 16, 24, 32, 40, 88]
