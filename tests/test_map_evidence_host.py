"""CPU tests of a voxel map's visibility evidence (include/icet_hip.h icet_voxel_map_evidence_*): the header the kernels compile
(icet_amd/csrc/icet_map_evidence.h), built with g++ into a stand-alone program (tests/cpp/test_map_evidence_rule.cpp), equals the NumPy model
(tests/map_evidence_model.py) bit for bit, plain and under the address and undefined-behaviour sanitizers; the entry points are exported and refuse NULL; the
records have the sizes of their ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_evidence_cases as cases
import map_evidence_model as em
import map_model as mm
import map_query_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_map_evidence_rule.cpp")
NEW_SYMBOLS = ("icet_voxel_map_evidence_device", "icet_voxel_map_evidence_posed_device", "icet_voxel_map_evidence_fetch_device")
BASE = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def rule_prog(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("map_evidence_rule_" + request.param)
    exe = str(d / "test_map_evidence_rule")
    if request.param == "plain":
        subprocess.check_call(BASE + ["-O2", SRC, "-o", exe])
        return exe
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtime")
    subprocess.check_call(BASE + san + [SRC, "-o", exe])              # a stand-alone program: never loaded into Python
    return exe


def _bits(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def _run(exe, mode, text, tmp_path):
    f = tmp_path / (mode + ".txt")
    f.write_text(text)
    r = subprocess.run([exe, mode, str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.split("\n")[:-1]


def _rows_case(exe, tmp_path, rows, mn, log2):
    rows = np.asarray(rows, np.float32).reshape(-1, 3)
    text = "%s %d %d\n" % (_bits(mn), log2, rows.shape[0]) + "".join(" ".join(_bits(v) for v in r) + "\n" for r in rows)
    got = _run(exe, "rows", text, tmp_path)
    part, pix, word = em.scan_rows(rows, mn, log2)
    assert len(got) == rows.shape[0]
    for i, line in enumerate(got):
        p, x, w = line.split()
        want = (1, int(pix[i]), int(word[i])) if part[i] else (0, 0, 0)
        assert (int(p), int(x), int(w, 16)) == want, (i, rows[i], mn, log2)
    return int(part.sum())


def test_rows_equal_the_model_on_the_direction_table_and_on_random_rows(rule_prog, tmp_path):
    table = cases.direction_rows()
    for log2 in (4, 5, 8, 10):
        assert _rows_case(rule_prog, tmp_path, table, 0.0, log2) == table.shape[0]
    rs = np.random.RandomState(33)
    rows = (rs.randn(3000, 3) * [20, 20, 3]).astype(np.float32)
    rows[::97, 1] = np.nan; rows[5::101, 0] = np.inf; rows[7::89, 2] = 0.0; rows[11::83, :2] = 0.0
    assert _rows_case(rule_prog, tmp_path, rows, 0.0, 8) > 2800
    assert 500 < _rows_case(rule_prog, tmp_path, rows, 20.0, 7) < 2500
    assert _rows_case(rule_prog, tmp_path, (rows * np.float32(1e30)).astype(np.float32), 0.0, 10) > 2800
    assert _rows_case(rule_prog, tmp_path, (rows * np.float32(1e-32)).astype(np.float32), 0.0, 4) > 2800
    assert _rows_case(rule_prog, tmp_path, [[3, 4, 0], [3, 4, 0.01], [0, 0, 0]], 5.0, 8) == 1


def _cells_case(exe, tmp_path, cents, poses, near, cell=0.1, mn=0.0, mx=40.0, mg=0.3, log2=8):
    cents = np.asarray(cents, np.float32).reshape(-1, 3); poses = np.asarray(poses, np.float32).reshape(-1, 16); near = np.asarray(near, np.uint32).reshape(-1)
    lines = ["%s %s %s %s %d %d" % (_bits(cell), _bits(mn), _bits(mx), _bits(mg), log2, cents.shape[0])]
    for m, T, w in zip(cents, poses, near):
        lines.append(" ".join(_bits(v) for v in list(T) + list(m)) + " %08x" % int(w))
    got = _run(exe, "cells", "\n".join(lines) + "\n", tmp_path)
    assert len(got) == cents.shape[0]
    seen = np.zeros(4, np.int64)
    for i, line in enumerate(got):
        ok, part, pix, cls = (int(v) for v in line.split())
        T = poses[i].reshape(4, 4)
        assert ok == int(qm.pose_ok(T)), (i, T)
        if not ok:
            assert (part, pix, cls) == (0, 0, 0)
            continue
        wp, wpix, d2 = em.cell_pixels(cents[i:i + 1], T, mn, mx, log2)
        assert part == int(wp[0]), (i, cents[i], T)
        if part:
            want = int(em.classes(d2, near[i:i + 1], mg)[0])
            assert (pix, cls) == (int(wpix[0]), want), (i, cents[i], T, near[i])
            seen[want] += 1
    return seen


def test_cells_equal_the_model_on_random_cells_poses_and_near_words(rule_prog, tmp_path):
    rs = np.random.RandomState(34)
    n = 3000
    cents = (rs.randn(n, 3) * [20, 20, 2]).astype(np.float32)
    poses = [mm.pose(t=rs.randn(3) * 10, r=rs.randn(3) * [0.3, 0.3, 3.0]) for _ in range(n)]
    # near words around the cell's own range, so that every class occurs; some empty, some +inf
    rc = np.array([np.sqrt(em.cell_pixels(cents[i:i + 1], poses[i], 0.0, 1e9, 8)[2][0]) for i in range(n)])
    near = (rc + rs.uniform(-0.6, 0.6, n)).astype(np.float32).view(np.uint32).copy()
    near[::13] = em.EMPTY; near[5::17] = 0x7F800000
    seen = _cells_case(rule_prog, tmp_path, cents, poses, near)
    assert (seen > 100).all(), seen
    seen = _cells_case(rule_prog, tmp_path, cents, poses, near, mn=5.0, mx=30.0, mg=0.0, log2=4)
    assert seen[1:].sum() > 500
    # matrices that are no rotations (R is the caller's), large coordinates, and non-finite poses
    bad = [rs.randn(4, 4).astype(np.float32) * 3 for _ in range(n)]
    assert _cells_case(rule_prog, tmp_path, cents * 1000, bad, near, mx=1e6, log2=10)[1:].sum() > 500
    nf = []
    for j in range(16):
        for v in (np.nan, np.inf, -np.inf):
            T = mm.pose(t=(1, 2, 3), r=(0.1, 0.2, 0.3)); T.reshape(-1)[j] = v
            nf.append(T)
    _cells_case(rule_prog, tmp_path, cents[:48], nf, near[:48])


def test_cells_equal_the_model_on_the_tie_table(rule_prog, tmp_path):
    pt, table = cases.tie_cases()
    for c in table:
        row = np.array([c["scan_row"]], np.float32)
        part, pix, word = em.scan_rows(row, c["mn"], 8)
        cell_pix = em.cell_pixels(pt, mm.pose(), c["mn"], c["mx"], 8)[1][0]
        near = word if part[0] and pix[0] == cell_pix else np.array([em.EMPTY], np.uint32)      # (window 0: the pixel's own word)
        seen = _cells_case(rule_prog, tmp_path, pt, [mm.pose()], near, cell=0.125, mn=c["mn"], mx=c["mx"], mg=c["mg"])
        got = "miss" if seen[em.MISS] else ("agree" if seen[em.AGREE] else "none")
        assert got == c["want"], c


def test_near_image_and_decision_equal_the_model(rule_prog, tmp_path):
    rs = np.random.RandomState(35)
    for log2, window in ((4, 0), (4, 1), (4, 2), (5, 2), (6, 1)):
        W = 1 << log2
        img = np.where(rs.rand(W, W) < 0.2, rs.uniform(1, 50, (W, W)).astype(np.float32).view(np.uint32), em.EMPTY).astype(np.uint32)
        img[0, 0] = 0x40400000; img[W - 1, W - 1] = 0x40000000; img[0, W - 1] = 0x3F800000      # the corners
        got = _run(rule_prog, "near", "%d %d\n" % (log2, window) + "\n".join("%08x" % int(w) for w in img.reshape(-1)) + "\n", tmp_path)
        assert [int(v, 16) for v in got] == em.near_image(img, window).reshape(-1).tolist(), (log2, window)
    big = 2 ** 31 - 1
    quads = [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(rs.randint(0, 50, 500), rs.randint(0, 50, 500), rs.randint(0, 5, 500), rs.randint(0, 4, 500))]
    quads += [(big, 2, 1, 2 ** 30), (big, 1, 1, 2 ** 30), (big, big, 1, big), (big, big, 0, 0), (big, 3, big, big // 3), (big, 3, big, big // 3 + 1), (0, 0, 0, 0), (1, 0, 0, 0),
              (1, big, 1, big), (70000, 65536, 2, 65536), (2 ** 20, 2 ** 11 - 1, 1, 2 ** 9), (2 ** 20, 2 ** 11, 1, 2 ** 9)]
    got = _run(rule_prog, "decide", "".join("%d %d %d %d\n" % q for q in quads), tmp_path)
    want = [int(em.decide([q[0]], [q[1]], q[2], q[3])[0]) for q in quads]
    assert [int(v) for v in got] == want and 100 < sum(want) < len(want) - 100


def test_parameters_and_the_pruning_interval(rule_prog, tmp_path):
    ok = (0.0, 40.0, 0.3, 8, 1, 2, 1, 0)
    table = [(ok, 1), ((0.5, 1e-3, 0.0, 4, 0, 0, 0, 0), 1), ((-1.0, 5.0, 0.0, 10, 2, 7, 9, 0), 1)]
    for j, v in ((0, np.nan), (0, np.inf), (1, np.nan), (1, np.inf), (1, 0.0), (1, -1.0), (2, np.nan), (2, np.inf), (2, -0.1), (3, 3), (3, 11), (4, -1), (4, 3), (5, -1), (6, -1),
                 (7, 1), (7, 2), (7, -1)):
        c = list(ok); c[j] = v
        table.append((tuple(c), 0))
    got = _run(rule_prog, "params", "".join("%s %s %s %d %d %d %d %d\n" % ((_bits(c[0]), _bits(c[1]), _bits(c[2])) + tuple(c[3:])) for c, _ in table), tmp_path)
    assert [int(v) for v in got] == [w for _, w in table]
    # the run of x cells: the query's for a rotation; everything for a matrix that is none (same bits, no pruning); empty for an unusable pose
    rs = np.random.RandomState(36)
    rots = [mm.pose(t=rs.randn(3) * 30, r=rs.randn(3)) for _ in range(20)]
    scaled = [T.copy() for T in rots[:5]]
    for T in scaled:
        T[:3, :3] *= 0.5
    nan = mm.pose(); nan[0, 1] = np.nan
    items = [(c, mx, p, T) for T in rots + scaled + [nan] for c in (0.1, 0.125) for mx in (5.0, 40.0) for p in (1, 0)]
    got = _run(rule_prog, "interval", "".join("%s %s %d %s\n" % (_bits(c), _bits(mx), p, " ".join(_bits(v) for v in T.reshape(-1))) for c, mx, p, T in items), tmp_path)
    lim = 1 << 20
    for line, (c, mx, p, T) in zip(got, items):
        is_rot = any(T is r for r in rots)
        want = qm.x_interval(T, c, mx, bool(p) and is_rot)
        assert tuple(int(v) for v in line.split()) == want, (c, mx, p, T)
        if is_rot and p:
            assert -lim < want[0] < want[1] < lim


def test_evidence_entry_points_are_exported_and_refuse_null():
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    e = api.MapEvidence(0.0, 40.0, 0.3, 8, 1, 2, 1, 0)
    s = api.MapEvidenceStats()
    T = np.eye(4, dtype=np.float32)
    rows = C.c_int64(-1)
    assert lib.icet_voxel_map_evidence_device(None, 0, None, None, C.byref(e), C.byref(s)) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_evidence_device(None, 1, None, T.ctypes.data, C.byref(e), None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_evidence_posed_device(None, 0, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_evidence_fetch_device(None, None, None, None, 0, C.byref(rows)) == api.ICET_ERR_BAD_ARG
    assert rows.value == -1 and api.VOXEL_MAP_QUERY_STATIC == 2


def test_evidence_record_sizes_match_the_ctypes_mirrors(tmp_path):
    from icet_amd import api
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icet_hip.h"\nint main(void){ printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d\\n", '
                   '(int)sizeof(icet_voxel_map_evidence), (int)offsetof(icet_voxel_map_evidence, margin), (int)offsetof(icet_voxel_map_evidence, image_log2), '
                   '(int)offsetof(icet_voxel_map_evidence, window), (int)offsetof(icet_voxel_map_evidence, min_miss), (int)offsetof(icet_voxel_map_evidence, agree_factor), '
                   '(int)offsetof(icet_voxel_map_evidence, flags), (int)sizeof(struct icet_voxel_map_evidence_stats), (int)offsetof(struct icet_voxel_map_evidence_stats, cells), '
                   '(int)offsetof(struct icet_voxel_map_evidence_stats, cells_transient), (int)offsetof(struct icet_voxel_map_evidence_stats, scans_used), '
                   '(int)offsetof(struct icet_voxel_map_evidence_stats, scans_bad_pose), (int)offsetof(struct icet_voxel_map_evidence_stats, reserved), '
                   'ICET_VOXEL_MAP_QUERY_STATIC); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
    E, S = api.MapEvidence, api.MapEvidenceStats
    assert got == [C.sizeof(E), E.margin.offset, E.image_log2.offset, E.window.offset, E.min_miss.offset, E.agree_factor.offset, E.flags.offset, C.sizeof(S), S.cells.offset,
                   S.cells_transient.offset, S.scans_used.offset, S.scans_bad_pose.offset, S.reserved.offset, api.VOXEL_MAP_QUERY_STATIC]
    assert got[0] == 32 and got[7] == 32
