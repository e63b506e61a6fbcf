"""CPU tests of the voxel map's query (include/icet_hip.h icet_voxel_map_query_*): the header the kernels compile
(icet_amd/csrc/icet_map_query.h), built with g++ into a stand-alone program (tests/cpp/test_map_query_rule.cpp), equals the NumPy model
(tests/map_query_model.py) bit for bit; the entry points are exported and refuse NULL; the records have the sizes of their ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_model as mm
import map_query_model as qm
from test_map_query_model import boundary_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icet_voxel_map_index", "icet_voxel_map_query_device", "icet_voxel_map_query_posed_device")


@pytest.fixture(scope="module")
def rule_prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_query_rule") / "test_map_query_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_map_query_rule.cpp"), "-o", exe])
    return exe


def _bits(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def _run(exe, mode, text, tmp_path):
    f = tmp_path / (mode + ".txt")
    f.write_text(text)
    return subprocess.check_output([exe, mode, str(f)]).decode().split("\n")[:-1]


def _cells_case(exe, tmp_path, cents, counts, poses, cell=0.1, mn=0.0, mx=0.0, minp=1, world=False):
    """cents (N x 3 float32), counts (N), poses (N x 4 x 4): the program's (pose_ok, kept, row bits) per line against the model's, each cell as a map of one."""
    cents = np.asarray(cents, np.float32).reshape(-1, 3); poses = np.asarray(poses, np.float32).reshape(-1, 16)
    lines = ["%s %s %s %d %d %d" % (_bits(cell), _bits(mn), _bits(mx), minp, 1 if world else 0, cents.shape[0])]
    for m, n, T in zip(cents, counts, poses):
        lines.append(" ".join(_bits(v) for v in list(T) + list(m)) + " %d" % n)
    got = _run(exe, "cells", "\n".join(lines) + "\n", tmp_path)
    assert len(got) == cents.shape[0]
    kept_any = 0
    for i, line in enumerate(got):
        ext = dict(xyz=cents[i:i + 1], count=np.array([counts[i]], np.int64), key=np.array([7], np.uint64))
        want = qm.query_extract(ext, poses[i].reshape(4, 4), min_range=mn, max_range=mx, min_points=minp, world=world)
        ok, kept, r0, r1, r2 = line.split()
        assert int(ok) == (0 if want["status"] & qm.BAD_POSE else 1), (i, poses[i])
        assert int(kept) == want["total"], (i, cents[i], poses[i])
        if want["total"]:
            kept_any += 1
            assert [int(v, 16) for v in (r0, r1, r2)] == [int(v) for v in want["xyz"].view(np.uint32)[0]], (i, cents[i], poses[i])
        else:
            assert (r0, r1, r2) == ("00000000",) * 3
    return kept_any


def test_header_equals_the_model_on_random_cells_and_poses(rule_prog, tmp_path):
    rs = np.random.RandomState(21)
    n = 3000
    cents = (rs.randn(n, 3) * [20, 20, 2]).astype(np.float32)
    counts = rs.randint(1, 6, n)
    poses = [mm.pose(t=rs.randn(3) * 10, r=rs.randn(3) * [0.3, 0.3, 3.0]) for _ in range(n)]
    assert _cells_case(rule_prog, tmp_path, cents, counts, poses) == n
    k = _cells_case(rule_prog, tmp_path, cents, counts, poses, mn=5.0, mx=30.0, minp=3)
    assert 300 < k < n - 300
    assert 300 < _cells_case(rule_prog, tmp_path, cents, counts, poses, mn=5.0, mx=30.0, minp=2, world=True) < n
    # rotations that are not rotations (R is the caller's), and large coordinates
    bad = [rs.randn(4, 4).astype(np.float32) * 3 for _ in range(n)]
    assert _cells_case(rule_prog, tmp_path, cents * 1000, counts, bad, mx=1e5) > 1000


def test_header_equals_the_model_on_the_boundary_table(rule_prog, tmp_path):
    model, pts = boundary_map()
    ext = model.extract(1)
    I = [mm.pose()] * ext["xyz"].shape[0]
    for kw in (dict(mx=5.0), dict(mn=5.0), dict(mx=13.0), dict(mn=13.0), dict(), dict(mn=5.0, mx=13.0)):
        _cells_case(rule_prog, tmp_path, ext["xyz"], ext["count"], I, cell=0.125, **kw)
    # the classes themselves, through the program: (3, 4, 0) kept at max_range 5 and dropped at min_range 5, one ulp further out flips both
    rows = np.array([pts[0], pts[2], pts[1], pts[3]], np.float32)
    for (mn, mx), want in (((0.0, 5.0), [1, 0, 0, 0]), ((5.0, 0.0), [0, 1, 1, 1]), ((0.0, 13.0), [1, 1, 1, 0]), ((13.0, 0.0), [0, 0, 0, 1])):
        lines = ["%s %s %s 1 0 4" % (_bits(0.125), _bits(mn), _bits(mx))]
        for m in rows:
            lines.append(" ".join(_bits(v) for v in list(mm.pose().reshape(-1)) + list(m)) + " 1")
        got = _run(rule_prog, "cells", "\n".join(lines) + "\n", tmp_path)
        assert [int(l.split()[1]) for l in got] == want, (mn, mx)
    # a centroid exactly at the origin of the query is dropped at min_range 0
    T = mm.pose(t=(0.125, 0, 0))
    assert _cells_case(rule_prog, tmp_path, [[0.125, 0, 0], [0.25, 0, 0]], [1, 1], [T, T], cell=0.125) == 1


def test_header_equals_the_model_on_non_finite_poses(rule_prog, tmp_path):
    rs = np.random.RandomState(22)
    cents, counts, poses = [], [], []
    for j in range(16):
        for v in (np.nan, np.inf, -np.inf):
            T = mm.pose(t=(1, 2, 3), r=(0.1, 0.2, 0.3)); T.reshape(-1)[j] = v
            poses.append(T); cents.append(rs.randn(3) * 5); counts.append(2)
    kept = _cells_case(rule_prog, tmp_path, cents, counts, poses)
    assert kept == 4 * 3                                              # only the last row of T may hold anything
    # the run of x cells: the model's, for usable and unusable poses, pruned and not, with and without a max_range, and at the ends of the key range
    cases = []
    for T in poses[::5] + [mm.pose(t=(t0, 0, 0)) for t0 in (0.0, -3.21, 17.5, 104857.0, -104857.6, 3e5, -3e5, 1e30, -1e30)]:
        for cell in (0.1, 0.125):
            for mx in (0.0, 5.0, 30.0, -1.0, 1e6):
                for prune in (1, 0):
                    cases.append((cell, mx, prune, T))
    text = "".join("%s %s %d %s\n" % (_bits(c), _bits(mx), p, " ".join(_bits(v) for v in T.reshape(-1))) for c, mx, p, T in cases)
    got = _run(rule_prog, "interval", text, tmp_path)
    assert len(got) == len(cases)
    for line, (c, mx, p, T) in zip(got, cases):
        assert tuple(int(v) for v in line.split()) == qm.x_interval(T, c, mx, bool(p)), (c, mx, p, T)


def test_bad_parameters_and_descriptors_are_refused_by_the_rule(rule_prog, tmp_path):
    cases = [((0.0, 0.0, 0, 0, 0, 0, 0), 1), ((0.5, 30.0, 1, 0, 0, 0, 0), 1), ((-1.0, -1.0, 0, 0, 0, 0, 0), 1), ((np.nan, 0.0, 0, 0, 0, 0, 0), 0), ((0.0, np.inf, 0, 0, 0, 0, 0), 0),
             ((0.0, -np.inf, 0, 0, 0, 0, 0), 0), ((0.0, 0.0, 2, 0, 0, 0, 0), 0), ((0.0, 0.0, 3, 0, 0, 0, 0), 0), ((0.0, 0.0, -1, 0, 0, 0, 0), 0), ((0.0, 0.0, 0, 1, 0, 0, 0), 0),
             ((0.0, 0.0, 0, 0, 0, 0, -1), 0)]
    got = _run(rule_prog, "params", "".join("%s %s %d %d %d %d %d\n" % ((_bits(c[0]), _bits(c[1])) + c[2:]) for c, _ in cases), tmp_path)
    assert [int(v) for v in got] == [w for _, w in cases]
    subs = [((0, 0, 0), 1), ((0, 5, 0), 1), ((1, 4, 4), 1), ((1, 9, 4), 1), ((1, 3, 4), 0), ((1, 4, -1), 0), ((0, 4, 4), 0), ((1, -1, 0), 0)]
    assert [int(v) for v in _run(rule_prog, "submap", "".join("%d %d %d\n" % c for c, _ in subs), tmp_path)] == [w for _, w in subs]


def test_query_entry_points_are_exported_and_refuse_null():
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    s = api.MapStats()
    T = np.eye(4, dtype=np.float32)
    q = api.MapQuery(0.0, 0.0, 1, 0)
    o = (api.MapSubmap * 1)(api.MapSubmap(None, 0, 0, None, None))
    rows = C.c_void_p(16)
    assert lib.icet_voxel_map_index(None, C.byref(s)) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_index(None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_query_device(None, 1, T.ctypes.data, C.byref(q), o, rows, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_query_posed_device(None, 1, None, C.byref(q), o, rows, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_query_device(None, 0, None, None, None, None, None, None) == api.ICET_ERR_BAD_ARG


def test_query_record_sizes_match_the_ctypes_mirrors(tmp_path):
    from icet_amd import api
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icet_hip.h"\nint main(void){ printf("%d %d %d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(icet_voxel_map_query), '
                   '(int)offsetof(icet_voxel_map_query, min_points), (int)offsetof(icet_voxel_map_query, flags), (int)offsetof(icet_voxel_map_query, reserved), '
                   '(int)sizeof(icet_voxel_map_submap), (int)offsetof(icet_voxel_map_submap, ld), (int)offsetof(icet_voxel_map_submap, cap_rows), '
                   '(int)offsetof(icet_voxel_map_submap, count), (int)offsetof(icet_voxel_map_submap, key), ICET_VOXEL_MAP_QUERY_CHUNK, ICET_VOXEL_MAP_MAX_QUERIES, '
                   'ICET_VOXEL_MAP_QUERY_BAD_POSE | ICET_VOXEL_MAP_QUERY_WORLD << 8 | ICET_VOXEL_MAP_TRUNCATED << 16); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
    Q, S = api.MapQuery, api.MapSubmap
    assert got == [C.sizeof(Q), Q.min_points.offset, Q.flags.offset, Q.reserved.offset, C.sizeof(S), S.ld.offset, S.cap_rows.offset, S.count.offset, S.key.offset,
                   api.MAP_QUERY_CHUNK, api.VOXEL_MAP_MAX_QUERIES, api.VOXEL_MAP_QUERY_BAD_POSE | api.VOXEL_MAP_QUERY_WORLD << 8 | api.VOXEL_MAP_TRUNCATED << 16]
    assert got[0] == 32 and got[4] == 40
    assert (qm.TRUNCATED, qm.BAD_POSE) == (api.VOXEL_MAP_TRUNCATED, api.VOXEL_MAP_QUERY_BAD_POSE)
