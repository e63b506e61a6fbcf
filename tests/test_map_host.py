"""CPU tests of the voxel map (include/icet_hip.h icet_voxel_map_*): the header the kernels compile (icet_amd/csrc/icet_map.h), built with
g++ into a stand-alone program (tests/cpp/test_map_rule.cpp), equals the NumPy model (tests/map_model.py) on every row; the entry points are exported and
refuse NULL; the records have the sizes of their ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icet_voxel_map_create", "icet_voxel_map_destroy", "icet_voxel_map_last_error", "icet_voxel_map_clear", "icet_voxel_map_add_device",
               "icet_voxel_map_add_posed_device", "icet_voxel_map_stats", "icet_voxel_map_extract_device", "icet_voxel_map_extract")


@pytest.fixture(scope="module")
def rule_prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_rule") / "test_map_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_map_rule.cpp"), "-o", exe])
    return exe


def _bits(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def _run(exe, mode, text, tmp_path):
    f = tmp_path / (mode + ".txt")
    f.write_text(text)
    return subprocess.check_output([exe, mode, str(f)]).decode().split("\n")[:-1]


def _rows_case(exe, tmp_path, rows, poses, cell, mn=0.0, mx=0.0):
    """rows (N x 3), poses (N x 4 x 4): the program's (class, key, q) per row against the model's."""
    rows = np.asarray(rows, np.float32); poses = np.asarray(poses, np.float32).reshape(-1, 16)
    lines = ["%s %s %s %d" % (_bits(cell), _bits(mn), _bits(mx), rows.shape[0])]
    for p, T in zip(rows, poses):
        lines.append(" ".join(_bits(v) for v in list(T) + list(p)))
    got = _run(exe, "rows", "\n".join(lines) + "\n", tmp_path)
    assert len(got) == rows.shape[0]
    for i, line in enumerate(got):
        cls, key, q, _ = mm.classify(rows[i:i + 1], poses[i].reshape(4, 4), cell, mn, mx)
        want = [int(cls[0])] + ([int(key[0])] + [int(v) for v in q[0]] if cls[0] == mm.KEPT else [0, 0, 0, 0])
        assert [int(v) for v in line.split()] == want, (i, rows[i], poses[i])


@pytest.mark.parametrize("cell", [0.125, 0.1])
def test_header_equals_the_model_on_the_edge_table(rule_prog, tmp_path, cell):
    rows, poses = [], []
    for r, T, _ in mm.edge_rows(cell):
        for p in r:
            rows.append(p); poses.append(T)
    _rows_case(rule_prog, tmp_path, rows, poses, cell)
    r, _ = mm.range_rows()
    _rows_case(rule_prog, tmp_path, r, [mm.pose()] * len(r), cell, 5.0, 13.0)


def test_header_equals_the_model_on_random_rows_and_poses(rule_prog, tmp_path):
    rs = np.random.RandomState(5)
    rows = (rs.randn(3000, 3) * [30, 30, 3]).astype(np.float32)
    rows[::11] = 0.0
    poses = [mm.pose(t=rs.randn(3) * 50, r=rs.randn(3) * [0.05, 0.05, 3.0]) for _ in range(3000)]
    _rows_case(rule_prog, tmp_path, rows, poses, 0.1)
    _rows_case(rule_prog, tmp_path, rows, poses, 0.37, 2.0, 40.0)
    # tiny coordinates around the cell borders, where floor and the clamp decide
    tiny = np.array([[s * 10.0 ** -e, 1.0, -1.0] for e in range(20, 46, 3) for s in (1, -1)], np.float32)
    _rows_case(rule_prog, tmp_path, tiny, [mm.pose()] * len(tiny), 0.125)


def test_centroid_equals_the_model_bit_for_bit(rule_prog, tmp_path):
    rs = np.random.RandomState(6)
    cases = []
    for cell in (0.125, 0.1, 0.37):
        for _ in range(300):
            n = int(rs.randint(1, 5000)) if rs.rand() < 0.8 else int(rs.randint(1, 1 << 40))
            mean = int(rs.randint(0, 1 << 32, dtype=np.int64))
            total = n * mean + int(rs.randint(0, n)) if rs.rand() < 0.7 else n * ((1 << 32) - 1)       # (sums above 2^53 round when they become doubles)
            total = min(total, (1 << 64) - 1)
            cases.append((cell, int(rs.randint(-(1 << 20) + 1, 1 << 20)), total, n))
        cases += [(cell, -1, (1 << 32) - 1, 1), (cell, 0, 0, 1), (cell, (1 << 20) - 1, 3 * ((1 << 32) - 1), 3)]
    cases = [c for c in cases if c[2] < c[3] << 32 and c[2] < 1 << 64]
    got = _run(rule_prog, "centroid", "".join("%s %d %d %d\n" % (_bits(c[0]), c[1], c[2], c[3]) for c in cases), tmp_path)
    assert len(got) == len(cases) > 800
    for line, (cell, c, total, n) in zip(got, cases):
        assert int(line, 16) == int(mm.centroid(c, total, n, cell).view(np.uint32)), (cell, c, total, n)


def test_bad_parameters_and_signs_are_refused_by_the_rule(rule_prog, tmp_path):
    cases = [((0.1, 0, 0, 22, 0), 1), ((0.1, 2.0, 80.0, 10, 0), 1), ((0.1, 0, 0, 30, 0), 1), ((0.0, 0, 0, 22, 0), 0), ((-0.1, 0, 0, 22, 0), 0),
             ((np.nan, 0, 0, 22, 0), 0), ((np.inf, 0, 0, 22, 0), 0), ((0.1, np.nan, 0, 22, 0), 0), ((0.1, 0, np.inf, 22, 0), 0), ((0.1, 0, 0, 9, 0), 0),
             ((0.1, 0, 0, 31, 0), 0), ((0.1, 0, 0, -1, 0), 0), ((0.1, 0, 0, 22, 1), 0)]
    got = _run(rule_prog, "params", "".join("%s %s %s %d %d\n" % (_bits(c[0]), _bits(c[1]), _bits(c[2]), c[3], c[4]) for c, _ in cases), tmp_path)
    assert [int(v) for v in got] == [w for _, w in cases]
    signs = [1, -1, 0, 2, -2, 1 << 30]
    assert [int(v) for v in _run(rule_prog, "sign", "".join("%d\n" % s for s in signs), tmp_path)] == [1, 1, 0, 0, 0, 0]
    # a call's scan descriptors (n, ld, has a pointer): n = 0 allowed, ld >= n, n >= 0, rows need a pointer
    scans = [((0, 0, 0), 1), ((0, 5, 0), 1), ((4, 4, 1), 1), ((4, 9, 1), 1), ((4, 3, 1), 0), ((-1, 4, 1), 0), ((4, 4, 0), 0), ((4, 1 << 30, 1), 0)]
    assert [int(v) for v in _run(rule_prog, "scan", "".join("%d %d %d\n" % c for c, _ in scans), tmp_path)] == [w for _, w in scans]


def test_voxel_map_entry_points_are_exported_and_refuse_null():
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    h = C.c_void_p(1)
    p = api.MapParams(0.1, 0.0, 0.0, 22, 0)
    s = api.MapStats()
    T = np.eye(4, dtype=np.float32)
    d = api._dev_scans([(0, 0, 0)])
    assert lib.icet_voxel_map_create(None, C.byref(p), C.byref(h)) == api.ICET_ERR_BAD_ARG and not h.value
    assert lib.icet_voxel_map_create(None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_destroy(None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_clear(None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_last_error(None) == b"null voxel map"
    assert lib.icet_voxel_map_add_device(None, 1, d, T.ctypes.data, 1) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_add_posed_device(None, 1, d, None, 1) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_stats(None, 1, C.byref(s)) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_extract_device(None, 1, None, 0, 0, None, None, C.byref(s)) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_extract(None, 1, None, 0, 0, None, None, C.byref(s)) == api.ICET_ERR_BAD_ARG
    assert np.array_equal(api.voxel_key_cells(np.array([(5 + (1 << 20)) << 42 | ((1 << 20) - 3) << 21 | (1 << 20)], np.uint64)), [[5, -3, 0]])


def test_voxel_map_record_sizes_match_the_ctypes_mirrors(tmp_path):
    from icet_amd import api
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icet_hip.h"\nint main(void){ printf("%d %d %d %d %d %d %d %d\\n", (int)sizeof(icet_voxel_map_params), '
                   '(int)offsetof(icet_voxel_map_params, table_log2), (int)offsetof(icet_voxel_map_params, reserved), (int)sizeof(struct icet_voxel_map_stats), '
                   '(int)offsetof(struct icet_voxel_map_stats, points_dropped), (int)offsetof(struct icet_voxel_map_stats, cells_occupied), '
                   '(int)offsetof(struct icet_voxel_map_stats, status), (int)offsetof(struct icet_voxel_map_stats, reserved)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
    assert got == [C.sizeof(api.MapParams), api.MapParams.table_log2.offset, api.MapParams.reserved.offset, C.sizeof(api.MapStats), api.MapStats.points_dropped.offset,
                   api.MapStats.cells_occupied.offset, api.MapStats.status.offset, api.MapStats.reserved.offset]
    assert got[0] == 32 and got[3] == 64
