"""CPU tests of the voxel map's shape (include/icet_hip.h icet_voxel_map_enable_shape / extract_shape): the header the kernels compile
(icet_amd/csrc/icet_map_shape.h), built with g++ into a stand-alone program (tests/cpp/test_map_shape_rule.cpp), equals the NumPy model (tests/map_shape_model.py)
on every row and every table; the entry points are exported and refuse NULL; the record has the size and the offsets of its ctypes mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_model as mm
import map_shape_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icet_voxel_map_enable_shape", "icet_voxel_map_extract_shape_device", "icet_voxel_map_extract_shape")
SRC = os.path.join(ROOT, "tests", "cpp", "test_map_shape_rule.cpp")


@pytest.fixture(scope="module")
def rule_prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_shape_rule") / "test_map_shape_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", SRC, "-o", exe])
    return exe


def _bits(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def _bits64(v):
    return "%016x" % int(np.float64(v).view(np.uint64))


def _run(exe, mode, text, tmp_path):
    f = tmp_path / (mode + ".txt")
    f.write_text(text)
    return subprocess.check_output([exe, mode, str(f)]).decode().split("\n")[:-1]


def _rows_case(exe, tmp_path, rows, poses, cell, mn=0.0, mx=0.0):
    """rows (N x 3), poses (N x 4 x 4): the program's class, h and nine increments per row against the model's."""
    rows = np.asarray(rows, np.float32); poses = np.asarray(poses, np.float32).reshape(-1, 16)
    lines = ["%s %s %s %d" % (_bits(cell), _bits(mn), _bits(mx), rows.shape[0])]
    for p, T in zip(rows, poses):
        lines.append(" ".join(_bits(v) for v in list(T) + list(p)))
    got = _run(exe, "rows", "\n".join(lines) + "\n", tmp_path)
    assert len(got) == rows.shape[0]
    kept = 0
    for i, line in enumerate(got):
        cls, _, q, _ = mm.classify(rows[i:i + 1], poses[i].reshape(4, 4), cell, mn, mx)
        want = [int(cls[0])] + [0] * 12
        if cls[0] == mm.KEPT:
            h = [int(v) >> 16 for v in q[0]]
            want = [mm.KEPT] + h + [int(v) for v in sm.row_moments(q)[0]]
            assert all(0 <= v <= 65535 for v in h) and want[4:7] == h
            kept += 1
        assert [int(v) for v in line.split()] == want, (i, rows[i], poses[i])
    return kept


@pytest.mark.parametrize("cell", [0.1, 0.5])
def test_header_equals_the_model_on_every_row(rule_prog, tmp_path, cell):
    rows, poses = [], []
    for r, T, _ in mm.edge_rows(cell):
        for p in r:
            rows.append(p); poses.append(T)
    assert _rows_case(rule_prog, tmp_path, rows, poses, cell) >= 16
    r, _ = mm.range_rows()
    assert _rows_case(rule_prog, tmp_path, r, [mm.pose()] * len(r), cell, 5.0, 13.0) == 2
    rs = np.random.RandomState(21)
    rows = (rs.randn(2000, 3) * [30, 30, 3]).astype(np.float32)
    poses = [mm.pose(t=rs.randn(3) * 50, r=rs.randn(3) * [0.05, 0.05, 3.0]) for _ in range(2000)]
    assert _rows_case(rule_prog, tmp_path, rows, poses, cell) == 2000


def _cov_cases():
    """(cell, n, nine words): cells of real rows, one row at the offsets 0 and 65535, counts up to 2^32 with M near 2^63 and above, words of a half-removed cell."""
    rs = np.random.RandomState(22)
    cases = []
    for cell in (0.1, 0.5, 0.37):
        m = sm.ShapeMap(cell).add([(rs.randn(3000, 3) * [3, 3, 0.4]).astype(np.float32)], [mm.pose(t=(0.3, -0.2, 0.1), r=(0.01, 0.02, 0.3))])
        cases += [(cell, m.cells[k][0], m.words(k)) for k in sorted(m.mom)]
        for h in (0, 1, 65535):
            cases.append((cell, 1, [h, h, h] + [h * h] * 6))
        cases.append((cell, 1, [0, 65535, 1, 0, 0, 0, 65535 * 65535, 65535, 1]))
        for n in (2, 3, 1000, (1 << 31) + 12345, (1 << 32) - 1):
            for _ in range(6):                                       # n rows spread over a few offsets: exact integer words of any size
                hs = rs.randint(0, 65536, size=(4, 3)); hs[0] = [65535, 0, 65535]
                cnt = [n // 4 + (1 if j < n % 4 else 0) for j in range(4)]
                w = [sum(c * int(h[a]) for c, h in zip(cnt, hs)) for a in range(3)]
                w += [sum(c * int(h[a]) * int(h[b]) for c, h in zip(cnt, hs)) for a, b in sm.PAIRS]
                cases.append((cell, n, w))
        n = (1 << 32) - 1
        cases.append((cell, n, [n * 65535] * 3 + [n * 65535 * 65535] * 6))      # every row at the largest offset: M = 1.8e19, above 2^63
        cases.append((cell, 1 << 31, [(1 << 31) * 65535] * 3 + [(1 << 31) * 65535 * 65535] * 6))      # M just below 2^63
        cases.append((cell, 5, [(-7) & sm.MASK, 3, 9, (-50) & sm.MASK, 4, 5, 6, 7, 8]))      # (words read as uint64 whatever they mean)
    assert any((1 << 62) < c[2][3] < (1 << 63) for c in cases) and any(c[2][3] > (1 << 63) for c in cases)
    return cases


def test_cov_equals_the_model_bit_for_bit(rule_prog, tmp_path):
    cases = _cov_cases()
    got = _run(rule_prog, "cov", "".join("%s %d %s\n" % (_bits(c), n, " ".join(str(int(v)) for v in w)) for c, n, w in cases), tmp_path)
    assert len(got) == len(cases) > 1000
    for line, (cell, n, w) in zip(got, cases):
        C6 = sm.cov(n, w, cell)
        want = [_bits(v) for v in C6.astype(np.float32)] + [_bits64(v) for v in C6]
        assert line.split() == want, (cell, n, w)
        if n == 1:
            assert not C6.any()


def test_eigen_equals_the_model_bit_for_bit(rule_prog, tmp_path):
    rs = np.random.RandomState(23)
    ex = sm.ShapeMap(0.5).add([sm.plane_rows(6000)], [mm.pose()]).extract_shape()
    mats = [C for C in ex["cov64"]]
    for _ in range(200):                                              # random symmetric matrices, some indefinite, some with zeros off the diagonal
        C = rs.randn(6) * 10.0 ** rs.randint(-8, 3)
        C[rs.rand(6) < 0.15] = 0.0
        mats.append(C)
    mats += [np.zeros(6), np.array([1.0, 1e-300, 0, 3, 0, 2]), np.array([2.0, 0, 0, 1, 0, 1]), np.array([1.0, -1, 0, 1, 0, 5]), np.array([1.0, 1, 1, 1, 1, 1])]
    got = _run(rule_prog, "eigen", "".join(" ".join(_bits64(v) for v in C) + "\n" for C in mats), tmp_path)
    assert len(got) == len(mats) > 300
    for line, C in zip(got, mats):
        ev, n = sm.eigen(C)
        assert line.split() == [_bits(v) for v in list(ev) + list(n)], C


def test_the_program_is_clean_under_the_address_and_undefined_sanitizers(tmp_path):
    """The stand-alone program alone, built with -fsanitize=address,undefined, on the edge rows and the extreme tables."""
    exe = str(tmp_path / "test_map_shape_rule_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe],
                       stderr=subprocess.PIPE)
    if r.returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime: " + r.stderr.decode()[-200:])
    cases = _cov_cases()[-40:]
    got = _run(exe, "cov", "".join("%s %d %s\n" % (_bits(c), n, " ".join(str(int(v)) for v in w)) for c, n, w in cases), tmp_path)
    assert len(got) == len(cases)
    rows, poses = [], []
    for r_, T, _ in mm.edge_rows(0.1):
        for p in r_:
            rows.append(p); poses.append(T)
    assert _rows_case(exe, tmp_path, rows, poses, 0.1) >= 16
    got = _run(exe, "eigen", " ".join(_bits64(v) for v in (1.0, 1e-300, 0, 3, 0, 2)) + "\n", tmp_path)
    assert len(got) == 1


def test_shape_entry_points_are_exported_and_refuse_null():
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    s = api.MapStats()
    sh = api.MapShape(None, None, None, None, 0, 0, 0)
    assert lib.icet_voxel_map_enable_shape(None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_extract_shape_device(None, 1, None, 0, 0, None, None, C.byref(sh), C.byref(s)) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_extract_shape(None, 1, None, 0, 0, None, None, C.byref(sh), C.byref(s)) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_extract_shape(None, 1, None, 0, 0, None, None, None, None) == api.ICET_ERR_BAD_ARG


def test_shape_record_size_and_offsets_match_the_ctypes_mirror(tmp_path):
    from icet_amd import api
    fields = ("cov", "normal", "evals", "moments", "ld", "flags", "reserved")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icet_hip.h"\nint main(void){ printf("%d", (int)sizeof(icet_voxel_map_shape));\n'
                   + "".join('printf(" %%d", (int)offsetof(icet_voxel_map_shape, %s));\n' % f for f in fields) + 'printf("\\n"); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
    assert got == [C.sizeof(api.MapShape)] + [getattr(api.MapShape, f).offset for f in fields]
    assert got == [48, 0, 8, 16, 24, 32, 40, 44]
