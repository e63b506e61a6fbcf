"""CPU tests of the neighbourhood rule of the registration against a shaped voxel map (include/icet_hip.h ICET_VOXEL_MAP_REG_NEIGHBOURS_*): the
header the kernels compile (icet_amd/csrc/icet_map_register.h), built with g++ into a stand-alone program (tests/cpp/test_map_register_neighbours.cpp), equals the
NumPy model (tests/map_register_neighbours_model.py) bit for bit on the selection and the terms of every row -- the named rows, the rows at the edge of the grid,
the tie -- and on a whole call run on the CPU, for 7 and 27 cells; the same program is clean under the address and undefined-behaviour sanitizers; a C99 program
compiles the public header and sees the two new macros."""
import os
import subprocess

import numpy as np
import pytest

import map_model as mm
import map_register_cases as cs
import map_register_model as rm
import map_register_neighbours_cases as nc
import map_register_neighbours_model as nm
import test_map_register_host as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_map_register_neighbours.cpp")
_b32, _b64, _run = th._b32, th._b64, th._run


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_register_neighbours") / "test_map_register_neighbours")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", SRC, "-o", exe])
    return exe


def _rows_case(exe, tmp_path, G, rows, pose, neighbours, scale=11.3449, mn=0.0, mx=0.0):
    """rows (N x 3 float32) at ONE float64 pose: the program's record per row against the model's, word for word.  Returns the model's terms."""
    rows = np.asarray(rows, np.float32).reshape(-1, 3)
    R, t = pose
    lines = ["%s %s %s %s %d %d %d" % (_b32(G.cell), _b32(mn), _b32(mx), _b64(scale), neighbours, G.key.shape[0], len(rows))]
    for k, mu, W in zip(G.key, G.mu, G.W):
        lines.append("%d %s" % (int(k), " ".join(_b64(v) for v in list(mu) + list(W))))
    head = " ".join(_b64(v) for v in list(np.asarray(R).reshape(9)) + list(t))
    lines += [head + " " + " ".join(_b32(v) for v in p) for p in rows]
    got = _run(exe, "rows", "\n".join(lines) + "\n", tmp_path)
    assert len(got) == rows.shape[0]
    tm = nm.row_terms(rows, R, t, G, neighbours, scale, mn, mx)
    for i, line in enumerate(got):
        want = [str(int(tm["cls"][i])), str(int(tm["key"][i])), str(int(tm["place"][i]) + 1)] + [_b64(tm[k][i]) for k in ("s", "omega", "rho")] + [_b64(v) for v in tm["v"][i]]
        assert line.split() == want, (neighbours, i, rows[i])
    return tm


@pytest.mark.parametrize("cell", [0.1, 0.5])
def test_header_equals_the_model_on_selection_and_terms(prog, tmp_path, cell):
    G = rm.Gaussians(nc.model_map(cell))
    rows = cs.term_rows(cell, 600)
    own = _rows_case(prog, tmp_path, G, rows, rm.pose64(cs.POSE), 1)
    assert np.array_equal(own["place"], np.where(own["matched"], 0, -1))
    seen = {}
    for nb in (7, 27):
        for mn, mx in ((0.05, 30.0), (0.0, 0.0)):
            tm = _rows_case(prog, tmp_path, G, rows, rm.pose64(cs.POSE), nb, mn=mn, mx=mx)
        seen[nb] = set(int(p) for p in tm["place"])
        assert mm.OUTSIDE in tm["cls"] and mm.NONFINITE in tm["cls"] and tm["place"][tm["cls"] != mm.KEPT].max() == -1
        edge = _rows_case(prog, tmp_path, G, nc.edge_case(cell)[1], rm.pose64(mm.pose()), nb)
        assert list(edge["place"]) == ([2, 1, 4, 3, 6, 5, -1] if nb == 7 else [22, 5, 16, 11, 14, 13, -1])
        assert list(edge["cls"]) == [mm.KEPT] * 6 + [mm.OUTSIDE]
    assert seen[7] == set(range(-1, 7)) and len(seen[27]) >= 20       # every place of N7 wins somewhere, and most of N27's


def test_header_equals_the_model_on_the_tie(prog, tmp_path):
    G = rm.Gaussians(nc.tie_map(), **nc.TIE_PARAMS)
    _, rows, want = nc.tie_case()
    for col, nb in enumerate((7, 27)):
        tm = _rows_case(prog, tmp_path, G, rows, rm.pose64(mm.pose()), nb)
        assert list(tm["place"]) == [w[col] for w in want]
        assert list(tm["s"]) == [64.0, 64.0, 16.0]


def _check_loop(exe, tmp_path, P, neighbours, cell=0.5):
    m = nc.model_map(cell)
    G = rm.Gaussians(m, P["sigma_min"], P["min_points"])
    queries = th._loop_queries() + [(nc.edge_case(cell)[1], mm.pose())]
    text = th._loop_text(m, queries, P)
    head, rest = text.split("\n", 1)
    got = _run(exe, "loop", head + " %d\n" % neighbours + rest, tmp_path)
    assert len(got) == len(queries)
    recs = []
    for line, (scan, T) in zip(got, queries):
        r = nm.register(scan, T, G, neighbours, order="chunks", **P)
        want = [str(r[k]) for k in ("status", "iterations", "accepted", "rows_scored", "rows_matched")] + [_b32(v) for v in r["pose"].reshape(16)]
        want += [_b64(r[k]) for k in ("cost", "cost_start", "lambda")] + [_b64(v) for v in list(r["g"]) + list(r["info"])]
        assert line.split() == want, (neighbours, T, r)
        recs.append(r)
    return recs


@pytest.mark.parametrize("neighbours", [7, 27])
def test_the_whole_loop_on_the_cpu_equals_the_model_bit_for_bit(prog, tmp_path, neighbours):
    recs = _check_loop(prog, tmp_path, rm.params(max_iters=30), neighbours)
    own = _check_loop(prog, tmp_path, rm.params(max_iters=0, min_matched=10), 1)
    assert [r["status"] for r in recs[2:5]] == [rm.NO_OVERLAP, rm.NO_OVERLAP, rm.BAD_POSE]
    assert recs[0]["accepted"] >= 3 and recs[0]["cost"] < recs[0]["cost_start"]
    scored = _check_loop(prog, tmp_path, rm.params(max_iters=0, min_matched=10), neighbours)
    for a, b in zip(scored, own):                                      # a neighbourhood scores the same rows, matches no fewer and costs no more
        assert a["rows_scored"] == b["rows_scored"] and a["rows_matched"] >= b["rows_matched"] and (a["cost"] <= b["cost"] or b["status"] == rm.BAD_POSE)
    assert scored[0]["rows_matched"] > own[0]["rows_matched"] and scored[-1]["rows_matched"] == 6 and own[-1]["rows_matched"] == 0


def test_the_program_is_clean_under_the_address_and_undefined_sanitizers(tmp_path):
    """The stand-alone program alone, built with -fsanitize=address,undefined: the whole loop against exact-size buffers, the rows at the edge of the grid (their
    outer neighbours have no key), the tie."""
    exe = str(tmp_path / "test_map_register_neighbours_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe],
                       stderr=subprocess.PIPE)
    if r.returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime: " + r.stderr.decode()[-200:])
    for nb in (7, 27):
        _check_loop(exe, tmp_path, rm.params(max_iters=4), nb)
        G = rm.Gaussians(nc.model_map(0.1))
        _rows_case(exe, tmp_path, G, cs.term_rows(0.1, 64), rm.pose64(cs.POSE), nb)
        _rows_case(exe, tmp_path, G, nc.edge_case(0.1)[1], rm.pose64(mm.pose()), nb)
        _rows_case(exe, tmp_path, rm.Gaussians(nc.tie_map(), **nc.TIE_PARAMS), nc.tie_case()[1], rm.pose64(mm.pose()), nb)


def test_flags_name_one_neighbourhood_or_none(prog):
    got = [int(v) for v in subprocess.check_output([prog, "flags"]).decode().split()]
    assert got == [0, 1, 0, 7, 0, 27, 0, 0, 0, 0, 0]                   # flags -1 .. 9: 0, 2 and 4 alone are accepted


def test_a_c99_program_sees_the_new_macros(tmp_path):
    from icet_amd import api
    src = tmp_path / "macros.c"
    src.write_text('#include <stdio.h>\n#include "icet_hip.h"\nint main(void){ printf("%d %d %d\\n", ICET_VOXEL_MAP_REG_NEIGHBOURS_7, ICET_VOXEL_MAP_REG_NEIGHBOURS_27, '
                   '(int)sizeof(icet_voxel_map_register_params)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "macros")])
    assert subprocess.check_output([str(tmp_path / "macros")]).decode().split() == ["2", "4", "72"]
    assert (api.VOXEL_MAP_REG_NEIGHBOURS_7, api.VOXEL_MAP_REG_NEIGHBOURS_27) == (2, 4)
    assert [api.map_register_params(neighbours=n).flags for n in (1, 7, 27)] == [0, 2, 4] and api.map_register_params().flags == 0
    assert api.map_register_params(flags=4).flags == 4 and set(api.MAP_REGISTER_DEFAULTS) == set(rm.DEFAULTS)
    for bad in (0, 3, 26, "7", None):
        with pytest.raises(ValueError):
            api.map_register_params(neighbours=bad)
