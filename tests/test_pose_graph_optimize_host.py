"""CPU tests of the pose-graph optimiser (-m "not gpu"): the WHOLE optimiser -- the driver of icet_posegraph_driver.h over the bodies of icet_posegraph_body.h --
run on the host by tests/cpp/test_posegraph_optimize.cpp against heap blocks of the exact sizes, plain, under the address and undefined-behaviour sanitizers,
and with a workgroup of four real threads; its results against the NumPy model.  And the ABI of the two entry points that needs no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_model as pgm      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _items():
    items = []
    for (n, pairs, fx) in pc.CASES:
        for noisy in (True, False):
            if n == 257 and not noisy:
                continue          # (the model takes seconds there; the noisy graph covers the sizes)
            g = pc.graph(n, pairs, fx, noisy)
            items.append((("loop", n, pairs, fx, noisy), g, {}))
    items.append((("chain", 65), dict(pgm.make_loop(65, [], seed=11), fixed=None), {}))
    items.append((("rank5",), pc.rank5_graph(), {}))
    items.append((("zero_row",), pc.zero_row_graph(), {}))
    items.append((("nan",), pc.nan_graph(), {}))
    items.append((("cap",), pc.graph(33, pc.CASES[4][1], None, True), dict(gn_iters=1)))
    items.append((("damped",), pc.graph(33, pc.CASES[4][1], None, True), dict(damping=1e-3)))
    items.append((("single",), dict(pgm.make_loop(1, [], seed=11), fixed=None), {}))
    return items


def test_whole_optimiser_on_the_host(tmp_path):
    """Built like test_host_side_of_the_device_code builds test_posegraph.cpp.  The one-thread and the four-thread workgroup must write the same bytes (the
    reductions have one order for any thread count), the sanitised build must end clean, and the results must agree with pgm.optimise under the tolerances of
    tests/pose_graph_cases.py."""
    src = os.path.join(ROOT, "tests", "cpp", "test_posegraph_optimize.cpp")
    items = _items()
    fin = str(tmp_path / "graphs.bin")
    pc.write_graphs(fin, [(g, o) for _, g, o in items])
    outs = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                        ("emu", ["-O2", "-DICET_PG_EMU", "-pthread"]), ("emu_san", ["-O1", "-g", "-DICET_PG_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("test_posegraph_optimize_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", ROOT, src, "-o", exe])
        fout = str(tmp_path / (name + ".bin"))
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        outs[name] = open(fout, "rb").read()
        if name == "plain":
            print(r.stdout)
    assert outs["plain"] == outs["san"] == outs["emu"] == outs["emu_san"]
    res = pc.read_results(str(tmp_path / "plain.bin"), [(g, o) for _, g, o in items])
    for (key, g, o), r in zip(items, res):
        m = pc.model(key, g, **o)
        if key[0] in ("zero_row", "nan"):
            print(key, "status", r["status"], "|", m["status"], "iterations", r["gn_iterations"], "|", m["gn_iterations"])
            assert r["status"] == m["status"] == (pgm.NOT_POSITIVE_DEFINITE if key[0] == "zero_row" else pgm.NON_FINITE)
            assert r["gn_iterations"] == m["gn_iterations"] == (1 if key[0] == "zero_row" else 0)
            assert np.array_equal(r["poses"].view(np.uint32), np.asarray(g["poses"], np.float32).view(np.uint32))
            assert np.array_equal(r["edge_chi2"][0], r["edge_chi2"][1], equal_nan=True) and (r["chi2_final"] == r["chi2_initial"] or key[0] == "nan")
            continue
        pc.compare(str(key[:2]), r, m, g)
        if key[0] == "cap":
            assert r["status"] == pgm.ITERATION_CAP and r["gn_iterations"] == 1
        if key[0] == "chain":
            assert r["pcg_iterations"] == r["gn_iterations"]
        if key[0] == "loop" and not key[4] and key[3] is None:
            dt, dr = pgm.pose_error(r["poses"], g["truth"])
            assert dt <= pc.CAP_T and dr <= pc.CAP_R


def test_abi_of_the_optimiser():
    import icet_amd
    from icet_amd import api
    lib = icet_amd.load_library()
    for name in ("icet_pose_graph_optimize", "icet_pose_graph_optimize_device"):
        assert name in api.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert getattr(lib, name)(None, 1, None, None, None, 0, None, None, None, None, None, None, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert C.sizeof(api.PoseGraphOptions) == 32 and C.sizeof(api.PoseGraphResult) == 40
