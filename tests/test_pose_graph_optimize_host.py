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
    items.append((("seam",), pc.seam_graph(), {}))
    items.append((("pcg_tol",), pc.graph(33, pc.CASES[4][1], None, True), dict(pcg_tol=1e-4)))
    items.append((("stalled",), pc.stalled_graph(), {}))
    items.append((("negative",), pc.negative_graph(), {}))
    items.append((("negative_cg",), pc.negative_graph(0.1), {}))
    items.append((("strong",), pc.strong_graph(), dict(max_pcg=100)))
    items.append((("strong_default",), pc.strong_graph(), dict(gn_iters=30)))
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
    by_key = {key[0]: r for (key, _, _), r in zip(items, res)}
    for (key, g, o), r in zip(items, res):
        m = pc.model(key, g, **pc.model_options(o))
        if key[0] == "strong_default":
            # the finding of DESIGN.md section 20: the default cap makes every step inexact, the run takes more iterations to the same optimum
            print(key, "iterations", r["gn_iterations"], "| the model", m["gn_iterations"], "band solves", r["pcg_iterations"], "status", r["status"])
            assert r["status"] == pgm.CONVERGED and r["gn_iterations"] > by_key["strong"]["gn_iterations"]
            continue
        if key[0] in ("zero_row", "nan", "negative", "negative_cg"):
            print(key, "status", r["status"], "|", m["status"], "iterations", r["gn_iterations"], "|", m["gn_iterations"])
            assert r["status"] == m["status"] == (pgm.NON_FINITE if key[0] == "nan" else pgm.NOT_POSITIVE_DEFINITE)
            assert r["gn_iterations"] == m["gn_iterations"] == (0 if key[0] == "nan" else 1)
            assert key[0] not in ("negative", "negative_cg") or (r["pcg_iterations"] > 0) == (key[0] == "negative_cg")      # a band pivot | p.Hp <= 0
            assert np.array_equal(r["poses"].view(np.uint32), np.asarray(g["poses"], np.float32).view(np.uint32))
            assert np.array_equal(r["edge_chi2"][0], r["edge_chi2"][1], equal_nan=True) and (r["chi2_final"] == r["chi2_initial"] or key[0] == "nan")
            continue
        pc.compare(str(key[:2]), r, m, g)
        if key[0] == "cap":
            assert r["status"] == pgm.ITERATION_CAP and r["gn_iterations"] == 1
        if key[0] == "chain":
            assert r["pcg_iterations"] == r["gn_iterations"]
        if key[0] == "stalled":
            assert r["status"] == m["status"] == pgm.STALLED and r["gn_iterations"] == m["gn_iterations"] == 2
        if key[0] == "pcg_tol":
            default = next(x for (k, _, _), x in zip(items, res) if k[:2] == ("loop", 33) and k[4])          # the same graph at the default pcg_tol
            print("    pcg_tol 1e-4: %d band solves in %d iterations (default: %d in %d)" % (r["pcg_iterations"], r["gn_iterations"], default["pcg_iterations"], default["gn_iterations"]))
            assert r["status"] == pgm.CONVERGED and r["pcg_iterations"] <= default["pcg_iterations"]
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
    # the step hook: exported, refuses a null context, and its struct has the header's layout (twelve pointers, eight int32, three doubles)
    assert "icet_debug_pose_graph_step" in api.EXPORTED_SYMBOLS and lib.icet_debug_pose_graph_step is not None
    assert lib.icet_debug_pose_graph_step(None, 1, None, None, None, 0, None, None, None, None, None, None, 0, None, None) == api.ICET_ERR_BAD_ARG
    assert C.sizeof(api.PoseGraphStep) == 152 and api.PoseGraphStep.cg_capacity.offset == 96 and api.PoseGraphStep.chi2_start.offset == 128
