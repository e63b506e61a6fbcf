"""CPU tests of the pose-graph optimiser's DIRECT solve (-m "not gpu"): the whole optimiser with it -- pg_optimise_direct of icet_posegraph_driver.h over the bodies
of icet_posegraph_body.h and icet_posegraph_direct.h -- run on the host by tests/cpp/test_posegraph_direct.cpp against heap blocks of the exact sizes: plain, under
the address and undefined-behaviour sanitizers, and with a workgroup of four real threads; its results against the NumPy model pgm.optimise.  The NumPy
restatement of the algorithm (tests/pose_graph_direct_model.py) against the same model.  And the ABI that needs no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_direct_model as pdm      # noqa: E402
import pose_graph_model as pgm      # noqa: E402


def test_whole_optimiser_with_the_direct_solve_on_the_host(tmp_path):
    """Every item of the conjugate-gradient host test's list that a direct run answers, strong at DEFAULT options: pc.compare with pc's tolerances (derived for the
    inexact CG solve; a direct solve is inside them a fortiori), status and gn_iterations the model's, two band solves per iteration where the graph has end nodes
    and one on a chain."""
    items = pdm.whole_run_items()
    fin = str(tmp_path / "graphs.bin")
    pc.write_graphs(fin, [(g, o) for _, g, o in items])
    res = pc.read_results(pdm.build_and_run(tmp_path, fin), [(g, o) for _, g, o in items])
    raw = open(str(tmp_path / "plain.bin"), "rb").read()
    assert int(np.frombuffer(raw, np.int32, 4, 0)[3]) == 1          # result.solver of the first graph
    for (key, g, o), r in zip(items, res):
        pdm.check_whole_run(key, g, o, r)
    by = {key[0]: (g, r) for (key, g, _), r in zip(items, res)}
    assert not pdm.graph_ends(by["chain"][0]) and by["chain"][1]["pcg_iterations"] == by["chain"][1]["gn_iterations"]
    assert by["negative"][1]["pcg_iterations"] == 0 and by["negative_cg"][1]["pcg_iterations"] == 0          # a band pivot | a pivot of Ks


@pytest.mark.parametrize("name", ["n6", "n33", "strong", "rank5", "negative_cg", "m0"])
def test_the_numpy_restatement_agrees_with_the_model(name):
    """pdm.optimise_direct (steps 1-7 in NumPy) against pgm.optimise: the same status and iterations, poses64 within pc.POSE64_TOL.  Each linear solve agrees with
    numpy.linalg.solve to rounding (tests/test_pose_graph_direct_step.py (d)); the runs still differ by up to their last step, which is below dx_tol and is kept
    or undone on a chi2 comparison that rounding decides -- the case pc.POSE64_TOL is derived for.  Measured: 2e-9 m at worst (rank5), 1e-11 where both keep it."""
    g = dict(n6=pc.graph(*pc.CASES[3], True), n33=pc.graph(*pc.CASES[4], True), strong=pc.strong_graph(), rank5=pc.rank5_graph(), negative_cg=pc.negative_graph(0.1),
             m0=pdm.m0_graph())[name]
    d = pdm.optimise_direct(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL)
    m = pgm.optimise(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL)
    dt, dr = pgm.pose_error(d["poses64"], m["poses64"])
    print(name, "status", d["status"], m["status"], "iterations", d["gn_iterations"], m["gn_iterations"], "poses64 differ by %.3e m %.3e rad" % (dt, dr))
    assert d["status"] == m["status"] and d["gn_iterations"] == m["gn_iterations"] and dt <= pc.POSE64_TOL and dr <= pc.POSE64_TOL
    if name == "negative_cg":
        assert d["status"] == pgm.NOT_POSITIVE_DEFINITE and d["pcg_iterations"] == 0
    if name == "m0":
        assert not pdm.graph_ends(g) and d["pcg_iterations"] == d["gn_iterations"]


def test_the_graphs_have_the_ends_they_are_named_for():
    assert len(pdm.graph_ends(pdm.ends288_graph())) == 96
    assert len(pdm.graph_ends(pdm.over_limit_graph())) == 138 > pdm.MAX_ENDS
    assert pdm.graph_ends(pdm.m0_graph()) == []
    assert pdm.graph_ends(pc.graph(*pc.CASES[3], True)) == [1, 2, 5]


def test_abi_of_the_direct_solve():
    import icet_amd
    from icet_amd import api
    lib = icet_amd.load_library()
    assert "icet_debug_pose_graph_direct" in api.EXPORTED_SYMBOLS and lib.icet_debug_pose_graph_direct is not None
    assert lib.icet_debug_pose_graph_direct(None, 1, None, None, None, 0, None, None, None, None, None, None, 0, None, None) == api.ICET_ERR_BAD_ARG
    assert C.sizeof(api.PoseGraphOptions) == 32 and C.sizeof(api.PoseGraphResult) == 40 and api.PoseGraphResult.solver.offset == 36
    assert C.sizeof(api.PoseGraphDirectStep) == 176 and api.PoseGraphDirectStep.ends.offset == 112 and api.PoseGraphDirectStep.ends_capacity.offset == 120
    assert api.PoseGraphDirectStep.chi2_start.offset == 152
    assert api.PG_DIRECT_MAX_ENDS == pdm.MAX_ENDS
    # the Python side's rule for the end nodes is the model's
    for g in (pdm.ends288_graph(), pdm.m0_graph(), pc.graph(*pc.CASES[3], True)):
        assert api.pose_graph_ends(g["poses"].shape[0], g["closures"], g["fixed"]) == pdm.graph_ends(g)
