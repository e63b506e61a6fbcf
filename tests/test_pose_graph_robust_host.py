"""CPU tests of the pose-graph optimiser's robust kernels (-m "not gpu"): pg_optimise_robust -- the driver of icet_posegraph_driver.h over the bodies of
icet_posegraph_robust.h and icet_posegraph_body.h -- run on the host by tests/cpp/test_posegraph_robust.cpp against heap blocks of the exact sizes: plain, under
the address and undefined-behaviour sanitizers, and with a workgroup of four real threads; its results against the NumPy model of
tests/pose_graph_robust_model.py.  And the ABI of the two entry points that needs no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_model as pgm      # noqa: E402
import pose_graph_robust_cases as rc      # noqa: E402
import pose_graph_robust_model as prm      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
          ("emu", ["-O2", "-DICET_PG_EMU", "-pthread"]), ("emu_san", ["-O1", "-g", "-DICET_PG_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def _items():
    """[(key, graph, options, kind, flags, scale, direct)]: key[0] says what the run is checked as."""
    items = []
    gs = rc.graphs()
    for (name, kind, K) in rc.fixed_runs():
        g, fl = gs[name]
        items.append((("fixed", name, kind, K, "direct"), g, dict(gn_iters=K, dx_tol=0.0), kind, fl, rc.SCALE, True))
        items.append((("fixed", name, kind, K, "cg"), g, dict(gn_iters=K, dx_tol=0.0, max_pcg=100), kind, fl, rc.SCALE, False))
    for (n, good, bad) in rc.TABLE:
        g = rc.planted(n, good, bad)
        for kind in (prm.CAUCHY, prm.GEMAN_MCCLURE):
            items.append((("converged", "n%d" % n, kind), g, dict(gn_iters=30), kind, 0, rc.SCALE, True))
        items.append((("converged_odo", "n%d" % n, prm.CAUCHY), g, dict(gn_iters=30), prm.CAUCHY, prm.ROBUST_ODOMETRY, rc.SCALE, True))
    for kind in (prm.HUBER, prm.CAUCHY, prm.GEMAN_MCCLURE):
        for direct in (True, False):
            items.append((("nan", kind, direct), pc.nan_graph(), {}, kind, 0, rc.SCALE, direct))
            items.append((("zero_row", kind, direct), pc.zero_row_graph(), {}, kind, prm.ROBUST_ODOMETRY, rc.SCALE, direct))
    # kind 0 on the plain optimiser's own graphs, both solvers (the program compares each with pg_optimise / pg_optimise_direct byte for byte)
    for (n, pairs, fx) in pc.CASES:
        for direct in (True, False):
            items.append((("kind0", n, direct), pc.graph(n, pairs, fx, True), {}, prm.NONE, 0, 0.0, direct))
    return items


@pytest.fixture(scope="module")
def host_runs(tmp_path_factory):
    """The four builds run once on every item: (items, results of the plain build)."""
    tmp = tmp_path_factory.mktemp("pg_robust")
    src = os.path.join(ROOT, "tests", "cpp", "test_posegraph_robust.cpp")
    items = _items()
    fin = str(tmp / "runs.bin")
    rc.write_runs(fin, [it[1:] for it in items])
    outs = {}
    for name, flags in BUILDS:
        exe = str(tmp / ("test_posegraph_robust_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", ROOT, src, "-o", exe])
        fout = str(tmp / (name + ".bin"))
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        outs[name] = open(fout, "rb").read()
        if name == "plain":
            n_kind0 = sum(1 for it in items if it[3] == prm.NONE)
            assert ("kind 0 as the plain driver: %d runs" % n_kind0) in r.stdout and n_kind0 >= 2 * len(pc.CASES)
    # the one-thread and the four-thread workgroup, sanitised or not, write the same bytes (the reductions have one order for any thread count)
    assert outs["plain"] == outs["san"] == outs["emu"] == outs["emu_san"]
    return items, rc.read_runs(str(tmp / "plain.bin"), [it[1:] for it in items])


def test_the_existing_host_programs_still_compile():
    """posegraph_host.h's backend has no rgrid / rgroup: the three programs beside it build untouched (the driver calls those only from the robust templates)."""
    for prog in ("test_posegraph_optimize.cpp", "test_posegraph_direct.cpp", "test_posegraph_marginals.cpp"):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsyntax-only", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", prog)])


def test_fixed_iteration_runs_against_the_model(host_runs):
    """dx_tol = 0, gn_iters = 1, 3 (6 for Cauchy and Geman-McClure), the direct solve and conjugate gradients with max_pcg = 100: status ITERATION_CAP with the
    model's iteration count; poses64, edge_weight, cost_final and the raw chi2_final within rc.bounds() = 16 x the measured host-against-model distance."""
    items, res = host_runs
    b = rc.bounds()
    worst = dict(t=0.0, r=0.0, w=0.0, cost=0.0)
    count = 0
    for it, r in zip(items, res):
        key = it[0]
        if key[0] != "fixed":
            continue
        m = rc.model(key[1], key[2], gn_iters=key[3], dx_tol=0.0)
        rc.check_fixed_run(str(key[1:]), r, m, it[1], b, worst)
        assert r["solver"] == (1 if key[4] == "direct" else 0)
        assert r["downweighted"] == int((r["edge_weight"] < 0.5).sum())
        count += 1
    print("the host build's largest distance from the model over %d runs: %s | recorded %s" % (count, worst, rc.MEASURED_HOST))
    assert count == 2 * len(rc.fixed_runs())


def test_converged_runs_and_their_outcome(host_runs):
    """Cauchy and Geman-McClure at the default options on the table's graphs: CONVERGED, iterations within one of the model's, poses within 10 dx_tol of the
    model's (the model's last steps contract: tests/test_pose_graph_robust_model.py), and the outcome conditions on this output."""
    items, res = host_runs
    count = 0
    for it, r in zip(items, res):
        key, g = it[0], it[1]
        if key[0] not in ("converged", "converged_odo"):
            continue
        n = g["poses"].shape[0]
        m = rc.model(key[1], key[2], gn_iters=30, flags=it[4] if key[0] == "converged_odo" else None)
        dt, dr = pgm.pose_error(r["poses64"], m["poses64"])
        print(key, "iterations %d | %d, %.3e m %.3e rad from the model" % (r["gn_iterations"], m["gn_iterations"], dt, dr))
        assert r["status"] == m["status"] == pgm.CONVERGED and abs(r["gn_iterations"] - m["gn_iterations"]) <= 1
        assert dt <= 10 * pc.DX_TOL and dr <= 10 * pc.DX_TOL
        if key[0] == "converged_odo":
            # Cauchy on the odometry edges too: the library's own weights, not only the model's
            rc.check_odometry_weights(str(key), r, g)
            count += 1
            continue
        c = rc.clean(n, rc.TABLE[[t[0] for t in rc.TABLE].index(n)][1])
        mc = pc.model(("robust_clean", n), c)
        rc.check_outcome(str(key), r, g, mc["poses64"])
        count += 1
    assert count == 3 * len(rc.TABLE)


def test_failures_return_the_inputs(host_runs):
    """The NaN graph: status 3; the singular-odometry graph: status 2.  Both return the input bits, the weights w(chi0), and cost_final == cost_initial."""
    items, res = host_runs
    count = 0
    for it, r in zip(items, res):
        key, g, kind, flags = it[0], it[1], it[3], it[4]
        if key[0] not in ("nan", "zero_row"):
            continue
        n = g["poses"].shape[0]
        print(key, "status", r["status"], "iterations", r["gn_iterations"])
        assert r["status"] == (pgm.NON_FINITE if key[0] == "nan" else pgm.NOT_POSITIVE_DEFINITE)
        assert r["gn_iterations"] == (0 if key[0] == "nan" else 1)
        assert np.array_equal(r["poses"].view(np.uint32), np.asarray(g["poses"], np.float32).view(np.uint32))
        assert np.array_equal(r["poses64"][:, :3, :], np.asarray(g["poses"], np.float32).astype(np.float64)[:, :3, :], equal_nan=True)
        assert np.array_equal(r["edge_chi2"][0], r["edge_chi2"][1], equal_nan=True)
        kinds = prm.edge_kinds(n, r["edge_weight"].shape[0], kind, flags)
        w0 = np.array([prm.weight(k, rc.SCALE, s) for k, s in zip(kinds, r["edge_chi2"][0])])
        assert np.allclose(r["edge_weight"], w0, rtol=1e-15, atol=0.0)
        assert np.array_equal(np.float64(r["cost_final"]).view(np.uint64), np.float64(r["cost_initial"]).view(np.uint64))
        assert np.array_equal(np.float64(r["chi2_final"]).view(np.uint64), np.float64(r["chi2_initial"]).view(np.uint64))
        assert np.isnan(r["cost_final"]) == (key[0] == "nan")
        count += 1
    assert count == 12


def test_abi_of_the_robust_entries():
    """The symbols are exported, the structs have the header's sizes, and each bad argument is refused (a NULL context: ICET_ERR_BAD_ARG before anything else;
    the context-free checks of kind, flags and scale run in tests/cpp/test_posegraph_robust.cpp, through pg_robust_args)."""
    import icet_amd
    from icet_amd import api
    lib = icet_amd.load_library()
    assert C.sizeof(api.PoseGraphRobust) == 16 and C.sizeof(api.PoseGraphRobustResult) == 64
    assert api.PoseGraphRobustResult.cost_initial.offset == 40 and api.PoseGraphRobustResult.downweighted.offset == 56
    assert C.sizeof(api.PoseGraphOptions) == 32 and C.sizeof(api.PoseGraphResult) == 40
    assert api.PG_ROBUST_DEFAULT_SCALE == prm.DEFAULT_SCALE == 16.8119 and api.PG_ROBUST_ODOMETRY == 1
    assert api.PG_ROBUST_KINDS == dict(huber=1, cauchy=2, geman_mcclure=3)
    res = api.PoseGraphRobustResult()
    for name in ("icet_pose_graph_optimize_robust", "icet_pose_graph_optimize_robust_device"):
        assert name in api.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        for rob in (None, api.PoseGraphRobust(1, 0, 16.8119), api.PoseGraphRobust(4, 0, 1.0), api.PoseGraphRobust(-1, 0, 1.0), api.PoseGraphRobust(1, 2, 1.0),
                    api.PoseGraphRobust(2, 0, 0.0), api.PoseGraphRobust(3, 0, float("nan")), api.PoseGraphRobust(1, 0, float("inf"))):
            st = getattr(lib, name)(None, 1, None, None, None, 0, None, None, None, None, None, None, None if rob is None else C.byref(rob), None, None, None, None, C.byref(res))
            assert st == api.ICET_ERR_BAD_ARG
    # the Python side refuses a kernel's name or a scale it does not know before any call
    ctx = api.Context.__new__(api.Context)
    for kw in (dict(robust="tukey"), dict(robust="cauchy", robust_scale=0.0), dict(robust="huber", robust_scale=float("nan")), dict(robust="cauchy", robust_scale=-1.0)):
        with pytest.raises(api.IcetError) as e:
            ctx._pose_graph_robust(**kw)
        assert e.value.status == api.ICET_ERR_BAD_ARG


def test_closure_helpers():
    """api.reweighted_closures scales every closure's information by its weight; api.inlier_closures keeps those at or above min_weight."""
    from icet_amd import api
    g = rc.planted(*rc.TABLE[0])
    n = g["poses"].shape[0]
    w = np.concatenate([np.ones(n - 1), [0.9, 0.7, 1e-5]])
    rw = api.reweighted_closures(g["closures"], w[n - 1:])
    assert len(rw) == 3
    for (i, j, X, info), (i2, j2, X2, info2), wi in zip(g["closures"], rw, w[n - 1:]):
        assert (i, j) == (i2, j2) and np.array_equal(X, X2) and info2.dtype == np.float32
        assert np.array_equal(info2, (np.asarray(info, np.float64) * wi).astype(np.float32))
    # the E weights of a result are taken too: the closures' are its last C
    rw2 = api.reweighted_closures(g["closures"], w, n=n)
    assert all(np.array_equal(a[3], b[3]) for a, b in zip(rw, rw2))
    inl = api.inlier_closures(g["closures"], w, n=n)
    assert [(c[0], c[1]) for c in inl] == [(0, 11), (1, 10)]
    assert len(api.inlier_closures(g["closures"], w[n - 1:], min_weight=0.8)) == 1
    # a length that is neither the closures' nor (with n) the edges' is another graph's
    for bad, kw in ((w[:2], {}), (w, {}), (w[1:], dict(n=n)), (w[n - 2:], {}), (w[n - 1:], dict(n=n + 1))):
        with pytest.raises(api.IcetError):
            api.reweighted_closures(g["closures"], bad, **kw)
