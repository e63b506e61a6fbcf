"""GPU tests of the pose-graph optimiser's DIRECT solve (DESIGN.md section 20 "The direct solve"; option "pg_solver", Context.optimize_pose_graph(solver=)): whole
runs against the NumPy model on the graphs of the conjugate-gradient tests, the option's scope, the end-to-end case at default options, the smallest shapes that
can still go wrong, and the limit of 128 end nodes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_direct_model as pdm      # noqa: E402
import pose_graph_model as pgm      # noqa: E402
import test_pose_graph_optimize as tpo      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ITEMS = pdm.whole_run_items()


def _item_id(key):
    return "n%d_c%d_%s" % (key[1], len(key[2]), "noisy" if key[4] else "exact") if key[0] == "loop" else "_".join(str(v) for v in key)


@pytest.fixture(scope="module")
def ctx():
    import icet_amd
    c = icet_amd.Context(0)
    yield c
    c.close()


def _run(ctx, g, solver="direct", **kw):
    return ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL, solver=solver, **kw)


def _same_bits(a, b):
    return tpo._same_bits(a, b) and a["solver"] == b["solver"]


def _run_device(ctx, g, solver="direct", **kw):
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(dev) for k in ("poses", "odo_X", "odo_info")]
    d = ctx.optimize_pose_graph_device(t[0], t[1], t[2], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL, solver=solver, **kw)
    return dict(d, poses=d["poses"].cpu().numpy(), poses64=pc.poses64_matrix(d["poses64"].cpu().numpy()), edge_chi2=d["edge_chi2"].cpu().numpy())


@pytest.mark.parametrize("item", range(len(ITEMS)), ids=[_item_id(k) for k, _, _ in ITEMS])
def test_whole_runs_against_the_model(ctx, item):
    """solver="direct" on the list of the host test: pc.compare with pc's tolerances, status and iterations the model's (strong: 3 at default options;
    negative(0.1): status 2 through a pivot of Ks, the inputs returned), twice the same bits, the device-pointer form the same bits."""
    key, g, o = ITEMS[item]
    r = _run(ctx, g, **o)
    assert r["solver"] == 1
    pdm.check_whole_run(key, g, o, r)
    assert _same_bits(r, _run(ctx, g, **o))
    assert _same_bits(r, _run_device(ctx, g, **o))


def test_the_option_does_not_leak(ctx):
    """A conjugate-gradient run and an icet_solve before and after a direct run on the same context: the same bits.  solver=None reads the context's option."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "scans_frame_804_805.npz"))
    a, b = d["scan1"][::4], d["scan2"][::4]
    g = pc.graph(33, pc.CASES[4][1], None, True)
    s0 = ctx.solve(a, b, 5, np.zeros(6, np.float32), 24, 75)
    cg0 = _run(ctx, g, solver=None)
    direct = _run(ctx, g, solver="direct")
    cg1 = _run(ctx, g, solver=None)
    s1 = ctx.solve(a, b, 5, np.zeros(6, np.float32), 24, 75)
    assert cg0["solver"] == 0 and direct["solver"] == 1 and direct["status"] == pgm.CONVERGED
    assert _same_bits(cg0, cg1) and _same_bits(cg0, _run(ctx, g, solver="cg"))
    for k in ("X", "pred_stds", "cov"):
        assert np.array_equal(s0[k].view(np.uint32), s1[k].view(np.uint32))
    ctx.set_option("pg_solver", 1)
    try:
        assert _same_bits(direct, _run(ctx, g, solver=None))
        assert _same_bits(cg0, _run(ctx, g, solver="cg")) and _same_bits(direct, _run(ctx, g, solver=None))
    finally:
        ctx.set_option("pg_solver", 0)
    assert _same_bits(cg0, _run(ctx, g, solver=None))


def test_end_to_end_at_default_options():
    """tests/test_pose_graph_optimize.py's end-to-end case (its graph, slots and starts imported; the store calls are that test's): closures from find_closures
    carry the registrations' own information, 1e7 .. 1e8 against the odometry's 2.5e3, and conjugate gradients spend their cap (status 1 after 10 iterations).
    solver="auto" at default options converges as the model does."""
    import icet_amd
    from icet_amd import api, lidar_sim as ls
    dev = torch.device("cuda", 0)
    g = tpo.e2e_graph()
    truth, start = g["truth"], g["poses"]
    scene = ls.make_scene(2000)
    scans = [ls.make_scan(scene, (T[:3, 3].astype(np.float64), T[:3, :3].astype(np.float64)), (100 + k) if k < 8 else (200 + k - 8), device=dev) for k, T in enumerate(truth)]
    ctx = icet_amd.Context(0)
    st = icet_amd.KeyframeStore(ctx, 16)
    try:
        st.put_device(tpo.KF_SLOTS, [(t.data_ptr(), t.shape[1], t.shape[1]) for t in scans[:8]])
        st.set_pose(tpo.KF_SLOTS, start[:8], np.arange(8, dtype=np.int64) * 10)
        torch.cuda.synchronize()
        recs = st.find_closures([t.cpu().numpy().T for t in scans[8:]], start[8:], np.array([500, 510, 520, 530], np.int64), 7, 2.6, 4, starts=tpo.OFFSETS)
        edges = api.closure_edges(recs, [8, 9, 10, 11], {s: k for k, s in enumerate(tpo.KF_SLOTS)})
        assert len(edges) == 4
        r = ctx.optimize_pose_graph(start, g["odo_X"], g["odo_info"], edges, solver="auto")
        m = pgm.optimise(start, g["odo_X"], g["odo_info"], edges)
        print("end to end, auto: status %d | %d after %d | %d iterations, %d band solves, chi2 %.6g -> %.12g | %.12g" % (r["status"], m["status"], r["gn_iterations"],
              m["gn_iterations"], r["pcg_iterations"], r["chi2_initial"], r["chi2_final"], m["chi2_final"]))
        assert r["solver"] == 1 and r["status"] == pgm.CONVERGED == m["status"] and r["gn_iterations"] == m["gn_iterations"]
        assert abs(r["chi2_final"] - m["chi2_final"]) <= pc.CHI2_RTOL * m["chi2_final"]
        pc.compare("end to end", r, m, dict(g, closures=edges, fixed=None))
    finally:
        st.close(); ctx.close()


SMALL = {"n1": lambda: dict(pgm.make_loop(1, [], seed=11), fixed=None),
         "n2_m0": lambda: pc.graph(2, ((0, 1),), None, True),
         "n3_far_end_fixed": lambda: pc.graph(3, ((0, 2),), None, True),
         "n6_duplicates_reversed_fixed_middle": lambda: pc.graph(*pc.CASES[3], True),
         "n33_nodes_1_and_32": lambda: pc.graph(33, ((1, 32),), None, True),
         "n65_nodes_1_and_64": lambda: pc.graph(65, ((1, 64),), None, True),
         "ends288": pdm.ends288_graph}


@pytest.mark.parametrize("name", list(SMALL))
def test_the_smallest_shapes_that_can_go_wrong(ctx, name):
    """n = 1; closures that leave no end node; shared, duplicate and reversed ends around a fixed node; a closure from node 1 to the last node where the chunk of
    32 matters; 96 end nodes (q = 576: more than two rounds of 256 threads)."""
    g = SMALL[name]()
    r = _run(ctx, g)
    m = pgm.optimise(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL)
    pc.compare(name, r, m, g)
    n_ends = len(pdm.graph_ends(g))
    assert n_ends == dict(n1=0, n2_m0=0, n3_far_end_fixed=0, n6_duplicates_reversed_fixed_middle=3, n33_nodes_1_and_32=2, n65_nodes_1_and_64=2, ends288=96)[name]
    assert r["solver"] == 1 and r["status"] == m["status"] == pgm.CONVERGED and r["gn_iterations"] == m["gn_iterations"]
    assert r["pcg_iterations"] == ((1 + pdm.REFINE) if n_ends else 1) * r["gn_iterations"]
    assert _same_bits(r, _run(ctx, g))


def test_limits(ctx):
    """138 end nodes: "direct" refuses with ICET_ERR_UNSUPPORTED and leaves the outputs untouched, "auto" gives the bits of "cg"; pg_solver = 3 is a bad argument."""
    import ctypes as C
    import icet_amd
    from icet_amd import api
    g = pdm.over_limit_graph()
    assert len(pdm.graph_ends(g)) == 138
    with pytest.raises(icet_amd.IcetError) as e:
        _run(ctx, g, solver="direct")
    assert e.value.status == api.ICET_ERR_UNSUPPORTED and "138" in str(e.value) and "128" in str(e.value)
    # the outputs untouched: the raw call with sentinel buffers
    pg = ctx._pose_graph_host(g["poses"], g["odo_X"], g["odo_info"], g["closures"], None); n = pg.n
    opt = api.PoseGraphOptions(10, 0, pc.DX_TOL, 0.0, 0.0)
    out = np.full((n, 16), 7.0, np.float32); p64 = np.full((n, 12), 7.0); chi = np.full((2, n - 1 + pg.nc), 7.0); res = api.PoseGraphResult()
    res.status = -5
    ctx.set_option("pg_solver", 1)
    try:
        s = icet_amd.load_library().icet_pose_graph_optimize(*pg.args, C.byref(opt), out.ctypes.data, p64.ctypes.data, chi.ctypes.data, C.byref(res))
    finally:
        ctx.set_option("pg_solver", 0)
    assert s == api.ICET_ERR_UNSUPPORTED and (out == 7.0).all() and (p64 == 7.0).all() and (chi == 7.0).all() and res.status == -5
    auto, cg = _run(ctx, g, solver="auto"), _run(ctx, g, solver="cg")
    assert auto["solver"] == 0 and _same_bits(auto, cg) and cg["status"] == pgm.CONVERGED
    with pytest.raises(icet_amd.IcetError) as e:
        ctx.set_option("pg_solver", 3)
    assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError) as e:
        _run(ctx, g, solver="woodbury")
    assert e.value.status == api.ICET_ERR_BAD_ARG
    # the option is where it was
    small = pc.graph(33, pc.CASES[4][1], None, True)
    assert _run(ctx, small, solver=None)["solver"] == 0
