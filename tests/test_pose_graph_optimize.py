"""The pose-graph optimiser on the GPU (include/icet_hip.h icet_pose_graph_optimize[_device]) against the NumPy model of
tests/pose_graph_model.py, against the truth, through its status paths and its invariants, and once end to end behind a keyframe store's closure query.  The
graphs, the tolerances and their derivation are in tests/pose_graph_cases.py; tests/test_pose_graph_optimize_host.py runs the same optimiser on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closure_model as cm      # noqa: E402
import pose_graph_cases as pc      # noqa: E402
import pose_graph_model as pgm      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import icet_amd
    c = icet_amd.Context(0)
    yield c
    c.close()


def _run(ctx, g, **kw):
    return ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL, **kw)


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in ("poses", "poses64", "edge_chi2")) and \
        all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in ("chi2_initial", "chi2_final", "status", "gn_iterations", "max_dx", "pcg_iterations"))


@pytest.mark.parametrize("noisy", [True, False], ids=["noisy", "noise_free"])
@pytest.mark.parametrize("case", range(len(pc.CASES)), ids=["n%d_c%d" % (c[0], len(c[1])) for c in pc.CASES])
def test_against_the_model_and_the_truth(ctx, case, noisy):
    """Measured on an MI355X (DESIGN.md section 20 has the table): the largest difference of poses64 to the model over the fourteen graphs was 6.9e-10 m /
    1.4e-10 rad against the bound of 4e-7; the largest relative difference of chi2 where chi2 > 1 was 1.2e-13 against 1e-8."""
    n, pairs, fx = pc.CASES[case]
    g = pc.graph(n, pairs, fx, noisy)
    r = _run(ctx, g)
    m = pc.model(("loop", n, pairs, fx, noisy), g)
    assert m["status"] == pgm.CONVERGED
    pc.compare("n = %d, %s" % (n, "noisy" if noisy else "noise-free"), r, m, g)
    if not noisy and fx is None:
        dt, dr = pgm.pose_error(r["poses"], g["truth"])
        mt, mr = pgm.pose_error(m["poses"], g["truth"])
        print("    of the truth: %.3e m %.3e rad (the model: %.3e m %.3e rad)" % (dt, dr, mt, mr))
        assert dt <= pc.CAP_T and dr <= pc.CAP_R
    # twice the same bits; the device-pointer form the same bits as the host-pointer form
    assert _same_bits(r, _run(ctx, g))
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(dev) for k in ("poses", "odo_X", "odo_info")]
    d = ctx.optimize_pose_graph_device(t[0], t[1], t[2], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL)
    p64 = d["poses64"].cpu().numpy()
    d = dict(d, poses=d["poses"].cpu().numpy(), poses64=pc.poses64_matrix(p64), edge_chi2=d["edge_chi2"].cpu().numpy())
    assert _same_bits(r, d)


def test_a_pure_chain_takes_one_band_solve_per_iteration(ctx):
    g = dict(pgm.make_loop(65, [], seed=11), fixed=None)
    r = _run(ctx, g)
    m = pc.model(("chain", 65), g)
    pc.compare("chain of 65", r, m, g)
    assert r["pcg_iterations"] == r["gn_iterations"] >= 1


def test_status_paths(ctx):
    """Results, not faults: a rank-5 closure converges as the model does; singular odometry information is status 2 and a NaN pose status 3 with the inputs
    returned; one iteration on a graph that needs three is status 1."""
    g = pc.rank5_graph()
    pc.compare("rank 5", _run(ctx, g), pc.model(("rank5",), g), g)
    g = pc.zero_row_graph()
    r, m = _run(ctx, g), pc.model(("zero_row",), g)
    assert r["status"] == m["status"] == pgm.NOT_POSITIVE_DEFINITE and r["gn_iterations"] == 1
    assert np.array_equal(r["poses"].view(np.uint32), g["poses"].view(np.uint32)) and r["chi2_final"] == r["chi2_initial"] and np.array_equal(r["edge_chi2"][0], r["edge_chi2"][1])
    g = pc.nan_graph()
    r = _run(ctx, g)
    assert r["status"] == pgm.NON_FINITE and r["gn_iterations"] == 0 and r["pcg_iterations"] == 0
    assert np.array_equal(r["poses"].view(np.uint32), g["poses"].view(np.uint32))
    g = pc.graph(33, pc.CASES[4][1], None, True)
    r, m = _run(ctx, g, gn_iters=1), pc.model(("cap",), g, gn_iters=1)
    assert r["status"] == m["status"] == pgm.ITERATION_CAP and r["gn_iterations"] == 1
    pc.compare("one iteration", r, m, g)


def test_paths_the_loop_graphs_do_not_take(ctx):
    """Against the model, with the comparison of the loop graphs: closures across the angle seam (measured and predicted yaw on opposite sides of +-pi), damping,
    a single pose, and a loose pcg_tol, which reaches the same optimum with no more band solves than the default."""
    g = pc.seam_graph()
    T = np.asarray(g["poses"], np.float64)
    assert sum(1 for c in g["closures"] if (pgm.xof(T[c[0]], T[c[1]])[5] > 0) != (c[2][5] > 0)) >= 2
    pc.compare("seam", _run(ctx, g), pc.model(("seam",), g), g)
    g = pc.graph(33, pc.CASES[4][1], None, True)
    pc.compare("damping 1e-3", _run(ctx, g, damping=1e-3), pc.model(("damped",), g, damping=1e-3), g)
    default, loose = _run(ctx, g), _run(ctx, g, pcg_tol=1e-4)
    pc.compare("pcg_tol 1e-4", loose, pc.model(("loop", 33, pc.CASES[4][1], None, True), g), g)
    print("    band solves: %d at pcg_tol 1e-4, %d at the default" % (loose["pcg_iterations"], default["pcg_iterations"]))
    assert loose["status"] == pgm.CONVERGED and loose["pcg_iterations"] <= default["pcg_iterations"]
    g = dict(pgm.make_loop(1, [], seed=11), fixed=None)
    r = _run(ctx, g)
    pc.compare("a single pose", r, pc.model(("single",), g), g)
    assert r["gn_iterations"] == 1 and r["edge_chi2"].shape == (2, 0)


def test_stalled_and_negative_definite(ctx):
    """A start thrown far from its chain ends stalled after the model's two iterations, at the model's poses.  A closure with negative definite information is
    status 2 on both sides -- through a band pivot at full strength, through p.Hp <= 0 in CG at a tenth of it (plain branches both) -- and the outputs are the
    inputs bit for bit."""
    g = pc.stalled_graph()
    r, m = _run(ctx, g), pc.model(("stalled",), g)
    pc.compare("stalled", r, m, g)
    assert r["status"] == m["status"] == pgm.STALLED and r["gn_iterations"] == m["gn_iterations"] == 2
    for key, scale in (("negative", 1.0), ("negative_cg", 0.1)):
        g = pc.negative_graph(scale)
        r, m = _run(ctx, g), pc.model((key,), g)
        print("    %s: status %d | %d after %d band solves" % (key, r["status"], m["status"], r["pcg_iterations"]))
        assert r["status"] == m["status"] == pgm.NOT_POSITIVE_DEFINITE and r["gn_iterations"] == m["gn_iterations"] == 1
        assert (r["pcg_iterations"] > 0) == (key == "negative_cg")          # a band pivot | p.Hp <= 0 in CG
        assert np.array_equal(r["poses"].view(np.uint32), g["poses"].view(np.uint32))
        assert np.array_equal(r["poses64"].view(np.uint64), pc.poses64_matrix(np.concatenate([g["poses"][:, :3, :3].reshape(-1, 9), g["poses"][:, :3, 3]], axis=1)).view(np.uint64))
        assert r["chi2_final"] == r["chi2_initial"] and abs(r["chi2_initial"] - m["chi2_initial"]) <= 1e-12 * np.abs(m["edge_chi2"][0]).sum()
        assert np.array_equal(r["edge_chi2"][0], r["edge_chi2"][1])


def test_refusals(ctx):
    import icet_amd
    from icet_amd import api
    g = pc.graph(6, pc.CASES[3][1], 4, True)
    for bad in (dict(closures=[(0, 6, np.zeros(6), np.eye(6))]), dict(closures=[(2, 2, np.zeros(6), np.eye(6))]), dict(gn_iters=0)):
        kw = dict(closures=g["closures"], gn_iters=10); kw.update(bad)
        with pytest.raises(icet_amd.IcetError) as e:
            ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], **kw)
        assert e.value.status == api.ICET_ERR_BAD_ARG


PG_METHODS = ["optimize_pose_graph", "optimize_pose_graph_device", "pose_graph_marginals", "pose_graph_marginals_device", "debug_pose_graph_marginals",
              "debug_pose_graph_step", "debug_pose_graph_direct"]


@pytest.mark.parametrize("method", PG_METHODS)
def test_every_pose_graph_method_checks_the_graph_alike(ctx, method):
    """The seven Context methods on a chain of three nodes with the closure (0, 2): odo_X one row short and a ``fixed`` of two entries are ICET_ERR_BAD_ARG from
    each, the well-formed call ends with status 0 -- the result's status, and every factor's status a hook reports."""
    import icet_amd
    from icet_amd import api
    g = pgm.make_loop(3, [(0, 2)], seed=11)
    dev = torch.device("cuda", 0)
    arg = (lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)) if method.endswith("_device") else (lambda v: v)

    def call(odo_X, fixed):
        return getattr(ctx, method)(arg(g["poses"]), arg(odo_X), arg(g["odo_info"]), g["closures"], fixed=fixed)
    for odo_X, fixed in ((g["odo_X"][:-1], None), (g["odo_X"], [0, 0])):
        with pytest.raises(icet_amd.IcetError) as e:
            call(odo_X, fixed)
        assert e.value.status == api.ICET_ERR_BAD_ARG
    r = call(g["odo_X"], None)
    statuses = {k: r[k] for k in ("status", "factor_status", "cg_status", "wm_status", "ks_status") if k in r}
    print(method, statuses)
    assert statuses and not any(statuses.values())


def test_the_optimiser_disturbs_nothing(ctx):
    """A small icet_solve on the same context before and after an optimisation: the same bits."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "scans_frame_804_805.npz"))
    a, b = d["scan1"][::4], d["scan2"][::4]
    before = ctx.solve(a, b, 5, np.zeros(6, np.float32), 24, 75)
    g = pc.graph(33, pc.CASES[4][1], None, True)
    r = _run(ctx, g)
    after = ctx.solve(a, b, 5, np.zeros(6, np.float32), 24, 75)
    assert r["status"] == pgm.CONVERGED
    for k in ("X", "pred_stds", "cov"):
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32))


# ---- end to end: store with poses -> find_closures -> closure_edges -> optimize_pose_graph -> set_pose ------------------------------------------------------
KF_SLOTS = [3, 0, 9, 5, 12, 7, 1, 14]
OFFSETS = np.array([[0, 0, 0, 0, 0, 0], [0.05, 0, 0, 0, 0, 0.005], [-0.05, 0.02, 0, 0, 0, -0.005]], np.float32)
E2E_SIGMA = (0.02, 0.002)          # the synthetic odometry: 2 cm, 2 mrad per step


def e2e_graph():
    """The drive of tests/test_loop_closure.py (scene 2000: 8 keyframes along a line, 4 revisit scans 0.3 - 0.6 m and 0.2 - 0.5 rad of yaw from keyframes 1, 3, 5
    and 7) as a chain of 12 nodes: synthetic odometry from the true poses with noise E2E_SIGMA, the start the chain of that odometry."""
    true_kf = [cm.pose_yaw((-5.0 + 1.5 * k, -1.0 + 0.1 * k, 0.0), 0.05 * k) for k in range(8)]
    near = [1, 3, 5, 7]
    off = [(0.35, 0.20, 0.30), (-0.30, 0.30, 0.45), (0.25, -0.35, -0.25), (0.40, 0.10, 0.20)]
    live = [cm.pose_yaw((true_kf[k][0, 3] + o[0], true_kf[k][1, 3] + o[1], 0.0), 0.05 * k + o[2]) for k, o in zip(near, off)]
    truth = np.array(true_kf + live, np.float64)
    rs = np.random.RandomState(23)
    sig = np.array([E2E_SIGMA[0]] * 3 + [E2E_SIGMA[1]] * 3)
    odo_X = np.array([pgm.xof(truth[k], truth[k + 1]) + sig * rs.standard_normal(6) for k in range(11)]).astype(np.float32)
    odo_info = np.array([pgm.diag_info(*E2E_SIGMA)] * 11, np.float32)
    return dict(truth=truth, poses=pgm.chain(truth[0].astype(np.float32), odo_X), odo_X=odo_X, odo_info=odo_info)


def test_end_to_end_with_a_keyframe_store():
    import icet_amd
    from icet_amd import api, lidar_sim as ls
    dev = torch.device("cuda", 0)
    g = e2e_graph()
    truth, start = g["truth"], g["poses"]
    scene = ls.make_scene(2000)
    scans = [ls.make_scan(scene, (T[:3, 3].astype(np.float64), T[:3, :3].astype(np.float64)), (100 + k) if k < 8 else (200 + k - 8), device=dev) for k, T in enumerate(truth)]
    ctx = icet_amd.Context(0)
    st = icet_amd.KeyframeStore(ctx, 16)
    try:
        st.put_device(KF_SLOTS, [(t.data_ptr(), t.shape[1], t.shape[1]) for t in scans[:8]])
        stamps = np.arange(8, dtype=np.int64) * 10
        st.set_pose(KF_SLOTS, start[:8], stamps)
        torch.cuda.synchronize()
        recs = st.find_closures([t.cpu().numpy().T for t in scans[8:]], start[8:], np.array([500, 510, 520, 530], np.int64), 7, 2.6, 4, starts=OFFSETS)
        edges = api.closure_edges(recs, [8, 9, 10, 11], {s: k for k, s in enumerate(KF_SLOTS)})
        # (every revisit finds a keyframe -- the best-scoring candidate, not necessarily the nearest)
        assert len(edges) == 4 and [e[1] for e in edges] == [8, 9, 10, 11] and all(0 <= e[0] < 8 for e in edges)
        r = ctx.optimize_pose_graph(start, g["odo_X"], g["odo_info"], edges)
        before = float(np.abs(start[:, :3, 3].astype(np.float64) - truth[:, :3, 3]).max())
        after = float(np.abs(r["poses"][:, :3, 3].astype(np.float64) - truth[:, :3, 3]).max())
        print("end to end: status %d after %d iterations, chi2 %.4g -> %.4g, largest translation error %.4f m -> %.4f m; closures' chi2 %s -> %s"
              % (r["status"], r["gn_iterations"], r["chi2_initial"], r["chi2_final"], before, after, r["edge_chi2"][0, 11:], r["edge_chi2"][1, 11:]))
        # (any status that keeps the step is a result here: the registrations' own covariances make information matrices of 1e7 .. 1e8 whose chi2 the
        # iteration lowers by four decades within the default ten iterations without the last step falling below dx_tol)
        assert r["status"] not in (pgm.NOT_POSITIVE_DEFINITE, pgm.NON_FINITE) and r["chi2_final"] < r["chi2_initial"]
        assert after < before
        assert (r["edge_chi2"][1, 11:] < r["edge_chi2"][0, 11:]).all()
        st.set_pose(KF_SLOTS, r["poses"][:8], stamps)
        for k, s in enumerate(KF_SLOTS):
            assert np.array_equal(st.debug_fetch(s, "pose"), r["poses"][k])
    finally:
        st.close(); ctx.close()
