"""The pose-graph optimiser's robust kernels on the GPU (include/icet_hip.h icet_pose_graph_optimize_robust[_device]; DESIGN.md section 20 "Robust kernels")
against the NumPy model of tests/pose_graph_robust_model.py: kind 0 against the plain entry bit for bit, fixed-iteration runs against the model, converged runs and
what they do to planted false closures, the invariants, and the marginals at the robust optimum.  The graphs and the bounds are in
tests/pose_graph_robust_cases.py; tests/test_pose_graph_robust_host.py runs the same optimiser on the CPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_model as pgm      # noqa: E402
import pose_graph_robust_cases as rc      # noqa: E402
import pose_graph_robust_model as prm      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
KIND_NAMES = {prm.HUBER: "huber", prm.CAUCHY: "cauchy", prm.GEMAN_MCCLURE: "geman_mcclure"}


@pytest.fixture(scope="module")
def ctx():
    import icet_amd
    c = icet_amd.Context(0)
    yield c
    c.close()


def _run(ctx, g, kind, flags=0, **kw):
    kw.setdefault("dx_tol", pc.DX_TOL)
    if kind == prm.NONE:
        return ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], **kw)
    return ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], robust=KIND_NAMES[kind], robust_scale=rc.SCALE,
                                   robust_odometry=bool(flags & prm.ROBUST_ODOMETRY), **kw)


def _raw_robust(ctx, g, kind, flags, scale, solver, gn_iters=10, dx_tol=pc.DX_TOL, max_pcg=0):
    """icet_pose_graph_optimize_robust itself (the Python call takes the plain entry without a kernel): the result dict of a robust call."""
    import icet_amd
    from icet_amd import api
    m = ctx._pose_graph_host(g["poses"], g["odo_X"], g["odo_info"], list(g["closures"]), g["fixed"]); n = m.n
    opt = api.PoseGraphOptions(gn_iters, max_pcg, dx_tol, 0.0, 0.0)
    rob = api.PoseGraphRobust(kind, flags, scale)
    out = np.zeros((n, 16), np.float32); p64 = np.zeros((n, 12), np.float64); chi = np.zeros((2, n - 1 + m.nc), np.float64); wt = np.zeros(n - 1 + m.nc, np.float64)
    res = api.PoseGraphRobustResult()
    with ctx._pose_graph_solver(solver):
        ctx._check(icet_amd.load_library().icet_pose_graph_optimize_robust(*m.args, C.byref(opt), C.byref(rob), out.ctypes.data, p64.ctypes.data, chi.ctypes.data,
                                                                            wt.ctypes.data, C.byref(res)))
    return dict(ctx._pose_graph_robust_result(res), poses=out.reshape(n, 4, 4), poses64=pc.poses64_matrix(p64), edge_chi2=chi, edge_weight=wt)


def _bits(v):
    return np.ascontiguousarray(np.asarray(v)).view(np.uint8)


SCALARS = ("chi2_initial", "chi2_final", "status", "gn_iterations", "max_dx", "pcg_iterations", "solver")


def _same_bits(a, b, keys=("poses", "poses64", "edge_chi2"), scalars=SCALARS):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys) and all(np.array_equal(_bits(np.float64(a[k])), _bits(np.float64(b[k]))) for k in scalars)


@pytest.mark.parametrize("solver", ["cg", "direct"])
@pytest.mark.parametrize("name", ["n12", "n33", "n257"])
def test_kind_zero_is_the_plain_entry_bit_for_bit(ctx, name, solver):
    g, _ = rc.graphs()[name]
    plain = ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL, solver=solver)
    # (a kind of 0 takes any scale and either flag)
    for flags, scale in ((0, 0.0), (prm.ROBUST_ODOMETRY, rc.SCALE)):
        r = _raw_robust(ctx, g, prm.NONE, flags, scale, solver)
        assert _same_bits(r, plain)
        assert (r["edge_weight"] == 1.0).all() and r["downweighted"] == 0
        assert np.array_equal(_bits(np.float64(r["cost_initial"])), _bits(np.float64(plain["chi2_initial"])))
        assert np.array_equal(_bits(np.float64(r["cost_final"])), _bits(np.float64(plain["chi2_final"])))
    assert set(plain) == {"chi2_initial", "chi2_final", "status", "gn_iterations", "max_dx", "pcg_iterations", "solver", "poses", "poses64", "edge_chi2"}


WORST = dict(t=0.0, r=0.0, w=0.0, cost=0.0)


@pytest.mark.parametrize("name", list(rc.graphs()))
def test_fixed_iteration_runs_against_the_model(ctx, name):
    """The runs of tests/test_pose_graph_robust_host.py on the device, under the same bounds (16 x the host build's measured distance from the model).  Measured
    on an MI355X: DESIGN.md section 20 has the device's largest distances beside the host's."""
    g, fl = rc.graphs()[name]
    b = rc.bounds()
    for (nm, kind, K) in rc.fixed_runs():
        if nm != name:
            continue
        m = rc.model(name, kind, gn_iters=K, dx_tol=0.0)
        for solver, extra in (("direct", {}), ("cg", dict(max_pcg=100))):
            if kind == prm.NONE:
                r = _raw_robust(ctx, g, prm.NONE, 0, 0.0, solver, gn_iters=K, dx_tol=0.0, **extra)          # (kind 0 through the robust entry)
            else:
                r = _run(ctx, g, kind, fl, gn_iters=K, dx_tol=0.0, solver=solver, **extra)
            rc.check_fixed_run("%s kind %d K %d %s" % (name, kind, K, solver), r, m, g, b, WORST)
            assert r["solver"] == (1 if solver == "direct" else 0)
    print("the device's largest distance from the model so far:", WORST)


@pytest.mark.parametrize("kind", [prm.CAUCHY, prm.GEMAN_MCCLURE], ids=["cauchy", "geman_mcclure"])
@pytest.mark.parametrize("case", rc.TABLE, ids=lambda c: "n%d" % c[0])
def test_converged_runs_switch_the_false_closures_off(ctx, case, kind):
    from icet_amd import api
    n, good, bad = case
    g = rc.planted(n, good, bad)
    plain = _run(ctx, g, prm.NONE, solver="direct")
    pt, pr = pgm.pose_error(plain["poses64"], g["truth"])
    print("plain: status %d, %.3f m %.3f rad from the truth" % (plain["status"], pt, pr))
    assert plain["status"] == pgm.CONVERGED and pt > rc.PLAIN_OFF_M
    r = _run(ctx, g, kind, gn_iters=30, solver="direct")
    m = rc.model("n%d" % n, kind, gn_iters=30)
    dt, dr = pgm.pose_error(r["poses64"], m["poses64"])
    tt, tr = pgm.pose_error(r["poses64"], g["truth"])
    print("iterations %d | %d, %.3e m %.3e rad from the model, %.4f m %.2e rad from the truth" % (r["gn_iterations"], m["gn_iterations"], dt, dr, tt, tr))
    assert r["status"] == m["status"] == pgm.CONVERGED and abs(r["gn_iterations"] - m["gn_iterations"]) <= 1
    assert dt <= 10 * pc.DX_TOL and dr <= 10 * pc.DX_TOL
    clean = pc.model(("robust_clean", n), rc.clean(n, good))
    rc.check_outcome("n%d kind %d" % (n, kind), r, g, clean["poses64"])
    inl = api.inlier_closures(g["closures"], r["edge_weight"], n=n)
    assert [(c[0], c[1]) for c in inl] == [tuple(p) for p in good]
    assert r["cost_final"] < r["cost_initial"] and r["cost_final"] < r["chi2_final"]
    # float32 poses: every pose rounded once, the fixed node's input bits
    assert np.array_equal(r["poses"][0].view(np.uint32), np.asarray(g["poses"], np.float32)[0].view(np.uint32))
    assert pgm.pose_error(r["poses"], r["poses64"])[0] <= pc.float32_tol(r["poses"])


@pytest.mark.parametrize("case", rc.TABLE, ids=lambda c: "n%d" % c[0])
def test_huber_bounds_the_damage(ctx, case):
    """Huber is convex and only bounds a false closure's pull: at least HUBER_GAIN x closer to the truth than the plain run, false weights well below 0.5."""
    n, good, bad = case
    g = rc.planted(n, good, bad)
    plain = _run(ctx, g, prm.NONE, solver="direct")
    r = _run(ctx, g, prm.HUBER, gn_iters=30, solver="direct")
    pt, _ = pgm.pose_error(plain["poses64"], g["truth"])
    ht, hr = pgm.pose_error(r["poses64"], g["truth"])
    w = r["edge_weight"][n - 1:]
    print("n%d Huber: status %d after %d iterations, %.3f m %.2e rad from the truth (plain %.3f m: %.1f x), false weights <= %.2e, downweighted %d"
          % (n, r["status"], r["gn_iterations"], ht, hr, pt, pt / ht, w[len(good):].max(), r["downweighted"]))
    assert r["status"] == pgm.CONVERGED and rc.HUBER_GAIN * ht <= pt
    assert (w[:len(good)] > rc.GOOD_WEIGHT_MIN).all() and (w[len(good):] < 0.05).all() and r["downweighted"] == len(bad)
    assert (r["edge_weight"][:n - 1] == 1.0).all()          # the odometry edges are left alone without the flag


@pytest.mark.parametrize("case", rc.TABLE[:2], ids=lambda c: "n%d" % c[0])
def test_cauchy_on_the_odometry_keeps_the_odometry(ctx, case):
    """A converged Cauchy run with ICET_PG_ROBUST_ODOMETRY: the model's run, every odometry weight above 0.5, the false closures switched off."""
    n, good, bad = case
    g = rc.planted(n, good, bad)
    r = _run(ctx, g, prm.CAUCHY, prm.ROBUST_ODOMETRY, gn_iters=30, solver="direct")
    m = rc.model("n%d" % n, prm.CAUCHY, gn_iters=30, flags=prm.ROBUST_ODOMETRY)
    dt, dr = pgm.pose_error(r["poses64"], m["poses64"])
    print("iterations %d | %d, %.3e m %.3e rad from the model" % (r["gn_iterations"], m["gn_iterations"], dt, dr))
    assert r["status"] == m["status"] == pgm.CONVERGED and abs(r["gn_iterations"] - m["gn_iterations"]) <= 1
    assert dt <= 10 * pc.DX_TOL and dr <= 10 * pc.DX_TOL
    rc.check_odometry_weights("n%d Cauchy, odometry too" % n, r, g)


def test_same_bits_run_to_run_and_form_to_form(ctx):
    """Two calls, the host-pointer and the device-pointer form, and an icet_solve on the same context before and after: the same bits."""
    g = rc.planted(*rc.TABLE[1])
    keys = ("poses", "poses64", "edge_chi2", "edge_weight")
    scalars = SCALARS + ("cost_initial", "cost_final", "downweighted")
    s = np.load(os.path.join(ROOT, "tests", "golden", "scans_frame_804_805.npz"))
    x0 = np.zeros(6, np.float32)
    before = ctx.solve(s["scan1"], s["scan2"], 3, x0, 24, 75)
    for solver in ("direct", "cg"):
        a = _run(ctx, g, prm.CAUCHY, prm.ROBUST_ODOMETRY, solver=solver, max_pcg=100)
        b = _run(ctx, g, prm.CAUCHY, prm.ROBUST_ODOMETRY, solver=solver, max_pcg=100)
        assert _same_bits(a, b, keys, scalars)
        dev = torch.device("cuda", 0)
        t = [torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(dev) for k in ("poses", "odo_X", "odo_info")]
        d = ctx.optimize_pose_graph_device(t[0], t[1], t[2], g["closures"], fixed=g["fixed"], dx_tol=pc.DX_TOL, solver=solver, max_pcg=100, robust="cauchy",
                                           robust_scale=rc.SCALE, robust_odometry=True)
        d = dict(d, poses=d["poses"].cpu().numpy(), poses64=pc.poses64_matrix(d["poses64"].cpu().numpy()), edge_chi2=d["edge_chi2"].cpu().numpy(),
                 edge_weight=d["edge_weight"].cpu().numpy())
        assert _same_bits(a, d, keys, scalars)
    after = ctx.solve(s["scan1"], s["scan2"], 3, x0, 24, 75)
    assert np.array_equal(before["X"].view(np.uint32), after["X"].view(np.uint32))


def test_failures_return_the_inputs(ctx):
    for g, status, its, flags in ((pc.nan_graph(), pgm.NON_FINITE, 0, 0), (pc.zero_row_graph(), pgm.NOT_POSITIVE_DEFINITE, 1, prm.ROBUST_ODOMETRY)):
        for solver in ("direct", "cg"):
            r = _run(ctx, g, prm.CAUCHY, flags, solver=solver)
            n = g["poses"].shape[0]
            assert r["status"] == status and r["gn_iterations"] == its
            assert np.array_equal(r["poses"].view(np.uint32), np.asarray(g["poses"], np.float32).view(np.uint32))
            assert np.array_equal(r["edge_chi2"][0], r["edge_chi2"][1], equal_nan=True)
            kinds = prm.edge_kinds(n, r["edge_weight"].shape[0], prm.CAUCHY, flags)
            w0 = np.array([prm.weight(k, rc.SCALE, s) for k, s in zip(kinds, r["edge_chi2"][0])])
            assert np.allclose(r["edge_weight"], w0, rtol=1e-14, atol=0.0)
            assert np.array_equal(_bits(np.float64(r["cost_final"])), _bits(np.float64(r["cost_initial"])))
            assert np.array_equal(_bits(np.float64(r["chi2_final"])), _bits(np.float64(r["chi2_initial"])))


def test_bad_arguments_are_refused(ctx):
    from icet_amd import api
    g = rc.planted(*rc.TABLE[0])
    for (kind, flags, scale) in ((4, 0, 1.0), (-1, 0, 1.0), (1, 2, 1.0), (0, 4, 1.0), (2, 0, 0.0), (3, 0, float("nan")), (1, 0, float("inf")), (2, 0, -3.0)):
        with pytest.raises(api.IcetError) as e:
            _raw_robust(ctx, g, kind, flags, scale, "direct")
        assert e.value.status == api.ICET_ERR_BAD_ARG and "icet_pose_graph_optimize_robust" in str(e.value)


# The largest ratio of a diagonal entry of the marginals with the closures reweighted to the clean graph's, from the MODEL's H^-1 at the model's Cauchy optimum
# (dense, on the CPU): 1.0442 at n = 12, 1.0639 at n = 33.  It is not the false closures' 1.9e-5 of weight (that moves no entry by more than 2e-4) but the GOOD
# closures' own Cauchy weights of 0.89 .. 0.97, which the clean graph counts in full.  So the factor of 1.05 that the false closures alone would allow holds at n = 12 and is widened at n = 33 to
# the model's own number with 0.5 % on top; and every entry's ratio must be the model's ratio to 1e-6.
MARGINALS_FACTOR = {12: 1.05, 33: 1.0639 * 1.005}


@pytest.mark.parametrize("case", rc.TABLE[:2], ids=lambda c: "n%d" % c[0])
def test_marginals_at_the_robust_optimum(ctx, case):
    from icet_amd import api
    n, good, bad = case
    g, c = rc.planted(n, good, bad), rc.clean(n, good)
    r = _run(ctx, g, prm.CAUCHY, gn_iters=30, solver="direct")
    rw = api.reweighted_closures(g["closures"], r["edge_weight"], n=n)
    a = ctx.pose_graph_marginals(r["poses"], g["odo_X"], g["odo_info"], rw)
    b = ctx.pose_graph_marginals(r["poses"], c["odo_X"], c["odo_info"], c["closures"])
    assert a["status"] == 0 and b["status"] == 0
    da, db = np.einsum("kaa->ka", a["cov"])[1:], np.einsum("kaa->ka", b["cov"])[1:]
    ratio = da / db
    # the model's ratio at the same float32 poses
    T = r["poses"].astype(np.float64)

    def diag(closures):
        X, info = pgm._measurements(n, g["odo_X"], g["odo_info"], closures)
        _, _, H, _ = pgm.linearise(T, pgm.edge_list(n, closures), X, info, pgm.fixed_mask(n))
        return np.diag(np.linalg.inv(H)).reshape(n - 1, 6)
    model_ratio = diag(rw) / diag(c["closures"])
    print("n %d: the marginals' diagonal with the closures reweighted over the clean graph's: %.5f .. %.5f (the model: %.5f .. %.5f), largest difference of the two %.2e"
          % (n, ratio.min(), ratio.max(), model_ratio.min(), model_ratio.max(), np.abs(ratio / model_ratio - 1).max()))
    assert np.abs(ratio / model_ratio - 1).max() <= 1e-6
    assert ratio.max() <= MARGINALS_FACTOR[n] and ratio.min() >= 1.0 / MARGINALS_FACTOR[n]
    # covariances=True of a robust call is this
    rr = _run(ctx, g, prm.CAUCHY, gn_iters=30, solver="direct", covariances=True)
    assert rr["cov_status"] == 0 and np.array_equal(_bits(rr["cov"]), _bits(a["cov"]))
