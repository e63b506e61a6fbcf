"""GPU tests of the pose graph's MARGINAL COVARIANCES (-m gpu), through the C ABI: icet_pose_graph_marginals, its _device form and the hook
icet_debug_pose_graph_marginals.  On every graph: checks (a) - (e) of tests/pose_graph_marginals_model.py through the hook, (c) through the public call, and the
device's cov against the plain host build's (tests/cpp/test_posegraph_marginals.cpp) within the bound of (b) -- the host build started from the device's own D,
B, A: the device's Jacobians are the same central differences in another rounding (contracted multiply-adds), which moves D, B, A by 1e-10 relative and the
covariance with them (measured from the poses: 2.2e-10 on n2), the term check (c) allows for; from the same blocks the two differ by the marginals' arithmetic alone.  Then the limit of 128 end nodes, the three
failures with their statuses, and the determinism the interface promises.  The graphs are the smallest at which each part can go wrong:
    n1                       only the fixed node
    n2, n3                   q = 0: the 6 x 6 substitutions and the recurrence alone
    n6                       a fixed interior node inside the recurrence; duplicate and reversed closures; q = 18
    n33, n65, chain65        one node past a staged chunk of 32; two chunks plus one
    m0                       closures on the band only: q = 0 with C > 0
    rank5, strong            singular closure information; cond(H) = 1.6e10
    ends288, ends128         q = 576: beyond one stride of 256 threads; q = 768: the limit itself
Measured on an MI355X: DESIGN.md section 20 has the table."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_direct_model as pdm      # noqa: E402
import pose_graph_marginals_model as pmm      # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["n1", "n2", "n3", "n6", "n33", "n65", "chain65", "m0", "rank5", "strong", "ends288", "ends128"]


@pytest.fixture(scope="module")
def ctx():
    import icet_amd
    c = icet_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx):
    """name -> the hook's result on the device."""
    return {k: ctx.debug_pose_graph_marginals(*_args(g), fixed=g["fixed"]) for k, g in ((k, pmm.graphs()[k]) for k in NAMES)}


@pytest.fixture(scope="module")
def host(dev, tmp_path_factory):
    """The plain host build's results from the device's own D, B, A (one compilation, one run)."""
    res = pmm.host_run_blocks(tmp_path_factory.mktemp("pg_marginals_ref"), [(pmm.graphs()[k], dev[k]["D"], dev[k]["B"], dev[k]["A"]) for k in NAMES])
    return dict(zip(NAMES, res))


def _args(g):
    return (g["poses"], g["odo_X"], g["odo_info"], g["closures"])


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


@pytest.mark.parametrize("name", NAMES)
def test_device_marginals(ctx, dev, host, name):
    g, r = pmm.graphs()[name], dev[name]
    m = pmm.context(name, g, r)
    pmm.check_status(r, m)
    pmm.check_a(r, m)
    b = pmm.check_b(r, m)
    pmm.check_c(r["cov"], m)
    pmm.check_d(r["cov"], m)
    if g["closures"]:
        ch = ctx.debug_pose_graph_marginals(g["poses"], g["odo_X"], g["odo_info"], (), fixed=g["fixed"])
        pmm.check_e(r["cov"], ch["cov"], m, b["b_bound"])
    if not pdm.graph_ends(g):
        assert np.array_equal(_bits(r["cov"][m["free"]]), _bits(r["band_cov"][m["free"]]))
    # the public call: the hook's bits, and (c) on its own
    w = ctx.pose_graph_marginals(*_args(g), fixed=g["fixed"])
    assert w["status"] == 0 and w["m"] == r["m"] and np.array_equal(_bits(w["cov"]), _bits(r["cov"]))
    pmm.check_c(w["cov"], m); pmm.check_d(w["cov"], m)
    # against the plain host build, within the bound of (b)
    if m["free"].size:
        d = pmm.scaled(r["cov"][m["free"]], host[name]["cov"][m["free"]])
        print("  %s: the device's cov is %.3e from the host build's (bound %.3e)" % (name, d, b["b_bound"]))
        assert d <= b["b_bound"]
    else:
        assert not r["cov"].any() and r["status"] == 0


def test_the_smallest_graphs(ctx):
    g = pmm.graphs()["n2"]
    r = ctx.debug_pose_graph_marginals(*_args(g), fixed=g["fixed"])
    assert pmm.scaled(r["cov"][1:], np.linalg.inv(r["D"][1])[None]) <= 1e-14


def test_over_the_limit(ctx):
    from icet_amd import api
    g = pdm.over_limit_graph()
    n = g["poses"].shape[0]
    with pytest.raises(api.IcetError) as e:
        ctx.pose_graph_marginals(*_args(g), fixed=g["fixed"])
    assert e.value.status == api.ICET_ERR_UNSUPPORTED
    # the outputs untouched, whatever pg_solver says: through the library itself
    import ctypes as C
    import icet_amd
    lib = icet_amd.load_library()
    pg = ctx._pose_graph_host(g["poses"], g["odo_X"], g["odo_info"], g["closures"], None)
    for solver in ("cg", "direct", "auto"):
        with ctx._pose_graph_solver(solver):
            cov = np.full((n, 36), 7.0); res = api.PoseGraphMarginalsResult(5, 5, 5, 5, 5, 5)
            st = lib.icet_pose_graph_marginals(*pg.args, cov.ctypes.data, C.byref(res))
            assert st == api.ICET_ERR_UNSUPPORTED and (cov == 7.0).all() and res.status == 5 and res.reserved == 5


@pytest.mark.parametrize("name", list(pmm.FAILING))
def test_failures_have_their_statuses(ctx, name):
    make, status, which = pmm.FAILING[name]
    g = make()
    pmm.check_failed(ctx.pose_graph_marginals(*_args(g), fixed=g["fixed"]), g, status, which)
    if which == "factor_status":          # (a fixed node beside node 0 is zero, not NaN; the band fails with it as without)
        fx = np.zeros(g["poses"].shape[0], np.uint8); fx[5] = 1
        r = ctx.debug_pose_graph_marginals(*_args(g), fixed=fx)
        pmm.check_failed(r, dict(g, fixed=fx), status, which)
        assert np.isnan(r["band_cov"]).all()          # (left as the caller passed it)


def test_the_measurements_do_not_enter(ctx):
    g = pmm.graphs()["n33"]
    w = ctx.pose_graph_marginals(*_args(g), fixed=g["fixed"])
    rng = np.random.default_rng(4)
    oX = g["odo_X"] + rng.standard_normal(g["odo_X"].shape).astype(np.float32)
    cl = [(i, j, np.asarray(X, np.float32) + 1.0, info) for (i, j, X, info) in g["closures"]]
    v = ctx.pose_graph_marginals(g["poses"], oX, g["odo_info"], cl, fixed=g["fixed"])
    assert v["status"] == 0 and np.array_equal(_bits(v["cov"]), _bits(w["cov"]))


def test_determinism(ctx):
    """Two calls, the host-pointer and the device-pointer form, and a call behind an icet_solve on the same context: the same bits."""
    g = pmm.graphs()["n65"]
    w = ctx.pose_graph_marginals(*_args(g), fixed=g["fixed"])
    assert np.array_equal(_bits(ctx.pose_graph_marginals(*_args(g), fixed=g["fixed"])["cov"]), _bits(w["cov"]))
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(dev) for k in ("poses", "odo_X", "odo_info")]
    d = ctx.pose_graph_marginals_device(*t, g["closures"], fixed=g["fixed"])
    assert d["status"] == 0 and d["cov"].is_cuda and np.array_equal(_bits(d["cov"].cpu().numpy()), _bits(w["cov"]))
    s = np.load(os.path.join(pdm.ROOT, "tests", "golden", "scans_frame_804_805.npz"))
    x0 = np.zeros(6, np.float32)
    before = ctx.solve(s["scan1"], s["scan2"], 3, x0, 24, 75)
    again = ctx.pose_graph_marginals(*_args(g), fixed=g["fixed"])
    after = ctx.solve(s["scan1"], s["scan2"], 3, x0, 24, 75)
    assert np.array_equal(_bits(again["cov"]), _bits(w["cov"]))
    assert np.array_equal(before["X"].view(np.uint32), after["X"].view(np.uint32))


def test_optimize_with_covariances(ctx):
    g = pmm.graphs()["n33"]
    plain = ctx.optimize_pose_graph(*_args(g), fixed=g["fixed"], solver="direct")
    assert "cov" not in plain and "cov_status" not in plain
    w = ctx.optimize_pose_graph(*_args(g), fixed=g["fixed"], solver="direct", covariances=True)
    assert set(w) == set(plain) | {"cov", "cov_status"} and w["cov_status"] == 0
    assert np.array_equal(w["poses"].view(np.uint32), plain["poses"].view(np.uint32))
    sep = ctx.pose_graph_marginals(w["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"])
    assert np.array_equal(_bits(w["cov"]), _bits(sep["cov"]))
    from icet_amd import api
    sd = api.pose_stds(w["cov"])
    assert sd.shape == (33, 6) and not sd[0].any() and (sd[1:] > 0).all()
