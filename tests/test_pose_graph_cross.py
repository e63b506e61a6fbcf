"""GPU tests of the pose graph's COVARIANCE COLUMNS and GATE (-m gpu), through the C ABI: icet_pose_graph_covariance_columns, icet_pose_graph_gate and their
_device forms.  On every graph checks (a) - (f) of tests/pose_graph_cross_model.py: the columns against the inverse of the dense H from the run's own D, B, A
(the marginals' hook on the same inputs; cov_out equal to the hook's cov bit for bit ties the two runs together), against the model's H, against each other
across two targets, the joint 12 x 12 covariances, the exact bits, and the device against the plain host build started from the device's D, B, A.  Then the
gate against the model on n6, n33 and strong, the anchor property, the refused calls and the three failures.  The graphs and their targets are the smallest at
which each part can go wrong:
    n1                       the target is the fixed node: all zeros
    n2, n3                   q = 0: Zt alone (T = 1 on n2)
    n6                       fixed node 4 as a target and as a row; duplicate and reversed closures
    n33, n65, chain65        targets 0, 31, 32, 33 and the last node, either side of a staged chunk of 32
    m0                       closures on the band only
    rank5, strong            singular closure information; cond(H) = 1.6e10
    ends288                  q = 576, past one stride of 256 threads; targets include an end node and a node that is not one
    ends128                  q = 768 with T = 32: both limits at once
Measured on an MI355X: DESIGN.md section 20 has the table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cross_model as pxm      # noqa: E402
import pose_graph_direct_model as pdm      # noqa: E402
import pose_graph_marginals_model as pmm      # noqa: E402
import pose_graph_model as pgm      # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["n1", "n2", "n3", "n6", "n33", "n65", "chain65", "m0", "rank5", "strong", "ends288", "ends128"]
bits = pxm.bits


@pytest.fixture(scope="module")
def ctx():
    import icet_amd
    c = icet_amd.Context(0)
    yield c
    c.close()


def _args(g):
    return (g["poses"], g["odo_X"], g["odo_info"], g["closures"])


@pytest.fixture(scope="module")
def hook(ctx):
    """name -> the marginals' hook on the device: D, B, A and cov on the same inputs."""
    return {k: ctx.debug_pose_graph_marginals(*_args(g), fixed=g["fixed"]) for k, g in ((k, pxm.graphs()[k]) for k in NAMES)}


@pytest.fixture(scope="module")
def dev(ctx):
    """name -> the columns on the device."""
    return {k: ctx.pose_graph_covariance_columns(*_args(g), targets=pxm.TARGETS[k], fixed=g["fixed"]) for k, g in ((k, pxm.graphs()[k]) for k in NAMES)}


@pytest.fixture(scope="module")
def host(hook, tmp_path_factory):
    """The plain host build's columns from the device's own D, B, A (one compilation, one run)."""
    res = pxm.host_run_blocks(tmp_path_factory.mktemp("pg_cross_ref"), [(pxm.graphs()[k], pxm.TARGETS[k], hook[k]["D"], hook[k]["B"], hook[k]["A"]) for k in NAMES])
    return dict(zip(NAMES, res))


@pytest.mark.parametrize("name", NAMES)
def test_device_columns(dev, hook, host, name):
    g, r, h = pxm.graphs()[name], dev[name], hook[name]
    m = pxm.context(name, g)
    assert r["status"] == 0 and r["m"] == h["m"] and r["cols"].shape == (len(m["targets"]), m["n"], 6, 6)
    assert np.array_equal(bits(r["cov"]), bits(h["cov"]))          # the marginals' bits: the hook's D, B, A are this run's
    ba = pxm.check_a(r["cols"], h, m)
    pxm.check_b(r["cols"], m)
    pxm.check_c(r["cols"], r["cov"], m, ba)
    pxm.check_d(r["cols"], r["cov"], m, ba)
    pxm.check_e(r["cols"], r["cov"], m)
    pxm.check_f(r["cols"], host[name], m, ba)
    if m["free"].size == 0:
        assert not bits(r["cols"]).any()


def test_exact_bits(ctx, dev):
    """Two calls, the _device form, the marginals' own call, a call without cov_out, and a call between two solves: the same bits; the solves do not move."""
    name = "n65"
    g, w = pxm.graphs()[name], dev[name]
    t = pxm.TARGETS[name]
    again = ctx.pose_graph_covariance_columns(*_args(g), targets=t, fixed=g["fixed"])
    assert np.array_equal(bits(again["cols"]), bits(w["cols"])) and np.array_equal(bits(again["cov"]), bits(w["cov"]))
    assert np.array_equal(bits(ctx.pose_graph_marginals(*_args(g), fixed=g["fixed"])["cov"]), bits(w["cov"]))
    d = torch.device("cuda", 0)
    tt = [torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(d) for k in ("poses", "odo_X", "odo_info")]
    dv = ctx.pose_graph_covariance_columns_device(*tt, g["closures"], targets=t, fixed=g["fixed"])
    assert dv["status"] == 0 and dv["cols"].is_cuda
    assert np.array_equal(bits(dv["cols"].cpu().numpy()), bits(w["cols"])) and np.array_equal(bits(dv["cov"].cpu().numpy()), bits(w["cov"]))
    # cov_out may be NULL, in both forms; one target alone gives its column of the five
    import icet_amd
    from icet_amd import api
    lib = icet_amd.load_library()
    pg = ctx._pose_graph_host(*_args(g), g["fixed"])
    one = np.ascontiguousarray([t[2]], np.int32); cols = np.full((1, 65, 6, 6), 7.0); res = api.PoseGraphMarginalsResult()
    assert lib.icet_pose_graph_covariance_columns(*pg.args, 1, one.ctypes.data, cols.ctypes.data, None, C.byref(res)) == api.ICET_OK and res.status == 0
    assert np.array_equal(bits(cols[0]), bits(w["cols"][2]))
    pgd = ctx._pose_graph_device(*tt, g["closures"], g["fixed"], None, None)
    dcols = torch.full((1, 65, 6, 6), 7.0, dtype=torch.float64, device=d)
    assert lib.icet_pose_graph_covariance_columns_device(*pgd.args, 1, one.ctypes.data, dcols.data_ptr(), None, C.byref(res)) == api.ICET_OK
    assert np.array_equal(bits(dcols.cpu().numpy()[0]), bits(w["cols"][2]))
    # between two solves
    s = np.load(os.path.join(pdm.ROOT, "tests", "golden", "scans_frame_804_805.npz"))
    x0 = np.zeros(6, np.float32)
    before = ctx.solve(s["scan1"], s["scan2"], 3, x0, 24, 75)
    mid = ctx.pose_graph_covariance_columns(*_args(g), targets=t, fixed=g["fixed"])
    after = ctx.solve(s["scan1"], s["scan2"], 3, x0, 24, 75)
    assert np.array_equal(bits(mid["cols"]), bits(w["cols"]))
    assert np.array_equal(before["X"].view(np.uint32), after["X"].view(np.uint32))


@pytest.mark.parametrize("name", pxm.GATE_GRAPHS)
def test_device_gate(ctx, name):
    g, cands = pxm.graphs()[name], pxm.candidates(name)
    r = ctx.pose_graph_gate(*_args(g), cands, fixed=g["fixed"])
    assert r["status"] == 0 and r["n_targets"] == len(pxm.gate_targets(cands)) and r["threshold"] == pxm.DEFAULT_THRESHOLD
    pxm.check_gate(name, r, cands)
    pxm.check_symmetric_bits(r["res_cov"])
    d2 = r["d2"]
    assert d2[0] < r["threshold"] and d2[1] < r["threshold"] and d2[2] > r["threshold"] and r["rejected"] >= 1
    assert r["accepted"][0] and r["accepted"][1] and not r["accepted"][2]
    assert np.array_equal(r["accepted"], (d2 < r["threshold"]) & (r["cand_status"] == 0))
    if name == "n6":          # both ends fixed: S is the symmetrised covariance bit for bit; with a zero covariance status 2 and NaN
        c = pxm.GATE_COV.astype(np.float64)
        assert np.array_equal(bits(r["res_cov"][6]), bits(0.5 * (c + c.T)))
        assert r["cand_status"][7] == pgm.NOT_POSITIVE_DEFINITE and bits(d2[7:8])[0] == pxm.QNAN and not r["res_cov"][7].any() and not r["accepted"][7]
    # a threshold of its own; the same bits run to run, through the _device form, and without res_cov_out
    low = ctx.pose_graph_gate(*_args(g), cands, fixed=g["fixed"], threshold=1e-3)
    assert np.array_equal(bits(low["d2"]), bits(d2)) and low["rejected"] == len(cands) and not low["accepted"].any()
    d = torch.device("cuda", 0)
    tt = [torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(d) for k in ("poses", "odo_X", "odo_info")]
    cX = torch.from_numpy(np.array([c[2] for c in cands], np.float32)).to(d); cC = torch.from_numpy(np.array([c[3] for c in cands], np.float32)).to(d)
    dv = ctx.pose_graph_gate_device(*tt, g["closures"], [c[0] for c in cands], [c[1] for c in cands], cX, cC, fixed=g["fixed"])
    assert dv["rejected"] == r["rejected"] and np.array_equal(bits(dv["d2"].cpu().numpy()), bits(d2))
    assert np.array_equal(bits(dv["res_cov"].cpu().numpy()), bits(r["res_cov"])) and np.array_equal(dv["cand_status"].cpu().numpy(), r["cand_status"])
    assert np.array_equal(dv["accepted"].cpu().numpy(), r["accepted"])


def test_device_anchor(ctx):
    """S of candidate (20, 50) in chain65 equals S of candidate (0, 30) in the sub-chain 20 .. 50, within the bound of (b)."""
    g, c, sub, cs = pxm.anchor_graphs()
    full = ctx.pose_graph_gate(*_args(g), c)
    part = ctx.pose_graph_gate(*_args(sub), cs)
    d = pxm.scaled_s(full["res_cov"], part["res_cov"])
    print("  anchor: S in the chain is %.3e from S in the sub-chain (bound %.3e); d2 %.6f and %.6f" % (d, pxm.anchor_bound(), full["d2"][0], part["d2"][0]))
    assert full["status"] == 0 and part["status"] == 0 and d <= pxm.anchor_bound()


def _columns_raw(lib, pg, n, T, targets, cols=True, result=True):
    from icet_amd import api
    t = None if targets is None else np.ascontiguousarray(targets, np.int32)
    out = np.full((max(T, 1), n, 36), 7.0); cov = np.full((n, 36), 7.0); res = api.PoseGraphMarginalsResult(5, 5, 5, 5, 5, 5)
    st = lib.icet_pose_graph_covariance_columns(*pg.args, T, None if t is None else t.ctypes.data, out.ctypes.data if cols else None, cov.ctypes.data,
                                                C.byref(res) if result else None)
    assert (out == 7.0).all() and (cov == 7.0).all() and res.status == 5 and res.reserved == 5
    return st


def test_refused_calls(ctx):
    """Each ICET_ERR_BAD_ARG case and the limit of 128 end nodes under each pg_solver: the outputs pre-filled with 7.0 are untouched."""
    import icet_amd
    from icet_amd import api
    lib = icet_amd.load_library()
    g = pxm.graphs()["n33"]
    pg = ctx._pose_graph_host(*_args(g), g["fixed"])
    bad = api.ICET_ERR_BAD_ARG
    assert _columns_raw(lib, pg, 33, 0, []) == bad
    assert _columns_raw(lib, pg, 33, 33, list(range(33))) == bad
    assert _columns_raw(lib, pg, 33, 2, [1, 33]) == bad
    assert _columns_raw(lib, pg, 33, 2, [-1, 3]) == bad
    assert _columns_raw(lib, pg, 33, 3, [4, 9, 4]) == bad
    assert _columns_raw(lib, pg, 33, 1, None) == bad
    assert _columns_raw(lib, pg, 33, 1, [1], cols=False) == bad
    assert _columns_raw(lib, pg, 33, 1, [1], result=False) == bad
    # the gate
    cands = pxm.candidates("n33")

    def gate_raw(gi, gj, n_cand=None):
        nc = len(gi) if n_cand is None else n_cand
        a = np.ascontiguousarray(gi, np.int32); b = np.ascontiguousarray(gj, np.int32)
        X = np.zeros((max(len(gi), 1), 6), np.float32); cv = np.tile(pxm.GATE_COV.reshape(1, 36), (max(len(gi), 1), 1))
        d2 = np.full(max(len(gi), 1), 7.0); S = np.full((max(len(gi), 1), 36), 7.0); cs = np.full(max(len(gi), 1), 7, np.int32); res = api.PoseGraphGateResult()
        res.rejected = 5
        st = lib.icet_pose_graph_gate(*pg.args, nc, a.ctypes.data, b.ctypes.data, X.ctypes.data, cv.ctypes.data, 0.0, d2.ctypes.data, S.ctypes.data, cs.ctypes.data, C.byref(res))
        assert (d2 == 7.0).all() and (S == 7.0).all() and (cs == 7).all() and res.rejected == 5
        return st
    assert gate_raw([3], [3]) == bad and gate_raw([3], [33]) == bad and gate_raw([-1], [3]) == bad and gate_raw([3], [4], n_cand=0) == bad
    assert gate_raw([0] * 513, [1] * 513) == bad
    g65 = pxm.graphs()["n65"]
    pg = ctx._pose_graph_host(*_args(g65), g65["fixed"])
    assert gate_raw([0] * 33, list(range(1, 34))) == bad          # 33 distinct live nodes
    # more than 128 end nodes, whatever pg_solver says
    go = pdm.over_limit_graph()
    n = go["poses"].shape[0]
    pg = ctx._pose_graph_host(*_args(go), go["fixed"])
    for solver in ("cg", "direct", "auto"):
        with ctx._pose_graph_solver(solver):
            assert _columns_raw(lib, pg, n, 2, [1, 5]) == api.ICET_ERR_UNSUPPORTED
            assert gate_raw([1], [5]) == api.ICET_ERR_UNSUPPORTED
    with pytest.raises(api.IcetError) as e:
        ctx.pose_graph_covariance_columns(*_args(go), targets=[1], fixed=go["fixed"])
    assert e.value.status == api.ICET_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", list(pmm.FAILING))
def test_failures_have_their_statuses(ctx, name):
    make, status, which = pmm.FAILING[name]
    g = make()
    r = ctx.pose_graph_covariance_columns(*_args(g), targets=pxm.FAILING_TARGETS, fixed=g["fixed"])
    assert r["status"] == status and r[which] == status
    pxm.check_failed(r["cols"], r["cov"], g, pxm.FAILING_TARGETS)
    if which == "factor_status":          # (a fixed node beside node 0, as a row and as a target, is zero, not NaN; the band fails with it as without)
        fx = np.zeros(g["poses"].shape[0], np.uint8); fx[5] = 1
        r = ctx.pose_graph_covariance_columns(*_args(g), targets=pxm.FAILING_TARGETS, fixed=fx)
        assert r["status"] == status
        pxm.check_failed(r["cols"], r["cov"], dict(g, fixed=fx), pxm.FAILING_TARGETS)
    # the gate behind a failed factorisation: NaN, and every candidate rejected
    c = [pxm.revisit(pxm.graphs()["rank5"], 3, 8)]
    gr = ctx.pose_graph_gate(*_args(g), c, fixed=g["fixed"])
    assert gr["status"] == status and np.isnan(gr["d2"]).all() and gr["rejected"] == 1 and not gr["accepted"].any()
