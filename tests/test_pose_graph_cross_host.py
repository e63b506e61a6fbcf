"""CPU tests of the pose graph's COVARIANCE COLUMNS and GATE (-m "not gpu"): pg_columns and pg_gate of icet_posegraph_driver.h over the bodies of
icet_posegraph_cross.h and the marginals', run on the host by tests/cpp/test_posegraph_cross.cpp against heap blocks of the exact sizes: plain, under the
address and undefined-behaviour sanitizers, and with a workgroup of four real threads -- the three must write the same bytes.  Checks (a) - (f) of
tests/pose_graph_cross_model.py on the output ((f) here: the run from its own D, B, A gives the bits of the run from the poses), the gate against the model,
the anchor property, the failures, and the ABI that needs no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cross_model as pxm      # noqa: E402
import pose_graph_marginals_model as pmm      # noqa: E402
import pose_graph_model as pgm      # noqa: E402

NAMES = ["n1", "n2", "n3", "n6", "n33", "n65", "chain65", "m0", "rank5", "strong", "ends288", "ends128", "n257"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return pxm.host_run(tmp_path_factory.mktemp("pg_cross"), NAMES + list(pmm.FAILING))


@pytest.fixture(scope="module")
def host_marginals(tmp_path_factory):
    """The marginals' own host program on the same graphs: the bits cov must carry."""
    return pmm.host_run(tmp_path_factory.mktemp("pg_cross_marg"), NAMES, builds=pmm.pdm.BUILDS[:1])


@pytest.mark.parametrize("name", NAMES)
def test_host_columns(host, host_marginals, name):
    g, r = pxm.graphs()[name], host[name]
    m = pxm.context(name, g)
    pmm.check_status(r, m)
    assert np.array_equal(pxm.bits(r["cov"]), pxm.bits(host_marginals[name]["cov"]))
    ba = pxm.check_a(r["cols"], r, m)
    pxm.check_b(r["cols"], m)
    pxm.check_c(r["cols"], r["cov"], m, ba)
    pxm.check_d(r["cols"], r["cov"], m, ba)
    pxm.check_e(r["cols"], r["cov"], m)


def test_host_columns_from_their_own_blocks(host, tmp_path):
    """(f) on the host: started from the band's factor on the run's own D, B, A the program writes the same columns."""
    names = ["n6", "n33", "ends288"]
    res = pxm.host_run_blocks(tmp_path, [(pxm.graphs()[k], pxm.TARGETS[k], host[k]["D"], host[k]["B"], host[k]["A"]) for k in names])
    for k, r in zip(names, res):
        m = pxm.context(k, pxm.graphs()[k])
        assert np.array_equal(pxm.bits(r["cols"]), pxm.bits(host[k]["cols"]))
        assert pxm.check_f(host[k]["cols"], r, m, 0.0) == 0.0


@pytest.mark.parametrize("name", pxm.GATE_GRAPHS)
def test_host_gate(host, name):
    cands = pxm.candidates(name)
    r = host[name]["gate"]
    assert r["status"] == 0 and r["n_targets"] == len(pxm.gate_targets(cands))
    pxm.check_gate(name, r, cands)
    pxm.check_symmetric_bits(r["res_cov"])
    d2 = r["d2"]
    assert d2[0] < pxm.DEFAULT_THRESHOLD and d2[1] < pxm.DEFAULT_THRESHOLD and d2[2] > pxm.DEFAULT_THRESHOLD and r["rejected"] >= 1
    if name == "n6":          # both ends fixed: S is the symmetrised covariance bit for bit; with a zero covariance status 2 and NaN
        c = pxm.GATE_COV.astype(np.float64)
        assert np.array_equal(pxm.bits(r["res_cov"][6]), pxm.bits(0.5 * (c + c.T)))
        assert r["cand_status"][7] == pgm.NOT_POSITIVE_DEFINITE and pxm.bits(d2[7:8])[0] == pxm.QNAN and not r["res_cov"][7].any()


def test_host_anchor(host):
    """S of candidate (20, 50) in chain65 equals S of candidate (0, 30) in the sub-chain 20 .. 50, within the bound of (b)."""
    d = pxm.scaled_s(host["anchor_full"]["gate"]["res_cov"], host["anchor_sub"]["gate"]["res_cov"])
    print("anchor: %.3e (bound %.3e)" % (d, pxm.anchor_bound()))
    assert d <= pxm.anchor_bound()


@pytest.mark.parametrize("name", list(pmm.FAILING))
def test_host_failures(host, name):
    make, status, which = pmm.FAILING[name]
    r = host[name]
    assert r["status"] == status and r[which] == status
    pxm.check_failed(r["cols"], r["cov"], make(), pxm.FAILING_TARGETS)


def test_abi_of_the_columns_and_the_gate():
    import icet_amd
    from icet_amd import api
    lib = icet_amd.load_library()
    for s in ("icet_pose_graph_covariance_columns", "icet_pose_graph_covariance_columns_device", "icet_pose_graph_gate", "icet_pose_graph_gate_device"):
        assert s in api.EXPORTED_SYMBOLS and getattr(lib, s) is not None
    z = (None, 1, None, None, None, 0, None, None, None, None, None)
    assert lib.icet_pose_graph_covariance_columns(*z, 1, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_pose_graph_covariance_columns_device(*z, 1, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_pose_graph_gate(*z, 1, None, None, None, None, 0.0, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_pose_graph_gate_device(*z, 1, None, None, None, None, 0.0, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert C.sizeof(api.PoseGraphGateResult) == 32 and api.PoseGraphGateResult.n_targets.offset == 24 and api.PoseGraphGateResult.rejected.offset == 28
    assert C.sizeof(api.PoseGraphMarginalsResult) == 24 and C.sizeof(api.PoseGraphMarginalsDebug) == 80


def test_the_python_helpers():
    from icet_amd import api
    rng = np.random.default_rng(3)
    a = rng.standard_normal((12, 12)); joint = a @ a.T
    J = rng.standard_normal((6, 12))
    S = api.relative_cov(J, joint[:6, :6], joint[6:, 6:], joint[:6, 6:])
    assert np.allclose(S, J @ joint @ J.T, rtol=1e-13, atol=0) and np.array_equal(S, S.T)
    recs = [dict(slot=2, accepted=True, X=np.arange(6, dtype=np.float32), cov=np.eye(6, dtype=np.float32)),
            dict(slot=None, accepted=False, X=np.zeros(6, np.float32), cov=np.eye(6, dtype=np.float32)),
            dict(slot=1, accepted=True, X=np.ones(6, np.float32), cov=2 * np.eye(6, dtype=np.float32)),
            dict(slot=0, accepted=False, X=np.ones(6, np.float32), cov=np.eye(6, dtype=np.float32))]
    c = api.closure_candidates(recs, [7, 8, 4, 9], {0: 0, 1: 4, 2: 3})
    e = api.closure_edges(recs, [7, 8, 4, 9], {0: 0, 1: 4, 2: 3})
    assert len(c) == len(e) == 1 and c[0][:2] == e[0][:2] == (3, 7) and np.array_equal(c[0][2], e[0][2])
    assert c[0][3].dtype == np.float32 and np.array_equal(c[0][3], np.eye(6, dtype=np.float32))
