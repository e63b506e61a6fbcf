"""CPU tests of the pose graph's MARGINAL COVARIANCES (-m "not gpu"): pg_marginals of icet_posegraph_driver.h over the bodies of icet_posegraph_body.h,
icet_posegraph_direct.h and icet_posegraph_marginals.h, run on the host by tests/cpp/test_posegraph_marginals.cpp against heap blocks of the exact sizes: plain,
under the address and undefined-behaviour sanitizers, and with a workgroup of four real threads -- the four must write the same bytes.  Checks (a) - (e) of
tests/pose_graph_marginals_model.py on its output, the NumPy restatement against the dense references (f), the checks against four corruptions (g), and the
ABI that needs no device.

Measured on the host build, scaled measure (the bound is 10 x the distance between the two NumPy references, for (c) plus 4 x the Jacobian term):
    graph     (a) band_cov   (b) cov      references   (c) vs model   Jacobian term
    n2        5.9e-16        7.2e-16      7.8e-16      3.3e-10        4.3e-10
    n3        1.3e-15        9.4e-16      6.4e-16      8.2e-10        5.4e-10
    n6        2.2e-15        1.7e-15      2.8e-15      9.5e-10        2.6e-09
    n33       7.4e-15        1.6e-14      2.1e-14      8.7e-10        1.1e-09
    n65       1.2e-14        3.8e-14      5.0e-14      3.6e-09        1.7e-09
    chain65   7.4e-14        7.3e-14      7.3e-14      3.8e-09        4.4e-09
    m0        7.1e-15        2.7e-14      2.5e-14      6.6e-10        1.9e-09
    rank5     1.4e-14        4.1e-14      4.1e-14      8.9e-10        1.8e-09
    strong    5.3e-15        8.9e-10      3.3e-10      1.4e-09        2.3e-09
    ends288   6.6e-15        7.2e-13      6.2e-13      2.9e-09        5.0e-09
    ends128   6.5e-15        1.1e-12      1.3e-12      3.2e-09        3.3e-09
    n257      6.2e-14        5.3e-13      4.7e-13      2.7e-09        2.7e-09
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_direct_model as pdm      # noqa: E402
import pose_graph_marginals_model as pmm      # noqa: E402
import pose_graph_model as pgm      # noqa: E402

NAMES = ["n1", "n2", "n3", "n6", "n33", "n65", "chain65", "m0", "rank5", "strong", "ends288", "ends128", "n257"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return pmm.host_run(tmp_path_factory.mktemp("pg_marginals"), NAMES + list(pmm.FAILING))


@pytest.mark.parametrize("name", NAMES)
def test_host_marginals(host, name):
    g, r = pmm.graphs()[name], host[name]
    m = pmm.context(name, g, r)
    pmm.check_status(r, m)
    pmm.check_a(r, m)
    b = pmm.check_b(r, m)
    pmm.check_c(r["cov"], m)
    pmm.check_d(r["cov"], m)
    pmm.check_d(r["band_cov"][m["free"]], dict(m, is_fixed=np.zeros(m["free"].size, bool), free=np.arange(m["free"].size)))
    if g["closures"]:
        pmm.check_e(r["cov"], host[name + "_chain"]["cov"], m, b["b_bound"])
    if not pdm.graph_ends(g):
        assert np.array_equal(r["cov"][m["free"]].view(np.uint64), r["band_cov"][m["free"]].view(np.uint64))
    assert np.array_equal(r["band_cov"][m["is_fixed"]], np.tile(np.eye(6), (int(m["is_fixed"].sum()), 1, 1)))


def test_the_smallest_graphs(host):
    """n = 1: only the fixed node.  n2: Sigma_1 = D_1^-1."""
    assert host["n1"]["status"] == 0 and not host["n1"]["cov"].any()
    r = host["n2"]
    assert pmm.scaled(r["cov"][1:], np.linalg.inv(r["D"][1])[None]) <= 1e-14


@pytest.mark.parametrize("name", list(pmm.FAILING))
def test_host_failures(host, name):
    make, status, which = pmm.FAILING[name]
    pmm.check_failed(host[name], make(), status, which)


def test_the_graphs_have_the_ends_they_are_named_for():
    assert len(pdm.graph_ends(pmm.ends128_graph())) == 128 == pdm.MAX_ENDS
    assert pdm.graph_ends(pmm.chain65_graph()) == [] and pmm.chain65_graph()["poses"].shape[0] == 65
    assert pdm.graph_ends(pmm.graphs()["n6"]) == [1, 2, 5]


@pytest.mark.parametrize("name", ["n2", "n6", "n33", "rank5", "m0", "ends288", "n257", "strong"])
def test_the_numpy_restatement_against_the_dense_reference(name):
    """(f): the recurrence and the P, Q correction in NumPy on the model's blocks against numpy.linalg.inv of the model's H: as good as the inverse through a
    Cholesky factor is (within 10 x their distance)."""
    g = pmm.graphs()[name]
    n = g["poses"].shape[0]
    closures = list(g["closures"])
    edges = pgm.edge_list(n, closures)
    X, info = pgm._measurements(n, g["odo_X"], g["odo_info"], closures)
    is_fixed = pgm.fixed_mask(n, g["fixed"])
    T = np.asarray(g["poses"], np.float32).reshape(n, 4, 4).astype(np.float64)
    Js, _, H, _ = pgm.linearise(T, edges, X, info, is_fixed)
    D, B, A = pdm.blocks_of(H, Js, info, edges, is_fixed)
    s = pmm.restate(D, B, A, edges, is_fixed)
    o, R = pmm.own(H)
    d = pmm.scaled(s["cov"][~is_fixed], R)
    print("%s: the restatement is %.3e from inv(H), the two references %.3e apart" % (name, d, o))
    assert pmm.MARGIN * o <= pmm.CAP and d <= pmm.MARGIN * o


def _copy(r, **kw):
    return dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}, **kw)


def test_the_checks_bite(host):
    """(g): four corruptions of a correct host result, pure NumPy from the result's own D, B, A: each fails the check it names (which the result itself passes)."""
    name = "n33"
    g, r = pmm.graphs()[name], host[name]
    m = pmm.context(name, g, r)
    pmm.check_a(r, m); pmm.check_b(r, m)
    args = (r["D"], r["B"], r["A"], m["edges"], m["is_fixed"])
    # the + Q Q^T term dropped
    with pytest.raises(AssertionError):
        pmm.check_b(_copy(r, cov=pmm.restate(*args, drop_qq=True)["cov"]), m)
    # the recurrence term left out of one node
    with pytest.raises(AssertionError):
        pmm.check_a(_copy(r, band_cov=pmm.restate(*args, skip_term_at=17)["band_cov"]), m)
    # Y_k transposed
    with pytest.raises(AssertionError):
        pmm.check_a(_copy(r, band_cov=pmm.restate(*args, transpose_y=True)["band_cov"]), m)
    # one end node's columns skipped
    with pytest.raises(AssertionError):
        pmm.check_b(_copy(r, cov=pmm.restate(*args, skip_end=1)["cov"]), m)
    # (and the restatement itself passes both)
    ok = pmm.restate(*args)
    pmm.check_a(_copy(r, band_cov=ok["band_cov"]), m); pmm.check_b(_copy(r, cov=ok["cov"]), m)


def test_abi_of_the_marginals():
    import icet_amd
    from icet_amd import api
    lib = icet_amd.load_library()
    for s in ("icet_pose_graph_marginals", "icet_pose_graph_marginals_device", "icet_debug_pose_graph_marginals"):
        assert s in api.EXPORTED_SYMBOLS and getattr(lib, s) is not None
    assert lib.icet_pose_graph_marginals(None, 1, None, None, None, 0, None, None, None, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_pose_graph_marginals_device(None, 1, None, None, None, 0, None, None, None, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_debug_pose_graph_marginals(None, 1, None, None, None, 0, None, None, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert C.sizeof(api.PoseGraphMarginalsResult) == 24 and api.PoseGraphMarginalsResult.ks_status.offset == 16 and api.PoseGraphMarginalsResult.reserved.offset == 20
    assert C.sizeof(api.PoseGraphMarginalsDebug) == 80 and api.PoseGraphMarginalsDebug.ends.offset == 40 and api.PoseGraphMarginalsDebug.ends_capacity.offset == 48
    assert api.PoseGraphMarginalsDebug.result.offset == 56
    # the structs the feature leaves alone
    assert C.sizeof(api.PoseGraphOptions) == 32 and C.sizeof(api.PoseGraphResult) == 40 and C.sizeof(api.PoseGraphStep) == 152 and C.sizeof(api.PoseGraphDirectStep) == 176


def test_the_python_helpers():
    from icet_amd import api
    rng = np.random.default_rng(2)
    a = rng.standard_normal((3, 6, 6)); cov = a @ a.transpose(0, 2, 1)
    assert np.allclose(api.pose_stds(cov), np.sqrt(np.einsum("kaa->ka", cov)), rtol=0, atol=0)
    poses = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    poses[1] = pgm.exp_se3(np.array([1, 2, 3, 0.3, -0.2, 0.9])).astype(np.float32)
    w = api.position_cov_world(poses, cov)
    assert w.shape == (3, 3, 3) and np.array_equal(w[0], cov[0, :3, :3])
    R = poses[1, :3, :3].astype(np.float64)
    assert np.allclose(w[1], R @ cov[1, :3, :3] @ R.T, rtol=1e-15, atol=0)
