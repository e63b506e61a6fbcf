"""CPU tests of the NumPy model of the pose-graph optimiser's robust kernels (tests/pose_graph_robust_model.py): the rule itself, kind 0 against the plain
model, and what the kernels do to graphs with planted false closures -- the conditions the host and device tests then ask of the library's output."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_model as pgm      # noqa: E402
import pose_graph_robust_cases as rc      # noqa: E402
import pose_graph_robust_model as prm      # noqa: E402

C = prm.DEFAULT_SCALE
MODEL_TABLE = rc.TABLE


@pytest.mark.parametrize("kind", [prm.NONE, prm.HUBER, prm.CAUCHY, prm.GEMAN_MCCLURE])
def test_weight_is_the_derivative_of_rho(kind):
    for s in 10.0 ** np.arange(-3, 7):
        for s in (s, 3.3 * s):
            h = 1e-5 * s
            if kind == prm.HUBER and abs(s - C) < 2 * h:
                continue
            d = (prm.rho(kind, C, s + h) - prm.rho(kind, C, s - h)) / (2 * h)
            w = prm.weight(kind, C, s)
            assert abs(d - w) <= 1e-6 * w, (kind, s, d, w)
    assert prm.weight(kind, C, 0.0) == 1.0 and prm.rho(kind, C, 0.0) == 0.0
    assert prm.weight(kind, C, -1.0) == 1.0 and prm.rho(kind, C, -1.0) == -1.0
    assert np.isnan(prm.rho(kind, C, float("nan"))) and prm.weight(kind, C, float("nan")) == 1.0
    # small s: every kind is the plain one to first order
    assert abs(prm.rho(kind, C, 1e-9) - 1e-9) <= 1e-17 and abs(prm.weight(kind, C, 1e-9) - 1.0) <= 1e-9


def test_the_model_restates_the_headers():
    """The constants of the model are the ones include/icet_hip.h declares and icet_amd/csrc/icet_posegraph.h uses."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    abi = open(os.path.join(root, "include", "icet_hip.h")).read()
    rule = open(os.path.join(root, "icet_amd", "csrc", "icet_posegraph.h")).read()
    for name, value in (("NONE", prm.NONE), ("HUBER", prm.HUBER), ("CAUCHY", prm.CAUCHY), ("GEMAN_MCCLURE", prm.GEMAN_MCCLURE), ("ODOMETRY", prm.ROBUST_ODOMETRY)):
        assert "#define ICET_PG_ROBUST_%s %d\n" % (name, value) in abi
    assert "#define ICET_PG_ROBUST_DEFAULT_SCALE %s\n" % repr(prm.DEFAULT_SCALE) in abi
    assert "kRobustDefaultScale = %s;" % repr(prm.DEFAULT_SCALE) in rule
    assert "enum RobustKind { kRobustNone = 0, kRobustHuber = 1, kRobustCauchy = 2, kRobustGemanMcClure = 3 };" in rule


def test_huber_is_continuous_at_the_threshold():
    lo, hi = np.nextafter(C, 0.0), np.nextafter(C, np.inf)
    assert prm.rho(prm.HUBER, C, C) == C and prm.weight(prm.HUBER, C, C) == 1.0
    assert abs(prm.rho(prm.HUBER, C, hi) - prm.rho(prm.HUBER, C, lo)) <= 4 * np.spacing(C)
    assert abs(prm.weight(prm.HUBER, C, hi) - 1.0) <= 4 * np.finfo(np.float64).eps


def test_the_device_order_of_a_sum():
    v = np.random.default_rng(0).standard_normal(600)
    assert abs(prm.tree_sum(v) - float(np.sum(v))) <= 1e-12
    assert prm.tree_sum([]) == 0.0 and prm.tree_sum([2.5]) == 2.5


@pytest.mark.parametrize("case", MODEL_TABLE, ids=lambda c: "n%d" % c[0])
def test_kind_zero_is_the_plain_model(case):
    g = rc.planted(*case)
    a = pgm.optimise(g["poses"], g["odo_X"], g["odo_info"], g["closures"], dx_tol=pc.DX_TOL)
    b = rc.model("n%d" % case[0], prm.NONE)
    assert np.array_equal(a["poses64"], b["poses64"]) and a["gn_iterations"] == b["gn_iterations"] and a["status"] == b["status"]
    assert np.array_equal(a["poses"], b["poses"]) and np.array_equal(a["edge_chi2"], b["edge_chi2"])
    assert (b["edge_weight"] == 1.0).all() and b["downweighted"] == 0 and b["cost_final"] == b["chi2_final"]


def _contracts(m):
    """The last two accepted steps contract: max |dx| of the last is at most half that of the step before it."""
    return len(m["steps"]) >= 2 and m["steps"][-1] <= 0.5 * m["steps"][-2]


@pytest.mark.parametrize("case", MODEL_TABLE, ids=lambda c: "n%d" % c[0])
def test_false_closures_are_switched_off(case):
    n, good, bad = case
    name = "n%d" % n
    g = rc.planted(n, good, bad)
    clean = pc.model(("robust_clean", n), rc.clean(n, good))
    plain = rc.model(name, prm.NONE)
    pt, pr = pgm.pose_error(plain["poses64"], g["truth"])
    print("plain: status %d, %.3f m %.3f rad from the truth" % (plain["status"], pt, pr))
    assert plain["status"] == pgm.CONVERGED and pt > rc.PLAIN_OFF_M          # the optimiser reports success on a bent map
    for kind in (prm.CAUCHY, prm.GEMAN_MCCLURE):
        m = rc.model(name, kind, gn_iters=30)
        rc.check_outcome("%s kind %d" % (name, kind), m, g, clean["poses64"])
        # what licenses the 10 dx_tol bound of the converged runs: the iteration contracts at its end, so a run that stops one step earlier or later than
        # another is within twice its last step of it
        print("    last steps", m["steps"][-2:])
        assert _contracts(m)
    hub = rc.model(name, prm.HUBER, gn_iters=30)
    ht, _ = pgm.pose_error(hub["poses64"], g["truth"])
    print("Huber: status %d after %d iterations, %.3f m from the truth (plain %.3f m: %.1f x)" % (hub["status"], hub["gn_iterations"], ht, pt, pt / ht))
    assert hub["status"] == pgm.CONVERGED and rc.HUBER_GAIN * ht <= pt
    odo = rc.model(name, prm.CAUCHY, gn_iters=30, flags=prm.ROBUST_ODOMETRY)
    rc.check_odometry_weights("%s Cauchy, odometry too" % name, odo, g)
