"""What the robust pose-graph tests share (tests/test_pose_graph_robust_model.py and tests/test_pose_graph_robust_host.py on the CPU, tests/test_pose_graph_robust.py
on the GPU): the graphs with planted false closures, the NumPy model's answer to each run (computed once per process), the bounds and where they come from, and the
binary files tests/cpp/test_posegraph_robust.cpp reads and writes."""
import functools
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc      # noqa: E402
import pose_graph_model as pgm      # noqa: E402
import pose_graph_robust_model as prm      # noqa: E402

SCALE = prm.DEFAULT_SCALE
# what a planted false closure's X is displaced by; the sign alternates with the closure's index in the list
DISPLACEMENT = np.array([2.0, -1.5, 0.3, 0.0, 0.0, 0.4])

# the outcome conditions of a robust run (measured worst cases in the model: 8.4e-4 m / 6.2e-5 rad against the clean optimum, good weights >= 0.76, odometry >= 0.92)
CLEAN_T, CLEAN_R = 2e-3, 2e-4
FALSE_WEIGHT_MAX, GOOD_WEIGHT_MIN = 1e-3, 0.5
PLAIN_OFF_M = 1.0
HUBER_GAIN = 5.0

# FIXED-ITERATION RUNS against the model.  Measured: the largest distance of the host build (g++ -O2 -ffp-contract=off, one thread) from the model over every
# fixed-iteration run of fixed_runs() x both solvers -- poses64 in metres and radians, weights and costs relative.  The bound is 16 x the measured value (the
# project's margin over a reference's worst case, DESIGN.md section 20 "the band solve"), and never above pc.CAP_T / pc.CAP_R for poses or 1e-6 relative for
# weights and costs.
# (tests/test_pose_graph_robust_host.py prints the figures of its run beside these: 148 runs.  The largest pose distances belong to runs that are far from
# converged -- the plain kind's steps from a start metres off, at n = 65 and n = 257 --, the largest weight distance to a Geman-McClure weight three iterations in.)
MEASURED_HOST = dict(t=7.0e-9, r=1.1e-9, w=2.1e-9, cost=1.8e-9)
MARGIN = 16.0


def bounds():
    b = dict(t=MARGIN * MEASURED_HOST["t"], r=MARGIN * MEASURED_HOST["r"], w=MARGIN * MEASURED_HOST["w"], cost=MARGIN * MEASURED_HOST["cost"])
    assert b["t"] <= pc.CAP_T and b["r"] <= pc.CAP_R and b["w"] <= 1e-6 and b["cost"] <= 1e-6
    return b


@functools.lru_cache(maxsize=None)
def planted(n, good, bad):
    """make_loop(n, good + bad, seed=11) with DISPLACEMENT added to the bad closures' X, the sign alternating with the closure's index.  dict of the graph
    with n_good, n_bad."""
    g = pgm.make_loop(n, list(good) + list(bad), seed=11)
    closures = []
    for q, (i, j, X, info) in enumerate(g["closures"]):
        if q >= len(good):
            X = (X.astype(np.float64) + (1.0 if q % 2 == 0 else -1.0) * DISPLACEMENT).astype(np.float32)
        closures.append((i, j, X, info))
    return dict(g, closures=closures, fixed=None, n_good=len(good), n_bad=len(bad))


@functools.lru_cache(maxsize=None)
def clean(n, good):
    """The same graph without the false closures (the same seed gives the same odometry and the same good closures)."""
    g = planted(n, good, ())
    return g


# the planted graphs of DESIGN.md section 20 "Robust kernels": (n, good closures, planted false closures)
TABLE = [(12, ((0, 11), (1, 10)), ((3, 8),)),
         (33, ((0, 32), (2, 30), (5, 27)), ((8, 20), (12, 25))),
         (65, ((0, 64), (3, 60), (10, 50), (20, 40)), ((15, 45), (25, 55)))]
BIG = (257, ((0, 256), (5, 250)), ((60, 200),))          # E = 259: crosses the 256-lane stride of the reduction


def fixed6_graph():
    """The 6-node graph of pose_graph_cases (duplicates, a reversed closure, node 4 fixed) with one closure displaced."""
    n, pairs, fx = pc.CASES[3]
    g = dict(pc.graph(n, pairs, fx, True))
    closures = list(g["closures"])
    i, j, X, info = closures[3]
    closures[3] = (i, j, (X.astype(np.float64) + DISPLACEMENT).astype(np.float32), info)
    return dict(g, closures=closures, n_good=len(closures) - 1, n_bad=1)


@functools.lru_cache(maxsize=None)
def graphs():
    """name -> (graph, flags): every graph the fixed-iteration runs use."""
    out = {}
    out["n2"] = (dict(pgm.make_loop(2, [], seed=11), fixed=None, n_good=0, n_bad=0), prm.ROBUST_ODOMETRY)          # E = 1
    out["n3"] = (dict(pgm.make_loop(3, [(0, 2)], seed=11), fixed=None, n_good=1, n_bad=0), 0)
    out["n6"] = (fixed6_graph(), 0)
    for (n, good, bad) in TABLE + [BIG]:
        out["n%d" % n] = (planted(n, good, bad), 0)
    out["n33odo"] = (planted(*TABLE[1]), prm.ROBUST_ODOMETRY)
    return out


def fixed_runs():
    """[(graph name, kind, gn_iters)]: dx_tol = 0, so every run ends at the iteration cap.  K = 1 and 3 for every kind, 6 for Cauchy and Geman-McClure (Huber is
    at rounding level by iteration 6 and stalls there), on every graph but n2."""
    runs = []
    for name in graphs():
        for kind in (prm.NONE, prm.HUBER, prm.CAUCHY, prm.GEMAN_MCCLURE):
            for K in (1, 3, 6):
                if K == 6 and kind not in (prm.CAUCHY, prm.GEMAN_MCCLURE):
                    continue
                if name == "n2" and K > 1:
                    continue          # (its start is the chain of its only edge: the first step is 1.4e-7, the second rounding, the third is refused -- no cap to run to)
                runs.append((name, kind, K))
    return runs


_MODEL = {}


def model(name, kind, gn_iters=10, dx_tol=pc.DX_TOL, graph=None, flags=None):
    """prm.optimise of a named graph (or `graph` under the key `name`), once per process and key."""
    key = (name, kind, gn_iters, dx_tol, flags)
    if key not in _MODEL:
        g, fl = graphs()[name] if graph is None else (graph, 0)
        fl = fl if flags is None else flags
        _MODEL[key] = prm.optimise(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], gn_iters=gn_iters, dx_tol=dx_tol, kind=kind, scale=SCALE, flags=fl)
    return _MODEL[key]


# ---- the files of tests/cpp/test_posegraph_robust.cpp ----------------------------------------------------------------------------------------------------------
def write_runs(path, items):
    """items = [(graph, options dict (pose_graph_cases._write_graph's keys), kind, flags, scale, direct)]: per run the graph record of
    test_posegraph_optimize.cpp, then int32 kind, flags, direct, 0 | double scale."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(items)))
        for g, o, kind, flags, scale, direct in items:
            pc._write_graph(f, g, o)
            f.write(struct.pack("<iiiid", kind, flags, int(direct), 0, scale))


def read_runs(path, items):
    """Per run: int32 status, gn_iterations, pcg_iterations, solver, downweighted, 0 | double chi2_initial, chi2_final, max_dx, cost_initial, cost_final |
    float poses[n x 16] | double poses64[n x 12], edge_chi2[2 x E], edge_weight[E]."""
    raw = open(path, "rb").read()
    pos, out = 0, []
    for it in items:
        g = it[0]
        n = g["poses"].shape[0]; E = n - 1 + len(g["closures"])
        hd = struct.unpack_from("<6i", raw, pos); pos += 24
        dd = struct.unpack_from("<5d", raw, pos); pos += 40
        poses = np.frombuffer(raw, np.float32, n * 16, pos).reshape(n, 4, 4); pos += n * 64
        p64 = np.frombuffer(raw, np.float64, n * 12, pos).reshape(n, 12); pos += n * 96
        chi = np.frombuffer(raw, np.float64, 2 * E, pos).reshape(2, E); pos += 16 * E
        w = np.frombuffer(raw, np.float64, E, pos); pos += 8 * E
        out.append(dict(status=hd[0], gn_iterations=hd[1], pcg_iterations=hd[2], solver=hd[3], downweighted=hd[4], chi2_initial=dd[0], chi2_final=dd[1], max_dx=dd[2],
                        cost_initial=dd[3], cost_final=dd[4], poses=poses, poses64=pc.poses64_matrix(p64), edge_chi2=chi, edge_weight=w))
    assert pos == len(raw)
    return out


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def cost_floor(g):
    """Below this a sum of chi2 is the rounding of its residuals and nothing else: a residual e = x - X carries an absolute error of a few eps |X| whatever its
    size, so chi2 = e^T Omega e has the floor sum_edges trace(Omega) (4 eps max(1, |X|))^2.  (n = 2 without a closure starts at its chain: its chi2 after one
    step is 1e-27, between 1e-4 and 1e-2 of this floor, on the host and in the model alike -- no relative comparison means anything there.)"""
    X = [np.asarray(x, np.float64) for x in np.asarray(g["odo_X"], np.float64).reshape(-1, 6)] + [np.asarray(c[2], np.float64) for c in g["closures"]]
    info = [np.asarray(m, np.float64).reshape(6, 6) for m in np.asarray(g["odo_info"], np.float64).reshape(-1, 6, 6)] + [np.asarray(c[3], np.float64).reshape(6, 6) for c in g["closures"]]
    return float(sum(np.trace(om) * (4 * np.finfo(np.float64).eps * max(1.0, np.abs(x).max())) ** 2 for x, om in zip(X, info)))


def rel_cost(a, b, floor):
    """|a - b| / |b|, or 0 where both lie under the floor."""
    if abs(a) <= floor and abs(b) <= floor:
        return 0.0
    return rel(a, b)


def distance(r, m, g):
    """How far a result is from the model's: dict(t, r: poses64 in metres and radians; w: the weights, relative; cost: cost_final and the raw chi2_final, relative
    where they are above cost_floor(g))."""
    dt, dr = pgm.pose_error(r["poses64"], m["poses64"])
    fl = cost_floor(g)
    return dict(t=dt, r=dr, w=rel(r["edge_weight"], m["edge_weight"]), cost=max(rel_cost(r["cost_final"], m["cost_final"], fl), rel_cost(r["chi2_final"], m["chi2_final"], fl)))


def check_fixed_run(name, r, m, g, b, worst):
    """One fixed-iteration run on graph g against the model under the bounds b; the figures printed first and folded into `worst`."""
    d = distance(r, m, g)
    print("%s: status %d | %d, iterations %d | %d, poses64 %.3e m %.3e rad, weights %.3e, costs %.3e" % (name, r["status"], m["status"], r["gn_iterations"], m["gn_iterations"],
                                                                                                       d["t"], d["r"], d["w"], d["cost"]))
    for k in worst:
        worst[k] = max(worst[k], d[k])
    assert r["status"] == m["status"] == pgm.ITERATION_CAP and r["gn_iterations"] == m["gn_iterations"]
    assert d["t"] <= b["t"] and d["r"] <= b["r"] and d["w"] <= b["w"] and d["cost"] <= b["cost"], d
    return d


ODOMETRY_WEIGHT_MIN = 0.5


def check_odometry_weights(name, r, g):
    """A converged Cauchy run with ROBUST_ODOMETRY on a planted graph: every odometry edge keeps a weight above ODOMETRY_WEIGHT_MIN (measured least: 0.92),
    every false closure's is below FALSE_WEIGHT_MAX."""
    n = g["poses"].shape[0]
    w = np.asarray(r["edge_weight"])
    print("%s: status %d after %d iterations, least odometry weight %.3f, false weights <= %.3e" % (name, r["status"], r["gn_iterations"], w[:n - 1].min(), w[n - 1 + g["n_good"]:].max()))
    assert r["status"] == pgm.CONVERGED
    assert (w[:n - 1] > ODOMETRY_WEIGHT_MIN).all() and (w[:n - 1] < 1.0).any()
    assert (w[n - 1 + g["n_good"]:] < FALSE_WEIGHT_MAX).all() and r["downweighted"] == g["n_bad"]


def check_outcome(name, r, g, clean_poses64):
    """The outcome conditions of a converged Cauchy or Geman-McClure run on a planted graph: within CLEAN_T / CLEAN_R of the clean graph's optimum, every false
    closure's weight below FALSE_WEIGHT_MAX, every good closure's above GOOD_WEIGHT_MIN."""
    n = g["poses"].shape[0]
    dt, dr = pgm.pose_error(r["poses64"], clean_poses64)
    wc = np.asarray(r["edge_weight"])[n - 1:]
    good, bad = wc[:g["n_good"]], wc[g["n_good"]:]
    print("%s: status %d after %d iterations, %.3e m %.3e rad from the clean optimum, false weights <= %.3e, good weights >= %.3f, downweighted %d"
          % (name, r["status"], r["gn_iterations"], dt, dr, bad.max() if bad.size else 0.0, good.min() if good.size else 1.0, r["downweighted"]))
    assert r["status"] == pgm.CONVERGED and r["gn_iterations"] <= 30
    assert dt <= CLEAN_T and dr <= CLEAN_R
    assert (bad < FALSE_WEIGHT_MAX).all() and (good > GOOD_WEIGHT_MIN).all()
    assert r["downweighted"] == g["n_bad"]
