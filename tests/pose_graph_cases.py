"""What the pose-graph optimiser's tests share (tests/test_pose_graph_optimize_host.py on the CPU, tests/test_pose_graph_optimize.py on the GPU): the graphs, the
NumPy model's answer to each (computed once per process), the tolerances and their derivation, and the binary file tests/cpp/test_posegraph_optimize.cpp reads."""
import functools
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_model as pgm      # noqa: E402

DX_TOL = 1e-7
# Both sides stop behind a step below dx_tol of a quadratically convergent iteration: neither is further than dx_tol from the optimum along any coordinate of the
# last step, the two last steps need not be the same one (gn_iterations may differ by one), and a coordinate of poses64 moves by at most the step (translation
# through a rotation of norm 1): 4 dx_tol in metres and radians.
POSE64_TOL = 4 * DX_TOL
# the hard cap no tolerance may exceed: a tenth of the smallest sigma of the graphs
CAP_T, CAP_R = 0.1 * pgm.SIGMA_CLOSURE[0], 0.1 * pgm.SIGMA_CLOSURE[1]
assert POSE64_TOL <= CAP_T and POSE64_TOL <= CAP_R
# chi2 where it exceeds 1: the model and scipy.optimize.least_squares agree to 1e-9 relative (tests/test_pose_graph_model.py); one decade for the inexact CG solve
CHI2_RTOL = 1e-8

# (n, closure pairs, a fixed node beside node 0 or None): 33, 65 and 257 straddle the 32-node chunk of the band sweeps and a 256-thread block
CASES = [(2, (), None), (2, ((0, 1),), None), (3, ((0, 2),), None),
         (6, ((1, 5), (1, 5), (2, 3), (5, 2), (0, 3), (4, 1)), 4),
         (33, ((0, 32), (1, 30), (5, 31)), None),
         (65, ((0, 64), (3, 60), (10, 63), (40, 8)), None),
         (257, ((0, 256), (7, 250), (100, 31), (128, 129), (31, 33)), None)]


def float32_tol(poses):
    """What the float32 poses may differ by beyond POSE64_TOL: two float32 ulps of the largest coordinate."""
    return 2 * float(np.spacing(np.float32(np.abs(np.asarray(poses, np.float32)[:, :3, :]).max())))


@functools.lru_cache(maxsize=None)
def graph(n, pairs, fixed_node, noisy):
    """make_loop(n, pairs, seed=11): `noisy` the graph as it is; otherwise exact measurements with the noisy graph's drifted chain as the start."""
    drifted = pgm.make_loop(n, list(pairs), seed=11, noise=1.0)
    g = drifted if noisy else dict(pgm.make_loop(n, list(pairs), seed=11, noise=0.0), poses=drifted["poses"])
    fixed = None
    if fixed_node is not None:
        fixed = np.zeros(n, np.uint8); fixed[fixed_node] = 1
    return dict(g, fixed=fixed)


_MODEL = {}


def model(key, g, **kw):
    """pgm.optimise of graph g, once per process and key."""
    if key not in _MODEL:
        _MODEL[key] = pgm.optimise(g["poses"], g["odo_X"], g["odo_info"], g["closures"], fixed=g["fixed"], dx_tol=DX_TOL, **kw)
    return _MODEL[key]


def model_options(o):
    """The options of a run that the model knows (it solves exactly: no max_pcg, no pcg_tol)."""
    return {k: v for k, v in o.items() if k in ("gn_iters", "damping")}


def rank5_graph():
    """The 12-node graph of the model's tests with a closure whose information has rank 5."""
    info = pgm.diag_info(*pgm.SIGMA_CLOSURE); info[2, 2] = 0
    return dict(pgm.make_loop(12, [(0, 11), (2, 9)], seed=11, closure_info=[info, None]), fixed=None)


def zero_row_graph():
    """A chain whose odometry information has a zero row and column on every edge, no closure: H is singular."""
    g = dict(pgm.make_loop(12, [], seed=11), fixed=None)
    oi = g["odo_info"].copy(); oi[:, 1, :] = 0; oi[:, :, 1] = 0
    # (a start off the chain's optimum, so that there is a step to ask for)
    return dict(g, odo_info=oi, poses=pgm.make_loop(12, [], seed=12)["poses"])


def nan_graph():
    g = dict(graph(33, CASES[4][1], None, True))
    p = g["poses"].copy(); p[7, 1, 3] = np.nan
    return dict(g, poses=p)


def _write_graph(f, g, o):
    n, C = g["poses"].shape[0], len(g["closures"])
    f.write(struct.pack("<iiii", n, C, o.get("gn_iters", 10), o.get("max_pcg", 0)))
    f.write(struct.pack("<ddd", o.get("dx_tol", DX_TOL), o.get("damping", 0.0), o.get("pcg_tol", 0.0)))
    f.write(np.ascontiguousarray(g["poses"], np.float32).tobytes())
    f.write(np.ascontiguousarray(g["odo_X"], np.float32).tobytes())
    f.write(np.ascontiguousarray(g["odo_info"], np.float32).tobytes())
    f.write(np.array([c[0] for c in g["closures"]], np.int32).tobytes())
    f.write(np.array([c[1] for c in g["closures"]], np.int32).tobytes())
    f.write(np.array([c[2] for c in g["closures"]], np.float32).tobytes())
    f.write(np.array([c[3] for c in g["closures"]], np.float32).tobytes())
    f.write((np.zeros(n, np.uint8) if g["fixed"] is None else np.asarray(g["fixed"], np.uint8)).tobytes())


def write_graphs(path, items):
    """The input file of tests/cpp/test_posegraph_optimize.cpp: items = [(graph, dict(gn_iters=, max_pcg=, dx_tol=, damping=, pcg_tol=))]."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(items)))
        for g, o in items:
            _write_graph(f, g, o)


def stalled_graph():
    """Six poses thrown far from their chain (0.5 m, 3 rad per pose, seeded): the first Gauss-Newton step is kept, the second raises chi2 with a step that is
    not small -- the run ends stalled.  Kept because the model and the host build of the optimiser agree on that (status 4 after two iterations)."""
    g = pgm.make_loop(6, [(0, 5), (1, 4)], seed=11)
    rng = np.random.default_rng(0)
    P = g["poses"].astype(np.float64)
    for k in range(1, 6):
        P[k] = P[k] @ pgm.exp_se3(np.concatenate([0.5 * rng.standard_normal(3), 3.0 * rng.standard_normal(3)]))
    return dict(g, poses=P.astype(np.float32), fixed=None)


def negative_graph(scale=1.0):
    """The 12-node graph with a closure whose information is negative definite: H is not positive definite.  At scale 1 the band is not either (a pivot of its
    factorisation fails); at scale 0.1 the band is and CG meets p.Hp <= 0 (after five band solves on the host build)."""
    return dict(pgm.make_loop(12, [(0, 11), (2, 9)], seed=11, closure_info=[None, -scale * pgm.diag_info(*pgm.SIGMA_CLOSURE)]), fixed=None)


def write_step_graphs(path, items):
    """The input file of the program's `step` mode: items = [(graph, options, p K x n x 6 doubles)]."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(items)))
        for g, o, p in items:
            _write_graph(f, g, o)
            p = np.ascontiguousarray(p, np.float64).reshape(-1, g["poses"].shape[0], 6)
            f.write(struct.pack("<i", p.shape[0])); f.write(p.tobytes())


STEP_ARRAYS = ("J", "res", "chi_start", "chi_trial", "D", "B", "A", "g", "x", "Pt", "q", "cg_scalars")


def read_step_results(path, items):
    """The output file of the `step` mode, one dict per graph with the keys of Context.debug_pose_graph_step."""
    raw = open(path, "rb").read()
    pos, out = 0, []
    for g, _, p in items:
        n, C = g["poses"].shape[0], len(g["closures"])
        E, K = n - 1 + C, np.asarray(p).reshape(-1, n, 6).shape[0]
        hd = struct.unpack_from("<8i", raw, pos); pos += 32
        r = dict(zip(("factor_status", "cg_status", "band_solves", "cg_end", "cap", "c_offband", "trial"), hd))
        r.update(zip(("chi2_start", "chi2_trial", "max_dx"), struct.unpack_from("<ddd", raw, pos))); pos += 24
        shapes = dict(J=(E, 6, 12), res=(E, 6), chi_start=(E,), chi_trial=(E,), D=(n, 6, 6), B=(n, 6, 6), A=(C, 6, 6), g=(n, 6), x=(n, 6), Pt=(n, 12), q=(K, n, 6),
                      cg_scalars=(r["cap"], 2))
        for k in STEP_ARRAYS:
            cnt = int(np.prod(shapes[k]))
            r[k] = np.frombuffer(raw, np.float64, cnt, pos).reshape(shapes[k]); pos += 8 * cnt
        r["cg_scalars"] = r["cg_scalars"][:r["band_solves"]]
        out.append(r)
    assert pos == len(raw)
    return out


def read_results(path, items):
    """The output file of the program, one dict per graph with the keys of Context.optimize_pose_graph."""
    raw = open(path, "rb").read()
    pos, out = 0, []
    for g, _ in items:
        n, E = g["poses"].shape[0], g["poses"].shape[0] - 1 + len(g["closures"])
        status, its, pcg, _ = struct.unpack_from("<iiii", raw, pos); pos += 16
        c0, c1, mdx = struct.unpack_from("<ddd", raw, pos); pos += 24
        poses = np.frombuffer(raw, np.float32, n * 16, pos).reshape(n, 4, 4); pos += n * 64
        p64 = np.frombuffer(raw, np.float64, n * 12, pos).reshape(n, 12); pos += n * 96
        chi = np.frombuffer(raw, np.float64, 2 * E, pos).reshape(2, E); pos += 16 * E
        out.append(dict(status=status, gn_iterations=its, pcg_iterations=pcg, chi2_initial=c0, chi2_final=c1, max_dx=mdx, poses=poses, poses64=poses64_matrix(p64), edge_chi2=chi))
    assert pos == len(raw)
    return out


def poses64_matrix(p12):
    """n x 12 doubles (R row-major, then t) as n x 4 x 4."""
    p12 = np.asarray(p12, np.float64).reshape(-1, 12)
    T = np.zeros((p12.shape[0], 4, 4)); T[:, 3, 3] = 1
    T[:, :3, :3] = p12[:, :9].reshape(-1, 3, 3); T[:, :3, 3] = p12[:, 9:]
    return T


def compare(name, r, m, g):
    """A result of the optimiser against the model's: the assertions of the issue, the measured figures printed first.  Returns the figures."""
    d64 = pgm.pose_error(r["poses64"], m["poses64"])
    d32 = pgm.pose_error(r["poses"], m["poses"])
    chi_rel = abs(r["chi2_final"] - m["chi2_final"]) / m["chi2_final"] if m["chi2_final"] > 0 else 0.0
    print("%s: status %d | %d, iterations %d | %d, band solves %d, poses64 differ by %.3e m %.3e rad, poses by %.3e m %.3e rad, chi2 %.12g | %.12g (rel %.2e)"
          % (name, r["status"], m["status"], r["gn_iterations"], m["gn_iterations"], r["pcg_iterations"], d64[0], d64[1], d32[0], d32[1], r["chi2_final"], m["chi2_final"], chi_rel))
    assert r["status"] == m["status"]
    assert abs(r["gn_iterations"] - m["gn_iterations"]) <= 1
    assert d64[0] <= POSE64_TOL and d64[1] <= POSE64_TOL
    f32 = float32_tol(m["poses"])
    assert d32[0] <= POSE64_TOL + f32 and d32[1] <= POSE64_TOL + f32 and POSE64_TOL + f32 <= min(CAP_T, CAP_R)
    if m["chi2_final"] > 1.0:
        assert chi_rel <= CHI2_RTOL
    else:
        assert r["chi2_final"] <= r["chi2_initial"]
    assert abs(r["edge_chi2"][1].sum() - r["chi2_final"]) <= 1e-12 * max(r["chi2_final"], 1e-300) * max(1, r["edge_chi2"].shape[1])
    assert abs(r["edge_chi2"][0].sum() - r["chi2_initial"]) <= 1e-12 * max(r["chi2_initial"], 1e-300) * max(1, r["edge_chi2"].shape[1])
    is_fixed = np.zeros(g["poses"].shape[0], bool); is_fixed[0] = True
    if g["fixed"] is not None:
        is_fixed |= np.asarray(g["fixed"]) != 0
    assert np.array_equal(r["poses"][is_fixed].view(np.uint32), np.asarray(g["poses"], np.float32)[is_fixed].view(np.uint32))
    assert np.array_equal(r["poses"][~is_fixed][:, 3, :], np.tile(np.float32([0, 0, 0, 1]), (int((~is_fixed).sum()), 1)))
    return dict(d64=d64, d32=d32, chi_rel=chi_rel)


# ---- the graphs of tests/test_pose_graph_step.py: one Gauss-Newton step taken apart -----------------------------------------------------------------------------
SEAM_PAIRS = ((0, 32), (5, 37), (40, 8))
STRONG_RATIO = 4e4        # the strong-closure graph: closure information over the odometry's
STRONG_PAIRS = ((1, 30), (5, 31), (3, 20), (12, 28))


def strong_graph():
    """33 poses, four closures off the band whose information is STRONG_RATIO times the odometry's with every axis within a decade of that (seeded), as a
    registration's own covariance gives: M^-1 H then has eigenvalues spread down to about 1 / STRONG_RATIO, and CG needs more band solves than the default
    cap of 12 x 4 + 8.  (With exactly STRONG_RATIO on every axis the small eigenvalues cluster and CG ends by tolerance after 41 band solves.)"""
    rng = np.random.default_rng(3)
    infos = [np.diag(STRONG_RATIO * np.diag(pgm.diag_info(*pgm.SIGMA_ODO)).astype(np.float64) * 10 ** rng.uniform(-1, 1, 6)).astype(np.float32) for _ in STRONG_PAIRS]
    return dict(pgm.make_loop(33, list(STRONG_PAIRS), seed=11, closure_info=infos), fixed=None)


def seam_graph():
    """A half loop: 64 poses, closures between nodes half a turn apart, so that their relative yaw is within 1e-3 of +-pi.  Where the measured yaw and the yaw
    the start poses predict are on the same side of the seam, the measurement is moved 1e-4 rad across it."""
    g = dict(pgm.make_loop(64, list(SEAM_PAIRS), seed=11), fixed=None)
    T = np.asarray(g["poses"], np.float64)
    closures = []
    for (i, j, X, info) in g["closures"]:
        X = np.array(X, np.float32)
        pred = pgm.xof(T[i], T[j])[5]
        if (pred > 0) == (X[5] > 0):
            X[5] = np.float32(-np.sign(pred) * (np.pi - 1e-4))
        closures.append((i, j, X, info))
    return dict(g, closures=closures)


@functools.lru_cache(maxsize=None)
def step_graphs():
    """name -> (graph, options): the graphs one Gauss-Newton step is taken apart on, noisy, seed 11."""
    out = {}
    out["n2"] = (graph(2, CASES[1][1], None, True), {})
    out["n3"] = (graph(3, CASES[2][1], None, True), {})
    # CASES[3] (duplicates, a reversed closure, node 4 fixed) and: reversed neighbour closures with a fixed end (4, 3) and between free nodes (3, 2); an
    # off-band closure whose far end j is the fixed node
    out["n6"] = (graph(6, CASES[3][1] + ((4, 3), (3, 2), (2, 4)), 4, True), {})
    for k in (4, 5, 6):
        out["n%d" % CASES[k][0]] = (graph(CASES[k][0], CASES[k][1], None, True), {})
    # C x 36 = 288 entries of A: two grid blocks
    out["c8"] = (graph(40, ((0, 39), (2, 30), (35, 4), (10, 20), (21, 11), (7, 8), (9, 8), (15, 38)), None, True), {})
    out["seam"] = (seam_graph(), {})
    out["strong"] = (strong_graph(), {})
    out["strong100"] = (out["strong"][0], dict(max_pcg=100))
    out["damped"] = (out["n33"][0], dict(damping=1e-3))
    return out
