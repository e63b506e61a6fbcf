"""An independent NumPy model of the pose-graph optimiser's robust kernels (include/icet_hip.h "ROBUST KERNELS"): iteratively reweighted
least squares over the model of tests/pose_graph_model.py.  Double arithmetic, a dense numpy.linalg.solve per iteration, the device's accept rule with the
objective F = sum rho(chi2) in the place of the sum of chi2.  rho and weight restate the expressions of icet_amd/csrc/icet_posegraph.h in their order of
operations; nothing else is shared with the device code."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_model as pgm      # noqa: E402

NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3
KINDS = {"none": NONE, "huber": HUBER, "cauchy": CAUCHY, "geman_mcclure": GEMAN_MCCLURE}
ROBUST_ODOMETRY = 1
DEFAULT_SCALE = 16.8119      # the 99 % quantile of chi2 with six degrees of freedom


def rho(kind, c, s):
    s = float(s)
    if not (s > 0.0):
        return s
    if kind == HUBER:
        return s if s <= c else 2.0 * math.sqrt(c * s) - c
    if kind == CAUCHY:
        return c * math.log1p(s / c)
    if kind == GEMAN_MCCLURE:
        return c * s / (c + s)
    return s


def weight(kind, c, s):
    s = float(s)
    if not (s > 0.0):
        return 1.0
    if kind == HUBER:
        return 1.0 if s <= c else math.sqrt(c / s)
    if kind == CAUCHY:
        return 1.0 / (1.0 + s / c)
    if kind == GEMAN_MCCLURE:
        t = c / (c + s)
        return t * t
    return 1.0


def edge_kinds(n, n_edges, kind, flags):
    """The kind every edge takes: the closures always, the odometry edges only under ROBUST_ODOMETRY."""
    return [kind if (e >= n - 1 or (flags & ROBUST_ODOMETRY)) else NONE for e in range(n_edges)]


def tree_sum(v):
    """The device's order of a sum: lane l of 256 adds the entries l, l + 256, ... ascending, then a binary tree over the lanes."""
    lane = [0.0] * 256
    for l in range(256):
        s = 0.0
        for i in range(l, len(v), 256):
            s += float(v[i])
        lane[l] = s
    h = 128
    while h > 0:
        for l in range(h):
            lane[l] += lane[l + h]
        h >>= 1
    return lane[0]


def optimise(poses, odo_X, odo_info, closures=(), fixed=None, gn_iters=10, dx_tol=1e-7, damping=0.0, kind=NONE, scale=DEFAULT_SCALE, flags=0):
    """pgm.optimise under a robust kernel.  dict of pgm.optimise's keys (chi2_initial, chi2_final: the RAW sums) and cost_initial, cost_final (F), edge_weight
    (E: w at the chi2 of the returned poses), downweighted, steps (max |dx| of every accepted step)."""
    P32 = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    n = P32.shape[0]
    closures = list(closures)
    edges = pgm.edge_list(n, closures)
    X, info = pgm._measurements(n, odo_X, odo_info, closures)
    kinds = edge_kinds(n, len(edges), kind, flags)
    is_fixed = pgm.fixed_mask(n, fixed)
    free = np.nonzero(~is_fixed)[0]
    col = -np.ones(n, int); col[free] = np.arange(free.size)

    def cost(chi):
        return tree_sum([rho(k, scale, s) for k, s in zip(kinds, chi)])

    def weights(chi):
        return np.array([weight(k, scale, s) for k, s in zip(kinds, chi)], np.float64).reshape(-1)

    T = P32.astype(np.float64)
    chi0 = pgm.edge_chi2(T, edges, X, info)
    chi_e, F = chi0.copy(), cost(chi0)
    F0 = F
    status, its, max_dx, failed, steps = pgm.ITERATION_CAP, 0, 0.0, False, []
    if not np.isfinite(F):
        status, failed = pgm.NON_FINITE, True
    for _ in range(gn_iters if not failed else 0):
        its += 1
        m = 6 * free.size
        w = weights(chi_e)
        _, _, H, g = pgm.linearise(T, edges, X, [wi * om for wi, om in zip(w, info)], is_fixed, damping)
        if m:
            if not (np.isfinite(H).all() and np.isfinite(g).all()):
                status, failed = pgm.NON_FINITE, True; break
            try:
                np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                status, failed = pgm.NOT_POSITIVE_DEFINITE, True; break
            dx = np.linalg.solve(H, -g)
        else:
            dx = np.zeros(0)
        max_dx = float(np.abs(dx).max()) if m else 0.0
        Tt = T.copy()
        for k in free:
            Tt[k] = T[k] @ pgm.exp_se3(dx[6 * col[k]:6 * col[k] + 6])
        chit = pgm.edge_chi2(Tt, edges, X, info)
        Ft = cost(chit)
        if not np.isfinite(Ft):
            status, failed = pgm.NON_FINITE, True; break
        if not (Ft < F):
            status = pgm.CONVERGED if max_dx < dx_tol else pgm.STALLED
            break
        T, chi_e, F = Tt, chit, Ft
        steps.append(max_dx)
        if max_dx < dx_tol:
            status = pgm.CONVERGED
            break
    out = T.astype(np.float32)
    out[:, 3, :] = (0, 0, 0, 1)
    if failed:
        out, chi_e, F, T = P32.copy(), chi0, F0, P32.astype(np.float64)
    out[is_fixed] = P32[is_fixed]
    wf = weights(chi_e)
    return dict(poses=out, poses64=T, chi2_initial=tree_sum(chi0), chi2_final=tree_sum(chi_e), cost_initial=F0, cost_final=F, status=status, gn_iterations=its,
                max_dx=max_dx, edge_chi2=np.stack([chi0, chi_e]), edge_weight=wf, downweighted=int((wf < 0.5).sum()), steps=steps)
