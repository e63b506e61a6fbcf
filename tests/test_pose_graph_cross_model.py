"""CPU tests of the NumPy model of the pose graph's COVARIANCE COLUMNS and GATE (-m "not gpu"; tests/pose_graph_cross_model.py): the formula
block (k, t) = [M^-1](k, t) - P_k P_t^T + Q_k Q_t^T against the dense inverse on the test graphs, the anchor property of the residual covariance, and the
corruptions that the checks must catch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cross_model as pxm      # noqa: E402
import pose_graph_direct_model as pdm      # noqa: E402
import pose_graph_marginals_model as pmm      # noqa: E402
import pose_graph_model as pgm      # noqa: E402

NAMES = ["n1", "n2", "n3", "n6", "n33", "n65", "chain65", "m0", "rank5", "strong", "ends288", "ends128"]


def _model_blocks(g):
    """(D, B, A, edges, is_fixed, H) of the model at the graph's poses."""
    n = g["poses"].shape[0]
    closures = list(g["closures"])
    edges = pgm.edge_list(n, closures)
    X, info = pgm._measurements(n, g["odo_X"], g["odo_info"], closures)
    is_fixed = pgm.fixed_mask(n, g["fixed"])
    T = np.asarray(g["poses"], np.float32).reshape(n, 4, 4).astype(np.float64)
    Js, _, H, _ = pgm.linearise(T, edges, X, info, is_fixed)
    D, B, A = pdm.blocks_of(H, Js, info, edges, is_fixed)
    return D, B, A, edges, is_fixed, H


@pytest.mark.parametrize("name", NAMES)
def test_the_formula_against_the_dense_inverse(name):
    """Every block of the restated formula against numpy.linalg.inv of the dense H, within MARGIN x the distance between the two NumPy references."""
    g = pxm.graphs()[name]
    D, B, A, edges, is_fixed, H = _model_blocks(g)
    t = pxm.TARGETS[name]
    cols = pxm.restate(D, B, A, edges, is_fixed, t)
    o, F = pxm.own_x(H, t, is_fixed)
    d = pxm.scaled_x(cols, F, t, is_fixed)
    print("%s: the formula is %.3e from inv(H), the two references %.3e apart" % (name, d, o))
    assert pxm.MARGIN * o <= pxm.CAP and d <= pxm.MARGIN * o
    # fixed rows and targets are zero
    for ti, tt in enumerate(t):
        assert not (cols[ti] if is_fixed[tt] else cols[ti][is_fixed]).any()


def test_the_anchor_property():
    """On chain65, S of candidate (20, 50) in the full chain equals S of candidate (0, 30) in the sub-chain 20 .. 50 -- only with the cross block."""
    g, c, sub, cs = pxm.anchor_graphs()
    Ff = pxm.embed(np.linalg.inv(pmm.model_H(g)), pgm.fixed_mask(65, None))
    Fs = pxm.embed(np.linalg.inv(pmm.model_H(sub)), pgm.fixed_mask(31, None))
    _, Sf = pxm.gate_model(g, c, Ff)
    _, Ss = pxm.gate_model(sub, cs, Fs)
    bound = pxm.anchor_bound()
    d = pxm.scaled_s(Sf, Ss)
    _, Sn = pxm.gate_model(g, c, Ff, cross=False)
    dn = pxm.scaled_s(Sn, Ss)
    print("anchor: with the cross block %.3e (bound %.3e), without it %.3e" % (d, bound, dn))
    assert d <= bound
    assert dn > 0.1          # the cross term left out of S: caught


def test_the_checks_bite():
    """Each corruption of the formula fails the check against the dense inverse, which the formula itself passes."""
    name = "n33"
    g = pxm.graphs()[name]
    D, B, A, edges, is_fixed, H = _model_blocks(g)
    t = pxm.TARGETS[name]
    o, F = pxm.own_x(H, t, is_fixed)
    bound = pxm.MARGIN * o

    def dist(**kw):
        return pxm.scaled_x(pxm.restate(D, B, A, edges, is_fixed, t, **kw), F, t, is_fixed)
    assert dist() <= bound
    for kw in (dict(drop_qq=True), dict(transpose_block=True), dict(swap_kt=True), dict(skip_end=1)):
        d = dist(**kw)
        print("corruption %s: %.3e (bound %.3e)" % (kw, d, bound))
        assert d > bound
    # the cross term left out of S: the gate's check against the model fails
    cands = pxm.candidates(name)
    d2, S = pxm.gate_model(g, cands, F)
    d2n, Sn = pxm.gate_model(g, cands, F, cross=False)
    ok = dict(d2=d2, res_cov=S, cand_status=np.zeros(len(cands), np.int32), rejected=int((~(d2 < pxm.DEFAULT_THRESHOLD)).sum()))
    pxm.check_gate(name, ok, cands)
    with pytest.raises(AssertionError):
        pxm.check_gate(name, dict(ok, d2=d2n, res_cov=Sn, rejected=int((~(d2n < pxm.DEFAULT_THRESHOLD)).sum())), cands)


@pytest.mark.parametrize("name", pxm.GATE_GRAPHS)
def test_the_candidates_are_what_they_are_named_for(name):
    """A true revisit passes the gate, the same moved by 1 m does not; the smallest eigenvalue of S is at least 3e-7 wherever the graph enters it."""
    g = pxm.graphs()[name]
    cands = pxm.candidates(name)
    edges = set(map(tuple, pgm.edge_list(g["poses"].shape[0], g["closures"])))
    assert all((c[0], c[1]) not in edges and (c[1], c[0]) not in edges for c in cands)
    assert len(pxm.gate_targets(cands)) <= pxm.MAX_TARGETS
    is_fixed = pgm.fixed_mask(g["poses"].shape[0], g["fixed"])
    F = pxm.embed(np.linalg.inv(pmm.model_H(g)), is_fixed)
    d2, S = pxm.gate_model(g, cands, F)
    print(name, d2)
    assert d2[0] < pxm.DEFAULT_THRESHOLD and d2[1] < pxm.DEFAULT_THRESHOLD and d2[2] > pxm.DEFAULT_THRESHOLD
    live = np.isfinite(d2)
    graph_enters = np.array([not (is_fixed[c[0]] and is_fixed[c[1]]) for c in cands])          # (both ends fixed: S is the measurement's covariance alone)
    assert min(np.linalg.eigvalsh(s)[0] for s in S[live & graph_enters]) >= 3e-7
    assert (~live).sum() == (1 if name == "n6" else 0)
