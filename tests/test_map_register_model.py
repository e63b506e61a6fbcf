"""CPU tests of the NumPy model of the registration against a shaped voxel map (tests/map_register_model.py): what the rule promises,
checked on the model alone -- the sums do not depend on the order of the rows, a miss costs the scale, a cell of one row weighs I / sigma_min^2, g and H are the
derivatives of F, a plane leaves the in-plane translations weakest, and the loop converges from every start of the convergence case."""
import math

import numpy as np
import pytest

import map_model as mm
import map_register_cases as cs
import map_register_model as rm
import map_shape_model as sm

U = 2.0 ** -53


@pytest.fixture(scope="module")
def slab():
    m = cs.model_map(0.5)
    return m, rm.Gaussians(m)


def test_sums_do_not_depend_on_the_order_of_the_rows(slab):
    """F, g and H of a permuted scan equal those of the scan up to the rounding of two sums of N terms: |a - b| <= 2 gamma_(N-1) sum |term|."""
    _, G = slab
    rows = cs.term_rows(0.5, 3000)
    R, t = rm.pose64(cs.POSE)
    tm = rm.row_terms(rows, R, t, G)
    a, ns, nm = rm.totals(tm, "forward")
    perm = np.random.RandomState(3).permutation(rows.shape[0])
    tp = rm.row_terms(rows[perm], R, t, G)
    for k in ("s", "omega", "rho", "v"):                              # a row's terms are its own: the same bits wherever it stands
        assert np.array_equal(tp[k].view(np.uint64), np.ascontiguousarray(tm[k][perm]).view(np.uint64))
    b, ns2, nm2 = rm.totals(tp, "forward")
    assert (ns, nm) == (ns2, nm2) and nm > 1500
    k = ns - 1
    bound = 2 * (k * U / (1 - k * U)) * np.abs(tm["v"]).sum(axis=0)
    bound[0] += 2 * (k * U / (1 - k * U)) * rm.DEFAULTS["scale"] * (ns - nm)
    assert (np.abs(a - b) <= bound).all() and (a != b).any()
    for order in ("reverse", "chunks", "exact"):
        assert (np.abs(rm.totals(tm, order)[0] - a) <= bound).all()


def test_a_miss_costs_the_scale(slab):
    _, G = slab
    R, t = rm.pose64(mm.pose())
    rows = np.array([[0.1, 0.2, 25.0], [0.3, 0.1, 22.6], [0.3, 0.1, -24.8], [0.3, 0.1, 27.6], [6e5, 0, 0], [np.nan, 0, 0], [0, 0, 0]], np.float32)
    for c in (11.3449, 3.0):
        tm = rm.row_terms(rows, R, t, G, c)
        assert list(tm["cls"]) == [mm.KEPT] * 4 + [mm.OUTSIDE, mm.NONFINITE, mm.RANGE] and not tm["matched"].any()
        assert (tm["rho"][:5] == c).all() and not tm["rho"][5:].any() and not tm["v"].any() and not tm["omega"].any()
        tot, ns, nm = rm.totals(tm, "forward")
        assert (ns, nm) == (5, 0) and tot[0] == c * 5 and not tot[1:].any()
        assert rm.totals(tm, "exact")[0][0] == math.fsum([c] * 5)
    # rho tends to the scale from below as s grows: a match never costs more than a miss
    tm = rm.row_terms(cs.term_rows(0.5, 3000), *rm.pose64(cs.POSE), G)
    assert (tm["rho"][tm["matched"]] < rm.DEFAULTS["scale"]).all() and (tm["rho"][tm["matched"]] >= 0).all()


def test_a_cell_of_one_row_weighs_the_identity_over_sigma_squared():
    for cell in (0.1, 0.5):
        p = np.array([[3.3 * cell, -2.2 * cell, 1.1 * cell]], np.float32)
        m = sm.ShapeMap(cell).add([p], [mm.pose()])
        (key, e), = m.cells.items()
        for sigma in (0.02, 0.1, 1e-3):
            mu, W = rm.gauss(key, e[0], e[1:4], m.words(key), cell, sigma, 1)
            assert W[1] == 0 and W[2] == 0 and W[4] == 0
            assert all(abs(W[j] * sigma * sigma - 1.0) <= 8 * U for j in (0, 3, 5))
            assert np.abs(np.array(mu) - p[0].astype(np.float64)).max() <= cell * 2.0 ** -31      # the offsets' resolution
            assert rm.gauss(key, e[0], e[1:4], m.words(key), cell, sigma, 2) is None


def _interior(rows, R, t, G, margin):
    """The rows whose world point lies at least ``margin`` inside its cell on every axis: a step below the margin moves none of them into another cell."""
    w = np.asarray(rows, np.float64) @ np.asarray(R).T + t
    f = w / G.cell - np.floor(w / G.cell)
    return rows[((f > margin / G.cell) & (f < 1 - margin / G.cell)).all(axis=1)]


def test_g_and_h_are_the_derivatives_of_f(slab):
    """F(delta) at the pose retracted by delta, by central differences of step h in each of the six directions, on rows that stay in their cells:
    dF / d delta = 2 g, with |error| <= h^2 / 6 max |F'''| + u sum |rho| / h: the third derivative is bounded through a finer difference of the gradients
    (measured on the model: it is the model's own smoothness, not the code's), the second term is the rounding of the two sums.  And with a scale so large
    that omega = 1 to 1e-9, d g / d rho_t = the first three columns of H: exactly (F is then quadratic in the translation), up to the rounding of the sums."""
    _, G = slab
    R, t = rm.pose64(cs.POSE)
    rows = _interior(cs.term_rows(0.5, 1500)[10:], R, t, G, 2e-3)
    assert rows.shape[0] > 1200
    h = 1e-4

    def at(delta, scale):
        Q = rm.retract(R, t, delta)
        return rm.totals(rm.row_terms(rows, Q[0], Q[1], G, scale), "exact")

    tot, ns, nm = at([0.0] * 6, rm.DEFAULTS["scale"])
    tm = rm.row_terms(rows, R, t, G)
    round_f = 4 * U * float(np.abs(tm["rho"]).sum()) * ns / h
    for j in range(6):
        e = np.zeros(6); e[j] = 1.0
        fp, fm = at(e * h, rm.DEFAULTS["scale"]), at(-e * h, rm.DEFAULTS["scale"])
        assert fp[1:] == (ns, nm) and fm[1:] == (ns, nm)              # no row changed its cell
        d1 = (fp[0][0] - fm[0][0]) / (2 * h)
        # F''' along e_j from the gradients at +-h and 0: (g(+h) - 2 g(0) + g(-h)) / h^2 x 2
        f3 = abs(2 * (fp[0][1 + j] - 2 * tot[1 + j] + fm[0][1 + j]) / (h * h))
        tol = h * h / 6 * max(f3, 1.0) * 2 + round_f
        assert abs(d1 - 2 * tot[1 + j]) <= tol, (j, d1, 2 * tot[1 + j], tol)
        assert abs(d1 - 2 * tot[1 + j]) <= 1e-5 * max(abs(d1), 1.0)   # (and the tolerance is no loophole: it is far below the gradient itself)
    big = 1e12
    tot, ns, nm = at([0.0] * 6, big)
    H = rm.info_matrix(tot[7:])
    tb = rm.row_terms(rows, R, t, G, big)
    for j in range(3):
        e = np.zeros(6); e[j] = 1.0
        gp, gm = at(e * h, big)[0][1:7], at(-e * h, big)[0][1:7]
        col = (gp - gm) / (2 * h)
        # omega differs from 1 by 2 s / scale at most, and so does each row's share of the column
        tol = np.abs(tb["v"][:, 1:7]).sum(axis=0) * 8 * U / h + (2 * float(tb["s"].max()) / big) * np.abs(H[:, j]) * 4 + 1e-9 * np.abs(H[:, j])
        assert (np.abs(col - H[:, j]) <= tol).all(), (j, col, H[:, j], tol)
    assert np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() > 0


def test_on_a_noisy_plane_the_in_plane_translations_are_weakest():
    """A map of one noisy plane (map_shape_model.plane_rows): of the three translations, the two in the plane are constrained by the cells' own extent alone, the
    one along the normal by the noise; the translation block of H has one large eigenvalue, its eigenvector the plane's normal, and two small ones.  A cell's
    in-plane variance is about cell^2 / 12 = 0.021 m^2 and its variance along the normal 0.02^2 + sigma_min^2 = 0.0008 m^2: a ratio of 26 for whole cells, less
    for the cells the slanted plane cuts at a corner -- 18 here; the test asks for 10."""
    rows = sm.plane_rows(20000)
    m = sm.ShapeMap(0.5).add([rows], [mm.pose()])
    G = rm.Gaussians(m)
    sub = rows[::7]
    tot, ns, nm = rm.totals(rm.row_terms(sub, *rm.pose64(mm.pose()), G), "forward")
    assert nm > 0.9 * ns
    H = rm.info_matrix(tot[7:])
    ev, V = np.linalg.eigh(H[:3, :3])
    assert ev[0] > 0 and ev[2] > 10 * ev[1]
    assert abs(float(V[:, 2] @ sm.PLANE_NORMAL)) > 0.999
    assert abs(float(V[:, 0] @ sm.PLANE_NORMAL)) < 0.05 and abs(float(V[:, 1] @ sm.PLANE_NORMAL)) < 0.05


def test_the_model_converges_from_every_start_of_the_convergence_case():
    s = cs.scene()
    fwd, rev = cs.scene_model("forward"), cs.scene_model("reverse")
    assert len(fwd) == len(s["starts"]) == 6
    worst = 0.0
    for k, (a, b) in enumerate(zip(fwd, rev)):
        Tt = np.asarray(s["held"][s["starts"][k][0]][1], np.float64)
        T0 = np.asarray(s["starts"][k][1], np.float64)
        assert a["status"] == rm.CONVERGED and b["status"] == rm.CONVERGED, (k, a["status"], b["status"])
        assert a["iterations"] <= s["params"]["max_iters"] and a["accepted"] >= 5 and a["cost"] < 0.7 * a["cost_start"]
        err0 = np.linalg.norm(T0[:3, 3] - Tt[:3, 3]); err = np.linalg.norm(a["pose64"][1] - Tt[:3, 3])
        assert err0 > 0.2 and err < 0.01, (k, err0, err)              # from 0.2 m and more to under a centimetre (the cells are 0.5 m)
        assert np.abs(a["pose64"][0] - Tt[:3, :3]).max() < 1e-3
        worst = max(worst, cs.pose_diff(a["pose64"], b["pose64"]))
    assert 0.0 < worst < 1e-12                                        # the order of the sums moves the pose in its last bits only
    # max_iters = 0 scores the start pose, and a start at the result stays there
    sc = rm.register(s["held"][0][0], s["starts"][0][1], s["G"], max_iters=0)
    assert sc["status"] == rm.ITERATION_CAP and sc["iterations"] == 0 and sc["cost"] == fwd[0]["cost_start"]
    again = rm.register(s["held"][0][0], fwd[0]["pose"], s["G"], max_iters=30)
    assert np.linalg.norm(again["pose64"][1] - fwd[0]["pose64"][1]) < 1e-3
