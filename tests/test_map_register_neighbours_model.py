"""CPU tests of the neighbourhood rule of the registration against a shaped voxel map on its NumPy model alone (tests/map_register_neighbours_model.py; DESIGN.md
section 26): a wider neighbourhood never costs a row more and never loses a match, the cost does not jump where a row crosses a face between two usable cells,
ties go to the earlier cell, cells outside the grid and unusable cells are passed over, g is still the gradient of F, and the loop takes fewer passes and reaches
further than the centre-only rule on the project's own convergence case."""
import numpy as np
import pytest

import map_model as mm
import map_register_cases as cs
import map_register_model as rm
import map_register_neighbours_cases as nc
import map_register_neighbours_model as nm

U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_orders_of_the_neighbourhoods():
    assert nm.N7 == [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    assert len(nm.N27) == 27 == len(set(nm.N27)) and nm.N27[0] == (0, 0, 0) and nm.N27[1] == (-1, -1, -1) and nm.N27[2] == (-1, -1, 0) and nm.N27[26] == (1, 1, 1)
    assert nm.N27[13] == (0, 0, -1) and nm.N27[14] == (0, 0, 1) and nm.N27[1:] == sorted(nm.N27[1:])      # dx slowest, the centre taken out
    assert nm.FLAGS == {1: 0, 7: 2, 27: 4}


@pytest.mark.parametrize("where", ["start", "truth"])
def test_a_wider_neighbourhood_costs_no_row_more(where):
    """On scene() at a start pose and at the true pose: rho(N27) <= rho(N7) <= rho(N1) for every scored row, the matched sets are nested, N1 under this model is
    map_register_model's own terms, and a row whose winner is its own cell has the centre-only terms bit for bit."""
    s = cs.scene()
    i, T0 = s["starts"][1]
    scan = s["held"][i][0]
    R, t = rm.pose64(T0 if where == "start" else np.asarray(s["held"][i][1], np.float32))
    base = rm.row_terms(scan, R, t, s["G"])
    tm = {nb: nm.row_terms(scan, R, t, s["G"], nb) for nb in (1, 7, 27)}
    for k in ("s", "omega", "rho", "v"):
        assert np.array_equal(_bits(tm[1][k]), _bits(base[k])), k
    assert np.array_equal(tm[1]["matched"], base["matched"]) and np.array_equal(tm[1]["place"], np.where(base["matched"], 0, -1))
    sc = base["scored"]
    assert sc.sum() > 7000
    for nb in (7, 27):
        assert np.array_equal(tm[nb]["scored"], sc) and np.array_equal(tm[nb]["key"], base["key"]) and np.array_equal(tm[nb]["cls"], base["cls"])
    assert (tm[27]["rho"][sc] <= tm[7]["rho"][sc]).all() and (tm[7]["rho"][sc] <= tm[1]["rho"][sc]).all()
    assert (tm[27]["rho"][sc] < tm[1]["rho"][sc]).sum() > 100
    assert not (tm[1]["matched"] & ~tm[7]["matched"]).any() and not (tm[7]["matched"] & ~tm[27]["matched"]).any()
    assert tm[27]["matched"].sum() > tm[7]["matched"].sum() > tm[1]["matched"].sum()
    for nb in (7, 27):
        own = tm[nb]["place"] == 0
        assert own.sum() > 1000 and tm[1]["matched"][own].all()
        for k in ("s", "omega", "rho", "v"):
            assert np.array_equal(_bits(tm[nb][k][own]), _bits(tm[1][k][own])), (nb, k)
        assert (tm[nb]["rho"][sc] <= rm.DEFAULTS["scale"]).all() and (tm[nb]["rho"][sc & ~tm[nb]["matched"]] == rm.DEFAULTS["scale"]).all()


def test_the_cost_does_not_jump_at_a_face_between_two_usable_cells():
    """Two rows a float32 step either side of the face x = 0.5 between two usable cells of model_map(0.5): centre only, their costs differ by more than 1; under
    either neighbourhood the row beyond the face still finds the nearer cell, and they differ by less than 1e-4."""
    G = rm.Gaussians(cs.model_map(0.5))
    rows = nc.seam_rows()
    I = rm.pose64(mm.pose())
    tm = {nb: nm.row_terms(rows, *I, G, nb) for nb in (1, 7, 27)}
    cells = [tuple(int(v) for v in mm.key_cells(k)) for k in tm[1]["key"]]
    assert cells == list(nc.SEAM_CELLS) and tm[1]["matched"].all() and rows[1, 0] - rows[0, 0] < 1e-7
    print("centre only %.8f %.8f; 7 cells %.8f %.8f; 27 cells %.8f %.8f" % (tuple(tm[1]["rho"]) + tuple(tm[7]["rho"]) + tuple(tm[27]["rho"])))
    assert abs(tm[1]["rho"][0] - tm[1]["rho"][1]) > 1.0
    for nb in (7, 27):
        assert abs(tm[nb]["rho"][0] - tm[nb]["rho"][1]) < 1e-4
        assert tm[nb]["rho"][0] == tm[1]["rho"][0] and tm[nb]["place"][0] == 0 and tm[nb]["place"][1] == (1 if nb == 7 else 5)      # the cell across the face: -x


def test_a_tie_goes_to_the_earlier_cell():
    G = rm.Gaussians(nc.tie_map(), **nc.TIE_PARAMS)
    assert (G.W[:, [0, 3, 5]] == 256.0).all() and not G.W[:, [1, 2, 4]].any()
    _, rows, want = nc.tie_case()
    I = rm.pose64(mm.pose())
    for col, nb in enumerate((7, 27)):
        tm = nm.row_terms(rows, *I, G, nb)
        c = tm["cand"]
        assert (np.nan_to_num(c[0], nan=64.0) == 64.0).all() and np.isfinite(c[0]).sum() == 6 and np.isfinite(c[1]).sum() == 4      # six, then four, equal candidates
        assert c[2][0] == 16.0 and c[2][1 if nb == 7 else 5] == 16.0                                                                 # own against -x, equal
        assert list(tm["place"]) == [w[col] for w in want] and list(tm["s"]) == [64.0, 64.0, 16.0]
    tm = nm.row_terms(rows, *I, G, 1)
    assert list(tm["place"]) == [-1, -1, 0]


def test_a_nan_or_infinite_s_never_wins():
    """Gaussians by hand: the own cell's W is NaN, the -x cell's is infinite (s = +infinity), the +x cell's is finite and large: +x wins; without it the row is a
    miss; and a NaN own cell does not hide a finite neighbour that comes later."""
    class Hand:
        cell = 0.5
        find = rm.Gaussians.find
    key = lambda c: int(mm.classify(np.array([[(c[0] + .5) * .5, (c[1] + .5) * .5, (c[2] + .5) * .5]], np.float32), mm.pose(), 0.5)[1][0])
    G = Hand()
    ks = [key((4, 4, 4)), key((3, 4, 4)), key((5, 4, 4))]
    order = np.argsort(ks)
    W = np.array([[np.nan, 0, 0, 1, 0, 1], [np.inf, 0, 0, np.inf, 0, np.inf], [1e6, 0, 0, 1e6, 0, 1e6]])
    G.key = np.array(ks, np.uint64)[order]; G.mu = np.array([[2.2, 2.2, 2.2], [1.7, 2.2, 2.2], [2.7, 2.2, 2.2]])[order]; G.W = W[order]
    row = np.array([[2.25, 2.25, 2.25]], np.float32)
    I = rm.pose64(mm.pose())
    for nb, plus_x in ((7, 2), (27, 22)):
        tm = nm.row_terms(row, *I, G, nb)
        assert np.isnan(tm["cand"][0][0]) or tm["cand"][0][0] != tm["cand"][0][0]
        assert tm["place"][0] == plus_x and np.isfinite(tm["s"][0]) and tm["s"][0] > 1e5
    G2 = Hand(); keep = np.array(ks, np.uint64)[order] != np.uint64(ks[2])
    G2.key, G2.mu, G2.W = G.key[keep], G.mu[keep], G.W[keep]
    for nb in (1, 7, 27):
        tm = nm.row_terms(row, *I, G2, nb)
        assert tm["place"][0] == -1 and not tm["matched"][0] and tm["rho"][0] == rm.DEFAULTS["scale"] and not tm["v"].any()


@pytest.mark.parametrize("cell", [0.1, 0.5])
def test_the_edge_of_the_grid_and_unusable_cells(cell):
    """A row in the last cell of the grid on each axis and side looks at the cells that exist and matches the inner neighbour; a row outside the grid is a miss; a
    row whose own cell is empty, below min_points, emptied or negative matches a usable neighbour where there is one."""
    G = rm.Gaussians(nc.model_map(cell))
    I = rm.pose64(mm.pose())
    _, rows = nc.edge_case(cell)
    for nb, want in ((1, [-1] * 7), (7, [2, 1, 4, 3, 6, 5, -1]), (27, [22, 5, 16, 11, 14, 13, -1])):
        tm = nm.row_terms(rows, *I, G, nb)
        assert list(tm["place"]) == want and list(tm["cls"]) == [mm.KEPT] * 6 + [mm.OUTSIDE]
        assert tm["rho"][6] == rm.DEFAULTS["scale"] and tm["scored"].all()
        for a in range(3):
            c = np.array(mm.key_cells(tm["key"][2 * a + 1]))
            assert c[a] == nc.EDGE and np.array(mm.key_cells(tm["key"][2 * a]))[a] == -nc.EDGE
    # the special cells of the slab map lie far above and below it: each is alone.  A usable cell next to each of them, in a copy of the map:
    add, rem, pts = cs.special_cells(cell)
    m = cs.model_map(cell)
    c = float(np.float32(cell))
    near = [np.array([[p[0] + c + 0.02 * c * k, p[1] + 0.03 * c * k, p[2]] for k in range(6)], np.float32) for p in pts]      # six rows one cell over in +x
    empty = np.array([[0.3 * c, 0.4 * c, 65.25 * c]], np.float32)
    near.append(np.array([[empty[0, 0] + c + 0.02 * c * k, empty[0, 1] + 0.03 * c * k, empty[0, 2]] for k in range(6)], np.float32))
    rows = np.concatenate([pts, empty]).astype(np.float32)
    alone = nm.row_terms(rows, *I, rm.Gaussians(m), 27)
    assert list(alone["place"]) == [-1] * 4
    m.add(near, [mm.pose()] * len(near))
    G = rm.Gaussians(m)
    assert list(nm.row_terms(rows, *I, G, 1)["place"]) == [-1] * 4
    for nb, plus_x in ((7, 2), (27, 22)):
        tm = nm.row_terms(rows, *I, G, nb)
        assert list(tm["place"]) == [plus_x] * 4 and tm["matched"].all() and (tm["rho"] < rm.DEFAULTS["scale"]).all()


@pytest.mark.parametrize("neighbours", [7, 27])
def test_g_is_the_gradient_of_f(neighbours):
    """dF / d delta = 2 g by central differences of step h, on the rows that keep their WINNER over the step (F is piecewise smooth: where the winner changes it has
    a kink).  The tolerance is test_map_register_model.py's: h^2 / 6 max |F'''| from a finer difference of the gradients, plus the rounding of the two sums."""
    G = rm.Gaussians(cs.model_map(0.5))
    R, t = rm.pose64(cs.POSE)
    rows = cs.term_rows(0.5, 1500)[10:]
    h = 1e-4
    key_of = lambda tm: (tm["key"].copy(), tm["place"].copy())
    at_all = lambda d: nm.row_terms(rows, *rm.retract(R, t, d), G, neighbours)
    k0 = key_of(at_all([0.0] * 6))
    keep = np.ones(rows.shape[0], bool)
    for j in range(6):
        for sg in (-1.0, 1.0):
            e = np.zeros(6); e[j] = sg * h
            k1 = key_of(at_all(e))
            keep &= (k1[0] == k0[0]) & (k1[1] == k0[1])
    rows = rows[keep]
    assert rows.shape[0] > 1100                                       # nearly all of them
    at = lambda d: rm.totals(nm.row_terms(rows, *rm.retract(R, t, d), G, neighbours), "exact")
    tot, ns, nmatch = at([0.0] * 6)
    tm = nm.row_terms(rows, R, t, G, neighbours)
    assert (tm["place"] > 0).sum() > 50                               # rows scored against a neighbour among them
    round_f = 4 * U * float(np.abs(tm["rho"]).sum()) * ns / h
    for j in range(6):
        e = np.zeros(6); e[j] = 1.0
        fp, fm = at(e * h), at(-e * h)
        assert fp[1:] == (ns, nmatch) and fm[1:] == (ns, nmatch)
        d1 = (fp[0][0] - fm[0][0]) / (2 * h)
        f3 = abs(2 * (fp[0][1 + j] - 2 * tot[1 + j] + fm[0][1 + j]) / (h * h))
        tol = h * h / 6 * max(f3, 1.0) * 2 + round_f
        assert abs(d1 - 2 * tot[1 + j]) <= tol, (j, d1, 2 * tot[1 + j], tol)
        assert tol <= 1e-4 * 2 * float(np.abs(tot[1:7]).max())          # (and the tolerance is no loophole: four decades below the gradient it checks)


def test_27_cells_take_fewer_passes_and_end_no_further_from_the_truth():
    """scene(), held against the centre-only model's own results (map_register_cases.scene_model), not against fixed figures: with 27 cells all six starts are
    CONVERGED, each in no more passes than centre-only from the same start, each no further from the truth than centre-only's worst."""
    own, n27 = nc.scene_model(1), nc.scene_model(27)
    worst = max(nc.truth_error(r, k) for k, r in enumerate(own))
    for k, (a, b) in enumerate(zip(own, n27)):
        print("start %d: centre only %d passes (%d accepted) %.1f mm; 27 cells %d passes (%d accepted) %.1f mm" %
              (k, a["iterations"], a["accepted"], 1e3 * nc.truth_error(a, k), b["iterations"], b["accepted"], 1e3 * nc.truth_error(b, k)))
        assert a["status"] == rm.CONVERGED and b["status"] == rm.CONVERGED
        assert b["iterations"] <= a["iterations"]
        assert nc.truth_error(b, k) <= worst


def test_both_neighbourhoods_reach_twice_as_far():
    """The six starts with their offsets doubled (0.45 m, 0.06 rad): 7 and 27 cells converge from all six to within centre-only's worst error from the ORDINARY
    starts; centre-only's fourth doubled start ends more than 0.1 m off."""
    worst = max(nc.truth_error(r, k) for k, r in enumerate(nc.scene_model(1)))
    own = nc.scene_model(1, doubled=True)
    for nb in (7, 27):
        recs = nc.scene_model(nb, doubled=True)
        for k, r in enumerate(recs):
            print("%d cells, doubled start %d: %s, %d passes (%d accepted), %.1f mm" % (nb, k, rm.STATUS_NAMES[r["status"]], r["iterations"], r["accepted"], 1e3 * nc.truth_error(r, k, True)))
            assert r["status"] == rm.CONVERGED and nc.truth_error(r, k, True) <= worst, (nb, k)
    print("centre only, doubled start 3: %s, %.1f mm" % (rm.STATUS_NAMES[own[3]["status"]], 1e3 * nc.truth_error(own[3], 3, True)))
    assert nc.truth_error(own[3], 3, True) > 0.1
