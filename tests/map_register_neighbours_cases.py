"""Inputs shared by the tests of the neighbourhood rule of the registration against a shaped voxel map, on top of map_register_cases: the
tie, the rows at the edge of the grid, the seam, the doubled starts of the convergence scene, and the model's own results on it -- each built once per session."""
import functools

import numpy as np

import map_model as mm
import map_register_cases as cs
import map_register_model as rm
import map_register_neighbours_model as nm
import map_shape_model as sm

EDGE = (1 << 20) - 1                                                  # the last cell index on every axis, either sign
TIE_SIGMA = 0.0625                                                    # a power of two: W = I / sigma^2 = 256 I exactly
TIE_PARAMS = dict(sigma_min=TIE_SIGMA, min_points=1)


def tie_case():
    """(map scans, rows, want) at cell 0.5 and the identity pose, every cell of ONE row (W = 256 I, mu the row itself: all exact).  Three clusters:
    - a row at the centre of an empty cell whose six face neighbours hold a point each, all 0.5 m from it: six equal s = 64; the earliest place wins: -x, which is
      place 1 of N7 and place 5 of N27;
    - the same without the two x neighbours: -y wins, place 3 of N7 and place 11 of N27;
    - a row ON the face between two cells of one point each, 0.25 m from both: its own cell (place 0) wins the tie.
    want: per row the place under (7, 27)."""
    c = 0.5
    pts, rows, want = [], [], []
    b = np.array([10.0, 10.0, 10.0]) * c + 0.25                       # the centre of cell (10, 10, 10)
    for a in range(3):
        for sgn in (-1.0, 1.0):
            e = np.zeros(3); e[a] = sgn * 0.5
            pts.append(b + e)
    rows.append(b); want.append((1, 5))
    b = np.array([20.0, 10.0, 10.0]) * c + 0.25
    for a in (1, 2):
        for sgn in (-1.0, 1.0):
            e = np.zeros(3); e[a] = sgn * 0.5
            pts.append(b + e)
    rows.append(b); want.append((3, 11))
    b = np.array([30.0, 10.0, 10.0]) * c
    pts += [b + [-0.25, 0.25, 0.25], b + [0.25, 0.25, 0.25]]
    rows.append(b + [0.0, 0.25, 0.25]); want.append((0, 0))
    return [np.array(pts, np.float32)], np.array(rows, np.float32), want


def edge_case(cell):
    """(map scans, rows) at the identity pose: per axis and sign a row in the LAST cell of the grid (index +-(2^20 - 1); its outer neighbour does not exist) and six
    points in the cell next to it on the inside, so that the row's own cell is empty and its only candidate is the inner neighbour; and one row beyond the grid."""
    c = float(np.float32(cell))
    pts, rows = [], []
    for a in range(3):
        for sgn in (-1, 1):
            w = np.full(3, 0.5 * c); w[a] = (sgn * EDGE + 0.5) * c
            rows.append(w)
            for k in range(6):
                p = np.full(3, (0.3 + 0.08 * k) * c); p[a] = (sgn * (EDGE - 1) + 0.5 + 0.05 * (k - 2.5)) * c
                pts.append(p)
    rows.append(np.array([0.5 * c, (EDGE + 1.5) * c, 0.5 * c]))
    rows = np.array(rows, np.float32)
    idx = np.floor(rows[:-1].astype(np.float64) / c)
    assert all(idx[2 * a + s, a] == (2 * s - 1) * EDGE for a in range(3) for s in range(2)), idx      # (float32 keeps the rows in the cells meant)
    return [np.array(pts, np.float32)], rows


def model_map(cell):
    """map_register_cases.model_map with the edge case's points."""
    m = cs.model_map(cell)
    m.add(edge_case(cell)[0], [mm.pose()])
    return m


def tie_map():
    return sm.ShapeMap(0.5).add(tie_case()[0], [mm.pose()])


SEAM_CELLS = ((0, 0, 0), (1, 0, 0))                                   # two usable cells of model_map(0.5) that share the face x = 0.5


def seam_rows():
    """Two rows a float32 step either side of the face x = 0.5 between SEAM_CELLS, at the centre of the face, at the identity pose."""
    x = np.float32(0.5)
    return np.array([[np.nextafter(x, np.float32(-1)), 0.25, 0.25], [np.nextafter(x, np.float32(2)), 0.25, 0.25]], np.float32)


DOUBLED = ((0.4, 0.2, 0.04), (-0.4, 0.3, -0.06), (0.2, -0.4, 0.06))


@functools.lru_cache(maxsize=None)
def doubled_starts():
    """The starts of scene() with the offsets doubled: [(held index, start pose)], z = 0.03."""
    s = cs.scene()
    starts = []
    for i, (_, T) in enumerate(s["held"]):
        yaw = float(np.arctan2(T[1, 0], T[0, 0]))
        for dx, dy, dyaw in DOUBLED:
            starts.append((i, mm.pose(t=(T[0, 3] + dx, T[1, 3] + dy, 0.03), r=(0, 0, yaw + dyaw))))
    return starts


@functools.lru_cache(maxsize=None)
def scene_model(neighbours, order="forward", doubled=False):
    """The model's record per start of scene() (or of doubled_starts()) under the neighbourhood, its rows summed in ``order``."""
    s = cs.scene()
    starts = doubled_starts() if doubled else s["starts"]
    if neighbours == 1 and not doubled:
        return cs.scene_model(order)
    return [nm.register(s["held"][i][0], T0, s["G"], neighbours, order=order, **s["params"]) for i, T0 in starts]


def truth_error(rec, k, doubled=False):
    """The distance of a record's translation from the true pose of start k's scan, metres."""
    s = cs.scene()
    starts = doubled_starts() if doubled else s["starts"]
    Tt = np.asarray(s["held"][starts[k][0]][1], np.float64)
    return float(np.linalg.norm(rec["pose64"][1] - Tt[:3, 3]))
