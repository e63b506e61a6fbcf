"""Inputs shared by the tests of a voxel map's visibility evidence: the direction table of the octahedral pixel, the tie table of the
thresholds, and the 8-pose drive of tests/test_map_query.py with a car that moves 2 m per scan."""
import numpy as np

import map_model as mm


def nf(v, up=True):
    """The float32 one ulp above (below) v."""
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)).astype(np.float32)


def direction_rows():
    """Rows (N x 3 float32) whose pixel is where the octahedral map can go wrong."""
    rows = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (-0.0, -0.0, -1), (0.0, -0.0, -2), (-0.0, 0.0, 3)]
    rows += [(1, 2, 0.0), (1, 2, -0.0), (-3, 1, 0.0), (-3, 1, -0.0), (2, -5, -0.0), (-1, -1, 0.0)]                     # z = +-0.0: the fold is not taken at -0.0
    rows += [(0.0, 1, -1), (-0.0, 1, -1), (1, 0.0, -1), (1, -0.0, -1), (0.0, -1, -1), (-1, -0.0, -3), (0.0, 2, -1), (-0.0, -2, -5)]      # px or py exactly 0 below the horizon
    rows += [(sx * 1.0, sy * 1.0, z) for sx in (1, -1) for sy in (1, -1) for z in (0.0, -0.0, -1e-3, 1e-3, -1.0, -2.0)]      # the four fold diagonals
    for k in range(17):                                               # exactly on the pixel borders of W = 16: px = k / 8 - 1, a = 1
        x = k / 8.0 - 1.0
        for y in (0.0, 0.125, -0.125):
            z = 1.0 - abs(x) - abs(y)
            if z >= 0:
                rows += [(x, y, z), (y, x, z), (x, y, -z), (y, x, -z)]
    base = [(1, 2, -1), (-3, 1, 2), (0.5, -0.25, -4), (1, 1, 1), (0, 0, -1), (-1, 0, 0)]
    rows += [tuple(np.float32(s) * np.float32(c) for c in b) for s in (1e-30, 3e38 / 4) for b in base]                  # magnitudes 1e-30 and up to 3e38
    rows += [(3e38, 3e38, 3e38), (3.4e38, 0, 0), (1e-30, 0, 0), (0, 0, -1e-30), (1e-38, 1e-38, -1e-38)]
    return np.array(rows, np.float32)


# +x, -x, +y, -y, +z, -z at W = 16 as (u, v), by hand: a = 1, (px, py) = (+-1, 0), (0, +-1), (0, 0), and -z folds (0, 0) to (1, 1)
AXIS_PIXELS_W16 = [(15, 8), (0, 8), (8, 15), (8, 0), (8, 8), (15, 15)]


def tie_cases():
    """The thresholds' tie table at cell 0.125: one point (5.0625, 0, 0) is the middle of cell 40 on x, so its centroid is the point and rc = 5.0625 exactly;
    a scan of the one row (rn, 0, 0) at the identity has the range word rn in the same pixel.  Each case: dict(scan_row, mn, mx, mg, want) with want one of
    'miss', 'agree', 'none' (occluded or no part: no evidence)."""
    rc, mg = np.float32(5.0625), np.float32(0.5)
    far, near = np.float32(5.5625), np.float32(4.5625)
    c = []
    base = dict(mn=np.float32(0.0), mx=np.float32(40.0), mg=mg)
    c.append(dict(base, scan_row=(far, 0, 0), want="agree"))                    # rn == rc + mg
    c.append(dict(base, scan_row=(nf(far), 0, 0), want="miss"))                 # one ulp above
    c.append(dict(base, scan_row=(near, 0, 0), want="agree"))                   # rn == rc - mg
    c.append(dict(base, scan_row=(nf(near, False), 0, 0), want="none"))         # one ulp below: occluded
    c.append(dict(base, scan_row=(rc, 0, 0), mg=np.float32(0.0), want="agree"))                 # margin 0: rn == rc
    c.append(dict(base, scan_row=(nf(rc), 0, 0), mg=np.float32(0.0), want="miss"))
    c.append(dict(base, scan_row=(nf(rc, False), 0, 0), mg=np.float32(0.0), want="none"))
    c.append(dict(base, scan_row=(np.float32(3e38), 3e38, 3e38), want="none"))                  # another pixel
    c.append(dict(base, scan_row=(np.float32(3.4e38), 0, 0), want="miss"))                      # a far return is evidence
    c.append(dict(base, scan_row=(np.float32(9.0), 0, 0), mx=rc, want="miss"))                  # d2 == max_range^2 takes part
    c.append(dict(base, scan_row=(np.float32(9.0), 0, 0), mx=nf(rc, False), want="none"))
    c.append(dict(base, scan_row=(np.float32(9.0), 0, 0), mn=rc, want="none"))                  # d2 == min_range^2 does not
    c.append(dict(base, scan_row=(np.float32(9.0), 0, 0), mn=nf(rc, False), want="miss"))
    return np.array([[rc, 0, 0]], np.float32), c


_CAR = {}


def car_boxes(scene, n=8):
    g = scene["ground"]
    return [(1.1 + 2 * k, 2.9 + 2 * k, 2.2, 3.8, g, g + 1.5) for k in range(n)]


def car_drive(rings, steps):
    """The drive of tests/test_map_query.py::_drive (scene 2000, poses t = (-5 + 1.5 k, -1 + 0.1 k, 0), yaw 0.05 k, noise seeds 50 + k) with one more box per
    scan k: a car that moves 2 m per scan.  All scans at their true poses, cell 0.1.  dict(scans, poses, boxes, ground, model, ext)."""
    key = (rings, steps)
    if key not in _CAR:
        from icet_amd import lidar_sim
        scene = lidar_sim.make_scene(2000)
        boxes = car_boxes(scene)
        poses, scans = [], []
        for k in range(8):
            t = (-5.0 + 1.5 * k, -1.0 + 0.1 * k, 0.0)
            T = mm.pose(t=t, r=(0, 0, 0.05 * k))
            poses.append(T)
            sc = dict(scene); sc["boxes"] = list(scene["boxes"]) + [boxes[k]]
            s = lidar_sim.make_scan(sc, (np.array(t), T[:3, :3].astype(np.float64)), 50 + k, rings=rings, steps=steps)
            scans.append(np.ascontiguousarray(s.cpu().numpy().T))
        model = mm.Map(0.1).add(scans, np.stack(poses))
        _CAR[key] = dict(scans=scans, poses=np.stack(poses), boxes=boxes, ground=scene["ground"], model=model, ext=model.extract(1))
    return _CAR[key]


def mover_cells(xyz, boxes, ground):
    """Cells whose centroid lies within 0.1 m of any of the boxes and more than 0.25 m above the ground."""
    m = np.zeros(xyz.shape[0], bool)
    for x0, x1, y0, y1, z0, z1 in boxes:
        m |= ((xyz[:, 0] >= x0 - 0.1) & (xyz[:, 0] <= x1 + 0.1) & (xyz[:, 1] >= y0 - 0.1) & (xyz[:, 1] <= y1 + 0.1) & (xyz[:, 2] >= z0 - 0.1) & (xyz[:, 2] <= z1 + 0.1))
    return m & (xyz[:, 2] > ground + 0.25)
