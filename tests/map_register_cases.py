"""Inputs shared by the tests of the registration against a shaped voxel map: small maps with every kind of cell, the rows that exercise
every class, and the convergence scene with the model's own results on it -- each built once per session."""
import functools

import numpy as np

import map_model as mm
import map_register_model as rm
import map_shape_model as sm

ROW_COUNTS = (1, 255, 256, 2047, 2048, 2049, 4097)                    # around the 256-lane trip, the 2048-row chunk and two chunks
POSE = mm.pose(t=(0.37, -0.21, 0.11), r=(0.02, -0.015, 0.4))           # not axis-aligned


def base_map(cell, seed=31):
    """(fused scans, poses): a slab of 16 x 16 x 3 cells around the origin, 9000 rows seen from two poses, so that most of its cells hold several rows."""
    rs = np.random.RandomState(seed)
    ext = np.array([16.0, 16.0, 3.0]) * cell
    a = (rs.rand(6000, 3) * ext - ext / 2).astype(np.float32)
    b = (rs.rand(3000, 3) * ext - ext / 2).astype(np.float32)
    return [a, b], [mm.pose(), mm.pose(t=(0.4 * cell, 0.2 * cell, 0.0), r=(0.0, 0.0, 0.1))]


def special_cells(cell):
    """Scans that make, above and below the slab, a cell below min_points (2 rows), an emptied cell (added, then removed) and a negative-count cell (removed only):
    (add scans, remove scans, the three world points), all at the identity pose."""
    c = float(np.float32(cell))
    few = np.array([[0.3 * c, 0.4 * c, 45.25 * c], [0.6 * c, 0.5 * c, 45.75 * c]], np.float32)
    gone = np.array([[0.3 * c, 0.4 * c, -49.75 * c], [0.6 * c, 0.7 * c, -49.25 * c]], np.float32)
    neg = np.array([[0.3 * c, 0.4 * c, 55.25 * c], [0.5 * c, 0.6 * c, 55.5 * c]], np.float32)
    return [few, gone], [gone, neg], np.stack([few[0], gone[0], neg[0]])


def model_map(cell):
    """The ShapeMap of base_map and special_cells."""
    scans, poses = base_map(cell)
    add, rem, _ = special_cells(cell)
    m = sm.ShapeMap(cell).add(scans, poses)
    m.add(add, [mm.pose()] * len(add))
    m.remove(rem, [mm.pose()] * len(rem))
    return m


def term_rows(cell, n, pose=POSE, seed=5):
    """n rows in the SENSOR frame of ``pose``: the first ones are the named edge cases -- a NaN, an infinite and an all-zero row, a row below min_range 0.05 and
    one beyond max_range 30, a row outside the grid, a row in an empty cell, one in each special cell -- the rest fall in and around the slab."""
    rs = np.random.RandomState(seed + n)
    T = np.asarray(pose, np.float64)
    ext = np.array([18.0, 18.0, 4.0]) * cell
    w = rs.rand(n, 3) * ext - ext / 2
    _, _, pts = special_cells(cell)
    named_w = [np.array([0.0, 0.0, 25.0])] + [p.astype(np.float64) for p in pts]      # an empty cell, then few / gone / neg
    k = 0
    for p in named_w:
        if k < n:
            w[k] = p; k += 1
    rows = ((w - T[:3, 3]) @ T[:3, :3]).astype(np.float32)              # R^T (w - t)
    named = [[np.nan, 1, 1], [1, np.inf, 1], [0, 0, 0], [0.01, 0.02, 0.01], [25, 25, 1], [3e5 * cell, 3e5 * cell, 1.1e6 * cell]]
    for p in named:
        if k < n:
            rows[k] = p; k += 1
    return rows


@functools.lru_cache(maxsize=None)
def scene():
    """The convergence case: lidar_sim.make_scene(3100), eight scans of rings=16, steps=512 along a gently curving path, fused at cell 0.5; two held-out scans at
    poses between them; per held-out scan three starts perturbed in translation and yaw.  dict(cell, scans, poses, G, held [(scan, true pose)], starts [(held
    index, start pose)], params)."""
    from icet_amd import lidar_sim as ls
    sc = ls.make_scene(3100)

    def P(x, y, yaw):
        return mm.pose(t=(x, y, 0.0), r=(0, 0, yaw))

    def scan_at(T, seed):
        T = np.asarray(T, np.float64)
        return ls.make_scan(sc, (T[:3, 3], T[:3, :3]), seed, rings=16, steps=512).numpy().T.copy()

    poses = [P(1.5 * k, 0.05 * k, 0.01 * k) for k in range(8)]
    scans = [scan_at(T, 500 + k) for k, T in enumerate(poses)]
    m = sm.ShapeMap(0.5).add(scans, poses)
    held = [(scan_at(T, 900 + i), T) for i, T in enumerate((P(2.2, 0.1, 0.02), P(6.8, 0.3, 0.05)))]
    starts = []
    for i, (_, T) in enumerate(held):
        yaw = float(np.arctan2(T[1, 0], T[0, 0]))
        for dx, dy, dyaw in ((0.2, 0.1, 0.02), (-0.2, 0.15, -0.03), (0.1, -0.2, 0.03)):
            starts.append((i, mm.pose(t=(T[0, 3] + dx, T[1, 3] + dy, 0.03), r=(0, 0, yaw + dyaw))))
    return dict(cell=0.5, scans=scans, poses=poses, map=m, G=rm.Gaussians(m), held=held, starts=starts, params=dict(max_iters=64))


@functools.lru_cache(maxsize=None)
def scene_model(order="forward"):
    """The model's record per start of scene(), its rows summed in ``order``."""
    s = scene()
    return [rm.register(s["held"][i][0], T0, s["G"], order=order, **s["params"]) for i, T0 in s["starts"]]


def pose_diff(a, b):
    """The largest absolute difference between the entries of two 4 x 4 (or (R, t)) poses, in float64."""
    if isinstance(a, tuple):
        return max(float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()))
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
