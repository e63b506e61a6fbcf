"""CPU tests of the deskew rule's NumPy model (tests/deskew_model.py; include/icet_hip.h icet_deskew_*): the three series against exact
rational sums, the model against a closed-form exp, the group property, a zero twist, the class table, the simulator's moving sweep against its own world
points, and the sharpness of a map fused from deskewed sweeps against one fused from raw sweeps."""
from fractions import Fraction
import math

import numpy as np
import pytest

import deskew_model as dm
from icet_amd import lidar_sim as ls


def _ulp(v):
    return float(np.spacing(np.float64(abs(v))))


@pytest.mark.parametrize("u", [0.0, 1e-300, 1e-8, 0.25, 1.0])
def test_series_equal_the_exact_rational_sums_within_a_few_ulp(u):
    """sum_k (-1)^k u^k / (2k + j)! for j = 1, 2, 3 in exact rationals (u itself is a double, so Fraction(u) is exact), k = 0 .. 9; the infinite series
    differs from that by less than the first dropped term, u^10 / (21 + j - 1)! <= 1 / 21!.  Horner in double: ten steps of at most one ulp each on a sum
    that is dominated by its first term, so four ulp of the value is a generous bound (the terms fall by 1 / 6 or faster)."""
    fu = Fraction(u)
    for j, c in ((1, dm.FA), (2, dm.FB), (3, dm.FC)):
        exact = sum(Fraction((-1) ** k, math.factorial(2 * k + j)) * fu ** k for k in range(10))
        got = float(dm.horner(c, u))
        remainder = float(fu ** 10 / math.factorial(20 + j))
        err = abs(Fraction(got) - exact)
        print("u = %g j = %d: |horner - exact| = %.3g ulp, remainder %.3g" % (u, j, float(err) / _ulp(got), remainder))
        assert err <= 4 * Fraction(_ulp(got)), (u, j)
        assert remainder <= 1.0 / math.factorial(21)
    # the closed forms the series stand for
    if u > 0:
        t = math.sqrt(u)
        assert abs(float(dm.horner(dm.FA, u)) - math.sin(t) / t) <= 1e-15


def test_model_equals_a_closed_form_exp_out_to_120_m():
    """Rows out to 120 m, d in [-1, 1], twists up to 1 rad of rotation: the float64 value before the final rounding against R p + t from np.sin / np.cos."""
    rs = np.random.RandomState(11)
    worst = 0.0
    for _ in range(20):
        xi = np.concatenate([rs.uniform(-3, 3, 3), rs.uniform(-1, 1, 3) * 0.57])
        rows = (rs.uniform(-1, 1, (200, 3)) * [120, 120, 10]).astype(np.float32)
        s = rs.uniform(0, 1, 200).astype(np.float32)
        ref = float(rs.uniform(0, 1))
        R, t = dm.exp_closed(xi, s.astype(np.float64) - ref)
        want = np.einsum("nab,nb->na", R, rows.astype(np.float64)) + t
        out, cls = dm.deskew(rows, xi, s, ref=ref)
        assert (cls == dm.MOVED).all()
        # the model's own float64 value: redo the arithmetic without the final rounding
        d = s.astype(np.float64) - ref
        th = d[:, None] * xi[None, 3:]; sg = d[:, None] * xi[None, :3]
        u = (th[:, 0] ** 2 + th[:, 1] ** 2) + th[:, 2] ** 2
        A, B, Cc = dm.horner(dm.FA, u), dm.horner(dm.FB, u), dm.horner(dm.FC, u)
        p = rows.astype(np.float64)
        c1 = dm.cross(th, p); c2 = dm.cross(th, c1); r1 = dm.cross(th, sg); r2 = dm.cross(th, r1)
        o = ((p + A[:, None] * c1) + B[:, None] * c2) + ((sg + B[:, None] * r1) + Cc[:, None] * r2)
        assert np.array_equal(o.astype(np.float32).view(np.uint32), out.view(np.uint32))
        worst = max(worst, float(np.abs(o - want).max()))
    print("max |model - closed form| = %.3g m" % worst)
    assert worst <= 1e-9


def test_group_property_ref_a_then_the_step_to_ref_b():
    """Deskewing to ref a and then applying exp((a - b) xi) equals deskewing to ref b, within float32 rounding of the coordinates: half an ulp at the size of the
    rows on the intermediate result, carried through a rotation (three terms), and half an ulp on each final result -- four ulp of float32 at the largest
    coordinate."""
    rs = np.random.RandomState(12)
    xi = dm.TWIST * 2.0
    rows = (rs.uniform(-1, 1, (500, 3)) * [100, 100, 10]).astype(np.float32)
    s = rs.uniform(0, 1, 500).astype(np.float32)
    for a, b in ((0.0, 1.0), (1.0, 0.0), (0.25, 0.75)):
        oa, _ = dm.deskew(rows, xi, s, ref=a)
        ob, _ = dm.deskew(rows, xi, s, ref=b)
        R, t = dm.exp_closed(xi, [a - b])
        moved = oa.astype(np.float64) @ R[0].T + t[0]
        tol = 4 * float(np.spacing(np.float32(np.abs(rows).max() + np.abs(xi[:3]).sum())))
        err = float(np.abs(moved - ob.astype(np.float64)).max())
        print("ref %g -> %g: %.3g m (bound %.3g)" % (a, b, err, tol))
        assert err <= tol


def test_zero_twist_returns_every_finite_row_unchanged():
    rs = np.random.RandomState(13)
    rows = (rs.randn(1000, 3) * [40, 40, 4]).astype(np.float32)
    rows[::7] = 0.0
    rows[5] = [1e-42, -1e-45, 3e-39]
    s = rs.uniform(-0.5, 1.5, 1000).astype(np.float32)
    out, cls = dm.deskew(rows, np.zeros(6), s, ref=0.3)
    assert (out == rows).all()
    assert np.array_equal(out.view(np.uint32), rows.view(np.uint32))
    assert dm.counts(cls)["zero"] == len(rows[::7]) and dm.counts(cls)["moved"] == 1000 - len(rows[::7])


def test_class_table():
    for rows, time, twist, kw, exp in dm.class_table():
        out, cls = dm.deskew(rows, twist, time, **kw)
        assert list(cls) == exp, (rows, time, kw)
        keep = cls != dm.MOVED
        assert np.array_equal(out[keep].view(np.uint32), np.asarray(rows, np.float32)[keep].view(np.uint32))      # signed zeros, NaN payloads: the bits
    # s < 0 and s > 1 are extrapolated as they stand: the same row at -0.7 and 1.9 moves to two different places, both finite
    rows, time, twist, kw, _ = dm.class_table()[0]
    out, _ = dm.deskew(rows, twist, time, **kw)
    assert np.isfinite(out[13:15]).all() and not np.array_equal(out[13], out[14]) and not np.array_equal(out[13], rows[13])
    # the column modes: row i of a scan with `period` columns, ring index slow / with `period` rows per column
    r = np.ones((12, 3), np.float32)
    fast, _ = dm.deskew(r, dm.TWIST, None, dm.TIME_COLUMN_FAST, 4, 0.0, 0.25, 0.0)
    slow, _ = dm.deskew(r, dm.TWIST, None, dm.TIME_COLUMN_SLOW, 3, 0.0, 0.25, 0.0)
    arr_f, _ = dm.deskew(r, dm.TWIST, (np.arange(12) % 4 + 0.5).astype(np.float32), dm.TIME_ARRAY, 0, 0.0, 0.25, 0.0)
    arr_s, _ = dm.deskew(r, dm.TWIST, (np.arange(12) // 3 + 0.5).astype(np.float32), dm.TIME_ARRAY, 0, 0.0, 0.25, 0.0)
    assert np.array_equal(fast.view(np.uint32), arr_f.view(np.uint32)) and np.array_equal(slow.view(np.uint32), arr_s.view(np.uint32))
    assert not np.array_equal(fast, slow)


def test_pose_and_twist_round_trip_in_the_model():
    for ang in (0.0, 1e-10, 1e-3, 0.1, 0.7, 1.5):
        xi = np.array([1.0, -2.0, 0.5, ang * 0.6, -ang * 0.64, ang * 0.48])
        assert np.abs(dm.twist_from_pose(dm.pose_from_twist(xi)) - xi).max() <= 1e-12
        R, t = dm.exp_closed(xi, [1.0])
        T = dm.pose_from_twist(xi)
        assert np.abs(T[:3, :3] - R[0]).max() <= 1e-14 and np.abs(T[:3, 3] - t[0]).max() <= 1e-14
    T = dm.pose_from_twist([0.3, 0.1, 0.0, 0.01, 0.02, 0.5]).astype(np.float32)
    assert (dm.twist_between(T, T, 3.0) == 0).all()                  # identical poses: exactly zero


@pytest.fixture(scope="module")
def truth_sweep():
    scene = ls.make_scene(2000)
    scan, s, world = ls.make_sweep(scene, (np.zeros(3), np.eye(3)), dm.TWIST, 1, 16, 256, 0.0, return_world=True)
    return scan.numpy().T.copy(), s.numpy(), world.numpy()


def test_simulator_truth_a_deskewed_sweep_lies_on_the_world_points(truth_sweep):
    """pose_start the identity, no range noise, ref 0: the deskewed rows are the ray caster's world hits.  Bound 2e-5 m: half an ulp of float32 at 120 m
    (3.8e-6) on the input and again on the output, plus the double arithmetic."""
    rows, s, world = truth_sweep
    out, cls = dm.deskew(rows, dm.TWIST, s, ref=0.0)
    assert (cls == dm.MOVED).all() and rows.shape[0] > 3000
    raw = float(np.abs(rows - world).max()); err = float(np.abs(out - world).max())
    print("raw rows off by %.3f m, deskewed rows off by %.3g m" % (raw, err))
    assert raw > 1.0
    assert err <= 2e-5


def test_make_sweep_layouts(truth_sweep):
    scene = ls.make_scene(2000)
    rows, s, _ = truth_sweep
    org, so, wo = ls.make_sweep(scene, (np.zeros(3), np.eye(3)), dm.TWIST, 1, 16, 256, 0.0, drop=False, return_world=True)
    org = org.numpy().T; so = so.numpy(); wo = wo.numpy()
    assert org.shape == (16 * 256, 3) and np.array_equal(so, ((np.arange(16 * 256) % 256 + 0.5) / 256).astype(np.float32))
    miss = (org == 0).all(1)
    assert miss.any() and not org[miss].view(np.uint32).any() and np.isnan(wo[miss]).all() and np.array_equal(org[~miss], rows) and np.array_equal(so[~miss], s)
    az, sa = ls.make_sweep(scene, (np.zeros(3), np.eye(3)), dm.TWIST, 1, 16, 256, 0.0, order="azimuth", drop=False)
    az = az.numpy().T
    assert np.array_equal(sa.numpy(), ((np.arange(16 * 256) // 16 + 0.5) / 256).astype(np.float32))
    assert np.allclose(az.reshape(256, 16, 3).transpose(1, 0, 2).reshape(-1, 3), org, atol=1e-5)
    # a still sensor: the sweep is make_scan's scan
    still, _ = ls.make_sweep(scene, (np.zeros(3), np.eye(3)), np.zeros(6), 7, 16, 256)
    assert np.array_equal(still.numpy(), ls.make_scan(scene, (np.zeros(3), np.eye(3)), 7, 16, 256).numpy())


def test_map_of_deskewed_sweeps_is_sharper():
    """Fused at their true start poses into cells of 0.5 m, the deskewed sweeps occupy strictly fewer cells than the raw ones (DESIGN.md section 24 quotes both)."""
    skewed, deskewed = dm.sharpness_counts(0.5)
    print("cells of 0.5 m: %d skewed, %d deskewed" % (skewed, deskewed))
    assert deskewed < skewed
