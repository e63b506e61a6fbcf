"""THE SHARED ARITHMETIC RULE pinned: angles and the spherical round trip against correctly rounded values.

Every bit-for-bit comparison between the device and the oracle rests on one sentence -- every transcendental that feeds a stored value is the correctly rounded
float32 of the exact function value.  tests/arith_rule_model.py follows that sentence with mpmath deciding every close call; here the oracle (CPU) and the device
(icet_debug_spherical, then the production kernels of scan 2 and scan 1) are held to it, bit for bit and sign of zero included, on
  * an edge table: axes, poles, signed zeros, denormals, overflowing / underflowing squares, NaN / inf, the 2 pi wrap, voxel edges;
  * windows: rows whose azimuth lies within 2^-1 .. 2^-60 of an axis, or whose direction lies that close to the horizontal plane or a pole -- where a sine or cosine
    is tiny and its ABSOLUTE error decides the float -- and the same with the small coordinate exactly +-0;
  * searched hard cases (tests/golden/arith_rule_cases.npz, scripts/gen_arith_rule_cases.py): exact values 4 .. 64 float64-ulps (angles) or 2^-47 .. 2^-43
    (sines / cosines) from a float32 rounding boundary;
  * bulk: 2 M random rows over 80 octaves of scale.
Closer to a boundary than the lower edges of those bands two honest evaluations of the rule may round apart: over the bulk at most CAP = 2 rows may differ, and only there
(decided by mpmath); on the other sets nothing may differ.
"""
import functools
import math
import os
import sys

import mpmath
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "scripts"))
import arith_rule_model as arm      # noqa: E402
import gen_arith_rule_cases as gen      # noqa: E402

F32, F64 = np.float32, np.float64
CAP = 2
T, P = 75, 24
STRICT_SETS = ["edge", "hard"] + ["win:" + w for w in gen.WINDOWS] + ["win0:" + w for w in gen.WINDOWS]
BULK_SETS = ["bulk:sigma20", "bulk:octaves"]


@functools.lru_cache(maxsize=None)
def rows_of(name):
    if name == "edge":
        return gen.edge_table()
    if name == "hard":
        return gen.load()["xyz"]
    if name.startswith("win"):
        return gen.windows(name.split(":")[1], exact_zero=name.startswith("win0"))
    return gen.bulk()[BULK_SETS.index(name)]


@functools.lru_cache(maxsize=None)
def model_of(name):
    return arm.model(rows_of(name), T, P)


def excluded(xyz):
    """One row: is some exact transcendental of it closer to a float32 rounding boundary than the bands allow to be decided (angles: 4 float64-ulps; sines /
    cosines of the float32 angles: 2^-47 absolute)?  Returns (bool, the distances)."""
    p = np.asarray(xyz, F32).reshape(1, 3)
    sph, rr = arm.c2s(p)
    out = {}
    with mpmath.workprec(arm.PREC), np.errstate(all="ignore"):
        if np.isfinite(p).all():
            v = arm.exact_atan2(float(p[0, 1]), float(p[0, 0]))
            if v != 0:
                out["theta_ulps"] = arm.boundary_distance(v) / float(np.spacing(abs(float(v))))
            q = float(p[0, 2] / rr[0])
            if abs(q) < 1:
                v = mpmath.acos(mpmath.mpf(q)); out["phi_ulps"] = arm.boundary_distance(v) / float(np.spacing(abs(float(v))))
        for k, a in (("theta", sph[0, 1]), ("phi", sph[0, 2])):
            for fn in ("sin", "cos"):
                v = getattr(mpmath, fn)(mpmath.mpf(float(a)))
                if v != 0:
                    out[fn + "_" + k + "_abs"] = arm.boundary_distance(v)
    close = any(d < (gen.ANGLE_BAND[0] if k.endswith("ulps") else gen.TRIG_BAND[0]) for k, d in out.items())
    return close, out


def check_rows(name, got, want, what, strict):
    """got / want: float32 (N, k).  strict: no row may differ.  Otherwise at most CAP rows, each inside the excluded distance."""
    bad = np.flatnonzero(~arm.same_bits(got, want))
    xyz = rows_of(name)
    report = []
    for i in bad[:20]:
        close, dist = excluded(xyz[i])
        report.append("row %d %r: got %r want %r, excluded=%s %s" % (i, xyz[i].tolist(), np.asarray(got[i]).tolist(), np.asarray(want[i]).tolist(), close, dist))
    msg = "%s / %s: %d of %d rows differ\n%s" % (name, what, bad.size, len(xyz), "\n".join(report))
    if bad.size:
        print(msg)
    if strict:
        assert bad.size == 0, msg
    else:
        assert bad.size <= CAP and all(excluded(xyz[i])[0] for i in bad), msg
    return bad.size


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_model_pins_the_known_values():
    """sin(float(pi)) = -8.74227800037e-08 lies 1.2e-16 from a float32 rounding boundary, cos(float(pi / 2)) is half of it: the model returns the correctly rounded
    floats (-8.7422777e-08, not the -8.7422784e-08 an absolute error of a few 1e-16 produces).  The NaN -> 1000 sentinels; the wrap of -tiny to float(2 pi) and its voxel."""
    pi_f, hpi_f = F32(np.pi), F32(np.pi / 2)
    with mpmath.workprec(arm.PREC):
        s, c = mpmath.sin(mpmath.mpf(float(pi_f))), mpmath.cos(mpmath.mpf(float(hpi_f)))
        assert abs(float(s) - -8.74227800037e-08) < 1e-19 and abs(float(c) - -8.74227800037e-08 / 2) < 1e-19
        assert 1.0e-16 < arm.boundary_distance(s) < 1.4e-16 and 0.5e-16 < arm.boundary_distance(c) < 0.7e-16
    assert arm.sin_cr(np.array([pi_f]))[0] == F32(-8.7422777e-08) and arm.cos_cr(np.array([hpi_f]))[0] == F32(-8.7422777e-08 / 2)
    assert arm.sin_cr(np.array([pi_f]))[0] != F32(-8.7422784e-08)
    p = np.array([[0, 0, 0], [np.nan, 1, 1], [1, np.nan, 1], [np.inf, 1, 1], [1, -1e-45, 0.25], [1, -0.0, 0.25], [-1, -0.0, 0], [-1, 0.0, 0]], F32)
    m = arm.model(p, T, P)
    assert m["sph"][0].tolist() == [0.0, 0.0, 1000.0] and m["sph"][1].tolist() == [1000.0, 1000.0, 1000.0] and m["sph"][2].tolist() == [1000.0, 1000.0, 1000.0]
    assert m["sph"][3].tolist() == [np.inf, 0.0, float(hpi_f)]                             # r = inf is no NaN: it stays, and acos(1 / inf) = pi / 2
    assert m["sph"][4, 1] == F32(2 * np.pi) and m["voxel"][4] % T == 0                    # -tiny wraps to float(2 pi), which falls into azimuth bin 0
    assert m["sph"][5, 1] == 0 and np.signbit(m["sph"][5, 1]) and np.signbit(m["rt"][5, 1]) and m["rt"][5, 1] == 0      # atan2(-0, +) = -0 is not negative: oy = -0
    assert m["sph"][6, 1] == F32(float(-pi_f) + 2 * np.pi) and m["sph"][6, 1] == np.nextafter(pi_f, F32(0))           # -pi wraps to the float BELOW float(pi)
    assert m["sph"][7, 1] == pi_f and m["sph"][7, 2] == hpi_f and m["rt"][7].tolist() == [-1.0, float(F32(-8.7422777e-08)), float(F32(-8.7422777e-08 / 2))]
    assert m["ordinary"].tolist() == [False, False, False, False, True, True, True, True]


@pytest.mark.parametrize("name", STRICT_SETS + BULK_SETS)
def test_oracle_follows_the_rule(name):
    """The oracle's c2s and s2c(c2s(.)) -- glibc's float64 functions rounded once -- equal the model bit for bit: the edge table, the windows, the hard cases, 100 k rows
    of each bulk set.  At most CAP rows may differ over all sets, each inside the excluded distance."""
    from oracle import pyoracle as po
    xyz, m = rows_of(name), model_of(name)
    sel = slice(None) if name not in BULK_SETS else slice(0, 100_000)
    strict = False
    n = check_rows(name, po.c2s(xyz[sel]), m["sph"][sel], "oracle c2s", strict) + check_rows(name, po.roundtrip(xyz[sel]), m["rt"][sel], "oracle roundtrip", strict)
    test_oracle_follows_the_rule.differing = getattr(test_oracle_follows_the_rule, "differing", 0) + n
    assert test_oracle_follows_the_rule.differing <= CAP


def test_fixture_is_what_its_metadata_says():
    c = gen.load()
    assert c["meta"]["seed"] == gen.SEED and c["xyz"].dtype == F32 and len(c["xyz"]) == len(c["kind"]) == len(c["dist"]) <= 4000
    assert c["meta"]["count_per_kind"] == [int((c["kind"] == k).sum()) for k in range(6)] and min(c["meta"]["count_per_kind"]) >= 30
    ang = c["kind"] < 2
    assert (c["dist"][ang] >= gen.ANGLE_BAND[0]).all() and (c["dist"][ang] <= gen.ANGLE_BAND[1]).all()
    assert (c["dist"][~ang] >= gen.TRIG_BAND[0]).all() and (c["dist"][~ang] <= gen.TRIG_BAND[1]).all()
    for i in (0, len(c["kind"]) // 2, len(c["kind"]) - 1):                                 # the recorded distance is the exact one
        assert gen._confirm(int(c["kind"][i]), c["xyz"][i]) == c["dist"][i]


# -- the wedge scan: scan 1's production path (k_fit_roundtrip) --------------------------------------------------------------------
def voxel_moments(rows):
    """mean and covariance of the oracle's mean_cov under the shared rule: exact sums over float32 addends, rounded once, divided in float32."""
    m = len(rows)
    mean = np.array([F32(math.fsum(rows[:, a].astype(F64))) / F32(m) for a in range(3)], F32)
    d = rows - mean
    cov = np.array([[F32(math.fsum((d[:, a] * d[:, b]).astype(F64))) / F32(m - 1) for b in range(3)] for a in range(3)], F32)
    return mean, cov


@functools.lru_cache(maxsize=None)
def wedge():
    from oracle import pyoracle as po
    scan, win = gen.wedge_scan()
    ref = po.solve(scan, scan, runlen=1, bins_phi=gen.WEDGE_P, bins_theta=gen.WEDGE_T, trace=True)
    return scan, win, ref


def test_wedge_scan_can_see_the_defect():
    """The condition of the scan-1 test, checked with the oracle alone: per window at least 40 wedge voxels are fitted; rebuilding their moments from the MODEL's round
    trip gives the oracle's mu1 / sigma1 bits; and per window (-x, +-y, the horizontal plane) at least one of them changes its sigma1 bits when the rows come from the algebraic evaluation instead."""
    scan, win, ref = wedge()
    t = ref["trace"]
    m = arm.model(scan, gen.WEDGE_T, gen.WEDGE_P)
    alg = arm.algebraic_roundtrip(scan)
    sph, b = m["sph"], t["bounds"]
    seen = {}
    for w, name in enumerate(gen.WEDGE_WINDOWS):
        vox = np.unique(m["voxel"][win == w])
        fitted = [v for v in vox if t["has_fit"][v] == 1]
        assert len(vox) == 50 and len(fitted) >= 40, (name, len(vox), len(fitted))
        changed = 0
        for v in fitted:
            rows = np.flatnonzero((m["voxel"] == v) & (sph[:, 1] >= b[v, 0]) & (sph[:, 1] <= b[v, 1]) & (sph[:, 2] >= b[v, 2]) & (sph[:, 2] <= b[v, 3])
                                  & (sph[:, 0] >= b[v, 4]) & (sph[:, 0] <= b[v, 5]))
            assert (win[rows] == w).all() and len(rows) >= 25
            mean, cov = voxel_moments(m["rt"][rows])
            assert np.array_equal(mean.view(np.uint32), t["mu1"][v].view(np.uint32)) and np.array_equal(cov.view(np.uint32), t["sigma1"][v].view(np.uint32)), (name, v)
            changed += not np.array_equal(voxel_moments(alg[rows])[1].view(np.uint32), cov.view(np.uint32))
        print("window %s: %d fitted voxels, %d change sigma1 under the algebraic evaluation" % (name, len(fitted), changed))
        seen[name[-1] if name[-1] in "xy" else name] = seen.get(name[-1] if name[-1] in "xy" else name, 0) + changed
    # (-y on its own shows nothing in the float64 restatement: there glibc's atan2 errs to the harmless side of -pi / 2; the +-y axes count as the one window they are)
    assert min(seen.values()) >= 1 and sorted(seen) == ["plane", "x", "y"], seen


# ---------------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", STRICT_SETS + BULK_SETS)
def test_device_functions_follow_the_rule(gpu_ctx, name):
    """icet_debug_spherical against the model: r, theta, phi, voxel, the round trip of any row and the ordinary-row round trip called as k_fit_roundtrip calls it."""
    xyz, m = rows_of(name), model_of(name)
    g = gpu_ctx.debug_spherical(xyz, T, P)
    strict = name in STRICT_SETS
    ordinary = m["ordinary"]
    nan = np.full((len(xyz), 5), np.nan, F32)
    want_cr = np.where(ordinary[:, None], np.concatenate([m["sph"][:, 1:], m["rt"]], 1), nan)
    got = np.concatenate([g["sph"], g["voxel"].view(F32)[:, None], g["rt_any"], g["cr_ang"], g["cr"]], 1)
    want = np.concatenate([m["sph"], m["voxel"].view(F32)[:, None], m["rt"], want_cr], 1)
    for lo, hi, what in ((0, 3, "c2s_cr"), (3, 4, "voxel_of"), (4, 7, "roundtrip_any"), (7, 12, "roundtrip_cr")):
        check_rows(name, got[:, lo:hi], want[:, lo:hi], what, strict)
    check_rows(name, got, want, "all outputs", strict)                                   # (the cap holds for the rows, not per output)


@pytest.mark.gpu
def test_scan2_round_trip_follows_the_rule(frames):
    """The production path of ICET_FLAG_ROUNDTRIP_SCAN2 (k_rt2_prepare): the window rows and the edge table fed as scan 2; the round-tripped copy the loop reads is the
    model's, bit for bit."""
    import icet_amd
    from icet_amd import api
    names = [n for n in STRICT_SETS if n != "hard"]
    b = np.concatenate([rows_of(n) for n in names]); want = np.concatenate([model_of(n)["rt"] for n in names])
    ctx = icet_amd.Context(0)
    try:
        ctx.solve(frames[0], b, 1, np.zeros(6), P, T, flags=api.FLAG_ROUNDTRIP_SCAN2)
        n = b.shape[0]; ld = (n + 63) // 64 * 64
        og = ctx.debug_fetch("rt2", 3 * ld).reshape(3, ld)[:, :n].T
    finally:
        ctx.close()
    bad = np.flatnonzero(~arm.same_bits(og, want))
    assert bad.size == 0, "%d of %d rows differ, first: %r" % (bad.size, n, [(int(i), b[i].tolist(), og[i].tolist(), want[i].tolist()) for i in bad[:8]])


@pytest.mark.gpu
def test_scan1_fit_of_wedge_clusters_is_the_oracles(gpu_ctx):
    """The production path of scan 1 (k_fit_roundtrip -> k_fit_moments): every fitted voxel of the wedge scan has the oracle's mu1 and sigma1 bits.
    test_wedge_scan_can_see_the_defect shows that these voxels tell the correctly rounded round trip from the algebraic one."""
    scan, win, ref = wedge()
    t = ref["trace"]
    g = gpu_ctx.solve(scan, scan, 1, np.zeros(6), gen.WEDGE_P, gen.WEDGE_T, aux=True)["aux"]
    assert np.array_equal(g["n1_raw"], t["n1_raw"]) and np.array_equal(g["has_fit"], t["has_fit"]) and np.array_equal(g["cluster_bounds"], t["bounds"])
    f = t["has_fit"] == 1
    assert int(f.sum()) >= 160
    bad_mu = np.flatnonzero(~arm.same_bits(g["mu1"][f], t["mu1"][f])); bad_sg = np.flatnonzero(~arm.same_bits(g["sigma1"][f].reshape(-1, 9), t["sigma1"][f].reshape(-1, 9)))
    print("fitted voxels %d: mu1 differs in %d, sigma1 in %d" % (int(f.sum()), bad_mu.size, bad_sg.size))
    assert bad_mu.size == 0 and bad_sg.size == 0, (np.flatnonzero(f)[bad_mu][:10], np.flatnonzero(f)[bad_sg][:10])
