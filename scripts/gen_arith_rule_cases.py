#!/usr/bin/env python3
"""Inputs of the shared-arithmetic-rule tests (tests/test_arith_rule.py): rows at which cartesianToSpherical / sphericalToCartesian can go wrong.

What is built in milliseconds is built by the tests from the functions below (edge_table, windows, bulk, wedge_scan); what has to be SEARCHED is kept in
tests/golden/arith_rule_cases.npz, which this script reproduces byte for byte from SEED:

    python scripts/gen_arith_rule_cases.py [--check]        # --check: build in memory and compare with the committed file

Searched hard cases (float32 rows, each with the distance of the exact function value to the nearest float32 rounding boundary):
  kinds 0 / 1   theta = atan2(y, x) / phi = acos(z / r) whose exact value lies ANGLE_BAND = 4 .. 64 float64-ulps from a boundary.  The lower edge is twice an
                assumed 2-ulp error of the device library's float64 atan2 / acos (no error table for them is installed with the ROCm documentation this was
                written against): closer than that the rule's two evaluations may legitimately round apart, farther they may not.
  kinds 2 .. 5  sin theta / cos theta / sin phi / cos phi of the row's float32 angles whose exact value lies TRIG_BAND = 2^-47 .. 2^-43 (absolute) from a boundary.
                The lower edge is about three times the absolute error bound of the device's algebraic evaluation, 2.1e-15 = 2 ulp of a float64 in [4, 8)
                (the angle's error under the same assumption) + three roundings of values <= 1.
The search filters random rows (normal, sigma = 20 m) through float64 and confirms every hit with mpmath.
"""
import argparse
import io
import json
import os
import sys
import zipfile
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import arith_rule_model as arm      # noqa: E402

F32, F64 = np.float32, np.float64
SEED = 20261
FIXTURE = os.path.join(ROOT, "tests", "golden", "arith_rule_cases.npz")
ANGLE_BAND = (4.0, 64.0)                    # float64 ulps of the angle
TRIG_BAND = (2.0 ** -47, 2.0 ** -43)        # absolute
CHUNK = 5_000_000
ANGLE_CHUNKS = 200                          # 1e9 rows filtered for kinds 0 / 1
TRIG_CHUNKS = 4                             # 2e7 rows for kinds 2 .. 5 (their band is ~1e4 times likelier)
TRIG_KEEP = 48                              # per kind
KINDS = ("theta", "phi", "sin_theta", "cos_theta", "sin_phi", "cos_phi")


# ---------------------------------------------------------------------------------------------------------------- built at test time
def edge_table():
    """Axes, poles, signed zeros, denormals, squares that overflow / underflow, NaN / inf, the 2 pi wrap, voxel edges of 75 x 24 and 10000 x 1."""
    v = np.array([0.0, -0.0, 1, -1, 3.5, -3.5, 1e-30, -1e-30, 1e-42, -1e-42, 1e19, -1e19], F32)
    g = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    odd = np.array([np.nan, np.inf, -np.inf], F32)
    fin = np.array([0.0, -0.0, 1.0, -2.5], F32)
    rows = [g]
    for a in odd:
        for k in range(3):
            for b in fin:
                for c in fin:
                    r = [b, c]; r.insert(k, a); rows.append(np.array([r], F32))
        for b in odd:
            rows.append(np.array([[a, b, 1.0], [a, 1.0, b], [1.0, a, b], [a, b, a]], F32))
    # y = -eps x across the 2 pi wrap (x > 0: theta -> float(2 pi); x < 0: just past pi), eps = 2^-k down to the last denormal
    for x in (1.0, 3.5, 77.0, -1.0, -3.5):
        y = -np.abs(np.ldexp(F32(x), -np.arange(1, 152))).astype(F32)
        y = np.unique(y[y != 0]); y = np.concatenate([y, [F32(-1e-45)]]).astype(F32)
        rows.append(np.stack([np.full_like(y, x), y, np.full_like(y, 0.25 * abs(x))], 1))
    # rows on voxel edges: the float32 edge angles of clusterBounds and their neighbours, turned into points
    def on_edges(T, P, ks, js):
        az = ((ks.astype(F32) / F32(T)).astype(F64) * arm.TWO_PI).astype(F32)
        el = ((js.astype(F32) / F32(P)).astype(F64) * np.pi).astype(F32)
        out = []
        for d in (-1, 0, 1):
            a = az if d == 0 else np.nextafter(az, F32(d * 10)); e = el if d == 0 else np.nextafter(el, F32(d * 10))
            a64, e64 = a.astype(F64), e.astype(F64)
            for R in (1.0, 7.3, 41.0):
                out.append(np.stack([R * np.cos(a64) * 0.8, R * np.sin(a64) * 0.8, np.full_like(a64, 0.6 * R)], 1))          # azimuth edges
                out.append(np.stack([R * np.sin(e64) * 0.6, R * np.sin(e64) * 0.8, R * np.cos(e64)], 1))                      # polar edges
        return np.concatenate(out).astype(F32)
    rows.append(on_edges(75, 24, np.arange(0, 76), np.arange(0, 25)))
    rows.append(on_edges(10000, 1, np.arange(0, 10001, 97), np.array([0, 1])))
    return np.concatenate(rows).astype(F32)


WINDOWS = ("+x", "-x", "+y", "-y", "plane", "poles")


def windows(which, n=20000, exact_zero=False, seed=SEED):
    """n rows of one window: the small coordinate is 2^-u times the large one, u uniform over 1 .. 60, every sign pattern; exact_zero: it is +-0 instead."""
    rng = np.random.default_rng([seed, WINDOWS.index(which), int(exact_zero)])
    rho = np.exp(rng.uniform(np.log(0.5), np.log(80.0), n))
    small = rho * 2.0 ** -rng.uniform(1.0, 60.0, n)
    if exact_zero:
        small = np.zeros(n)
    s1, s2, s3 = (rng.integers(0, 2, n) * 2.0 - 1.0 for _ in range(3))
    if which in ("+x", "-x", "+y", "-y"):
        big = rho * (1.0 if which[0] == "+" else -1.0)
        z = rho * np.tan(rng.uniform(-0.4, 0.4, n))
        x, y = (big, s1 * small) if which[1] == "x" else (s1 * small, big)
    elif which == "plane":
        a = rng.uniform(0, 2 * np.pi, n)
        x, y, z = rho * np.cos(a), rho * np.sin(a), s1 * small
    else:
        a = rng.uniform(0, 2 * np.pi, n)
        x, y, z = s2 * np.abs(small * np.cos(a)), s3 * np.abs(small * np.sin(a)), s1 * rho
    return np.stack([x, y, z], 1).astype(F32)


def bulk(n=1_000_000, seed=SEED):
    """(n normal rows, sigma = 20 m; n normal rows scaled by 2^k, k in -40 .. 39)."""
    rng = np.random.default_rng([seed, 100])
    a = (rng.standard_normal((n, 3)) * 20.0).astype(F32)
    b = np.ldexp(rng.standard_normal((n, 3)), rng.integers(-40, 40, (n, 1))).astype(F32)
    return a, b


WEDGE_T, WEDGE_P = 75, 65                   # an odd number of polar bins: the horizontal plane lies in the middle of bin 32, not on an edge
WEDGE_WINDOWS = ("-x", "+y", "-y", "plane")


def wedge_scan(seed=SEED, clusters=50, rows=60):
    """A synthetic scan 1 of wedge clusters on a WEDGE_T x WEDGE_P grid: every row of a voxel lies in ONE window (its azimuth rounds to float(pi),
    float(pi / 2), float(3 pi / 2), or its polar angle to float(pi / 2)), so the voxel's Gaussian is built from round-tripped rows whose tiny sine / cosine carries a
    whole coordinate.  One cluster per voxel: `rows` rows within 0.1 m of range, the small coordinate +-rho 2^-j, j over 25 .. 40 -- every angle rounds to the
    axis' float32 exactly, so the round-tripped small coordinate is rho sin(phi) sin(float(pi)) and its spread within a voxel is a few per cent of 1e-7 m: a last
    bit of one row's sine moves the covariance by far more than a float32 ulp (with j from 12 the rows' own 1e-3 m spread hides it; tried).  The axis windows fill polar bins
    6 .. 56 without bin 32 of their one azimuth bin, the plane window azimuth bins 12 .. 61 of polar bin 32.  Returns (scan (N, 3) float32, window index per row)."""
    rng = np.random.default_rng([seed, 200])
    pts, win = [], []
    polar_bins = [k for k in range(6, 58) if k != 32][:clusters]
    for w, name in enumerate(WEDGE_WINDOWS):
        for c in range(clusters):
            small = (rng.integers(0, 2, rows) * 2.0 - 1.0) * 2.0 ** -rng.uniform(25.0, 40.0, rows)
            rho = 6.0 + 0.05 * c + rng.uniform(0.0, 0.1, rows)
            if name == "plane":
                az = (c + 12 + 0.5 + rng.uniform(-0.3, 0.3, rows)) / WEDGE_T * 2 * np.pi
                x, y, z = rho * np.cos(az), rho * np.sin(az), rho * small
            else:
                ph = (polar_bins[c] + 0.5 + rng.uniform(-0.3, 0.3, rows)) / WEDGE_P * np.pi
                big, z = rho * np.sin(ph), rho * np.cos(ph)
                x, y = {"-x": (-big, big * small), "+y": (big * small, big), "-y": (big * small, -big)}[name]
            pts.append(np.stack([x, y, z], 1)); win.append(np.full(rows, w))
    return np.concatenate(pts).astype(F32), np.concatenate(win)


# ---------------------------------------------------------------------------------------------------------------- searched
def _boundary_dist64(v):
    """float64 estimate of |v - nearest float32 rounding boundary|."""
    lo, hi = arm.f32_neighbours(v.astype(F32))
    return np.minimum(np.abs(v - lo), np.abs(hi - v))


def _chunk(k):
    """Candidate rows of chunk k: list of (kind, row index in chunk, xyz)."""
    rng = np.random.default_rng([SEED, 300, k])
    p = (rng.standard_normal((CHUNK, 3)) * 20.0).astype(F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rr = arm.radius_raw(x, y, z)
    td = np.arctan2(y.astype(F64), x.astype(F64))
    pd = np.arccos((z / rr).astype(F64))
    hits = []
    for kind, v in ((0, td), (1, pd)):
        d = _boundary_dist64(v) / np.spacing(np.abs(v))
        for i in np.flatnonzero((d >= ANGLE_BAND[0] - 2) & (d <= ANGLE_BAND[1] + 2)):
            hits.append((kind, k, int(i), p[i].copy()))
    if k < TRIG_CHUNKS:
        t0 = td.astype(F32)
        th = np.where(t0 < 0, (t0.astype(F64) + arm.TWO_PI).astype(F32), t0).astype(F64)
        ph = pd.astype(F32).astype(F64)
        for kind, v in ((2, np.sin(th)), (3, np.cos(th)), (4, np.sin(ph)), (5, np.cos(ph))):
            d = _boundary_dist64(v)
            for i in np.flatnonzero((d >= TRIG_BAND[0] * 0.99) & (d <= TRIG_BAND[1] * 1.01))[:4 * TRIG_KEEP]:
                hits.append((kind, k, int(i), p[i].copy()))
    return hits


def _confirm(kind, xyz):
    """Exact distance to the boundary (kinds 0 / 1: in float64 ulps of the value; else absolute), or None outside the band."""
    import mpmath
    with mpmath.workprec(arm.PREC):
        x, y, z = (float(c) for c in xyz)
        sph, rr = arm.c2s(xyz.reshape(1, 3))
        if kind == 0:
            v = arm.exact_atan2(y, x)
        elif kind == 1:
            v = mpmath.acos(mpmath.mpf(float(F32(z) / rr[0])))
        else:
            a = mpmath.mpf(float(sph[0, 1 if kind in (2, 3) else 2]))
            v = mpmath.sin(a) if kind in (2, 4) else mpmath.cos(a)
        d = arm.boundary_distance(v)
        if kind < 2:
            d = d / float(np.spacing(abs(float(v))))
            return d if ANGLE_BAND[0] <= d <= ANGLE_BAND[1] else None
        return d if TRIG_BAND[0] <= d <= TRIG_BAND[1] else None


def search(procs):
    with Pool(procs) as pool:
        found = [h for hits in pool.imap(_chunk, range(ANGLE_CHUNKS)) for h in hits]      # imap keeps chunk order: the result does not depend on procs
    xyz, kind, dist = [], [], []
    kept = [0] * 6
    for kd, _, _, p in found:
        if kd >= 2 and kept[kd] >= TRIG_KEEP:
            continue
        d = _confirm(kd, p)
        if d is None:
            continue
        kept[kd] += 1; xyz.append(p); kind.append(kd); dist.append(d)
    meta = dict(seed=SEED, rows_filtered_angles=ANGLE_CHUNKS * CHUNK, rows_filtered_trig=TRIG_CHUNKS * CHUNK, angle_band_f64_ulps=ANGLE_BAND, trig_band_abs=TRIG_BAND,
                assumed_library_error_f64_ulps=2.0, assumption="no error table for the device library's float64 atan2 / acos is installed with the ROCm documentation; 2 ulp assumed, "
                "the bands' lower edges are twice that (angles) and three times the algebraic form's 2.1e-15 bound (sines / cosines)", kinds=KINDS, count_per_kind=kept,
                dist_unit="float64 ulps of the exact value for kinds 0, 1; absolute for kinds 2 .. 5")
    return dict(hard_xyz=np.array(xyz, F32).reshape(-1, 3), hard_kind=np.array(kind, np.uint8), hard_dist=np.array(dist, F64),
                meta=np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8).copy())


def npz_bytes(arrays):
    """An .npz without time stamps: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as zf:
        for name in sorted(arrays):
            b = io.BytesIO(); np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)); zi.external_attr = 0o644 << 16
            zf.writestr(zi, b.getvalue())
    return buf.getvalue()


def load():
    d = np.load(FIXTURE)
    return dict(xyz=d["hard_xyz"], kind=d["hard_kind"], dist=d["hard_dist"], meta=json.loads(bytes(d["meta"]).decode()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    data = npz_bytes(search(a.procs))
    if a.check:
        same = open(FIXTURE, "rb").read() == data
        print("fixture reproduced byte for byte" if same else "fixture DIFFERS")
        sys.exit(0 if same else 1)
    with open(FIXTURE, "wb") as f:
        f.write(data)
    c = load()
    print("wrote %s: %d bytes, per kind %s" % (FIXTURE, len(data), c["meta"]["count_per_kind"]))
