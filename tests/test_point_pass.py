"""The point pass (icet_amd/csrc/icet_accumulate.hip) held to an exact reference, voxel by voxel and word by word: the raw accumulator records
(icet_debug_point_sums_device) against tests/point_pass_model.py -- counts exactly, the nine fixed-point sums within
    8 u sum |terms| + m 2^-37,   u = 2^-24
(derived in the model's docstring: float partial sums of at most 7 terms, one rounding to the 2^-36 grid per flush) -- for every stream order, length,
layout and launch shape that takes another path through the kernel; and the float -> fixed-point conversions on their own (icet_debug_fix) against
Python's exact round-half-even.  The CPU tests check the model against the oracle's trace and the bound against the model alone."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import point_pass_model as pm

GRID = dict(bins_phi=24, bins_theta=75, n=10, thresh=0.3, buff=0.3)          # (32 rings x 1024 steps are a quarter of a full scan: with these, ~350 voxels are active)
COARSE = dict(bins_phi=2, bins_theta=4, n=25, thresh=4.0, buff=8.0)
WALL = dict(bins_phi=24, bins_theta=75, n=25, thresh=0.5, buff=4.0)


# ---- the cases: (scan 1, scan 2, grid), shared by the CPU and the GPU tests ------------------------------------------------------------

def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy().T)


@functools.lru_cache(maxsize=None)
def _synthetic(seed=0, steps=1024):
    from icet_amd import lidar_sim as ls
    s1, s2, xt = ls.make_pair(scene_seed=3000 + seed, noise_seed=3100 + seed, rings=32, steps=steps)
    return _np(s1), _np(s2), xt


def _move(scan, X):
    """Scan 2 moved on the host: the device's own float32 transform, so that the pass at X = 0 sees exactly these rows."""
    return pm.transform(scan, np.asarray(X, np.float32))


def _wall(offset, seed):
    """A planar wall x = 80 + offset m seen through 16 rings x 1024 steps (ring-major), 1 cm of range noise: thin voxels at long range."""
    rng = np.random.default_rng(seed)
    az = np.deg2rad(np.linspace(-24.9, 24.9, 1024) + 0.2); el = np.deg2rad(np.linspace(-5.0, 8.0, 16) + 0.2)
    E, A = np.meshgrid(el, az, indexing="ij")
    r = (80.0 + offset) / (np.cos(E) * np.cos(A)) + rng.normal(0.0, 0.01, E.shape)
    return np.stack([r * np.cos(E) * np.cos(A), r * np.cos(E) * np.sin(A), r * np.sin(E)], -1).reshape(-1, 3).astype(np.float32)


def _ring(seed):
    """A closed wall at 260 m (+- 1.5 m, three lobes; 5 cm of range noise) seen through 16 rings x 1024 steps, ring-major: on a 2 x 4 grid each of the 8
    voxels holds ~2048 points spread over a 90-degree arc, |d| from centimetres to 190 m."""
    rng = np.random.default_rng(seed)
    az = np.deg2rad(np.arange(1024) * (360.0 / 1024) + 0.2); el = np.deg2rad(np.linspace(-10.0, 10.0, 16) + 0.2)
    E, A = np.meshgrid(el, az, indexing="ij")
    r = 260.0 + 1.5 * np.sin(3.0 * A) + rng.normal(0.0, 0.05, E.shape)
    return np.stack([r * np.cos(E) * np.cos(A), r * np.cos(E) * np.sin(A), r * np.sin(E)], -1).reshape(-1, 3).astype(np.float32)


def _hostile(b):
    """Scan 2 salted with exact-zero rows of every sign pattern, NaN / inf rows and 1e18 magnitudes (every 37th row)."""
    o = b.copy()
    idx = np.arange(5, o.shape[0], 37)
    signs = [(sx, sy, sz) for sx in (0.0, -0.0) for sy in (0.0, -0.0) for sz in (0.0, -0.0)]
    rows = signs + [(np.nan, 1.0, 2.0), (1.0, np.nan, 2.0), (np.nan, np.nan, np.nan), (np.inf, 1.0, 2.0), (1.0, -np.inf, 2.0), (1.0, 2.0, np.inf),
                    (1e18, 1.0, 2.0), (-1e18, 1e18, 2.0), (3.0, 2.0, -1e18), (1e18, 1e18, 1e18)]
    for k, i in enumerate(idx):
        o[i] = rows[k % len(rows)]
    return o


@functools.lru_cache(maxsize=None)
def _case(name):
    """name -> (scan 1, scan 2 at X = 0, grid keywords)."""
    a, b, xt = _synthetic()
    if name == "synthetic":
        return a, _move(b, xt), GRID                                           # scan 2 moved onto scan 1 by the true motion: ~every active voxel fills
    if name == "hostile":
        return a, _hostile(_move(b, xt)), GRID
    if name.startswith("coarse"):                                              # 90-degree voxels at 255-265 m; scan 2 translated by (off, 0.3 off, 0.1 off) m
        off = float(name[6:] or 0.0)
        return _ring(21), _move(_ring(22), [off, 0.3 * off, 0.1 * off, 0, 0, 0]), COARSE
    if name.startswith("wall"):
        return _wall(0.0, 11), _wall(float(name[4:]), 12), WALL
    raise KeyError(name)


SUM_CASES = ("synthetic", "hostile", "coarse", "coarse1", "coarse3", "wall0.5", "wall1", "wall2", "wall3")


@functools.lru_cache(maxsize=None)
def _oracle_kf(name):
    from oracle import pyoracle as po
    a, b, g = _case(name)
    tr = po.solve(a, b, runlen=1, trace=True, mode=po.DEVICE_ARITH, **g)["trace"]
    return pm.keyframe_tables(tr, g["n"]), tr


@functools.lru_cache(maxsize=None)
def _oracle_ref(name):
    a, b, g = _case(name)
    return pm.reference(b, _oracle_kf(name)[0], g["bins_phi"], g["bins_theta"])


# ---- CPU: the model against the oracle's trace, the bound against the model ---------------------------------------------------------------

def _check_against_trace(ref, kf, tr, n):
    act = kf["active"]
    assert act.sum() > 0
    assert np.array_equal(ref.n2[act], tr["n2_raw"][0][act])
    gate = act & (tr["n2_raw"][0] > n)                                         # (the trace's n2_in is 0 where the voxel was gated off before the filter)
    assert np.array_equal(ref.m[gate], tr["n2_in"][0][gate])
    used = np.nonzero(tr["used"][0])[0]
    assert used.size > 0
    for v in used:
        m = int(ref.m[v])
        mu2, cov = pm.moments(ref.S[v], m, kf["mu1"][v])
        got_mu = tr["mu2"][0][v]; got_c = tr["sigma2"][0][v]
        for k in range(3):                                                     # float rounding: one ulp of the float32 result (the trace sums in double, rounds once)
            assert abs(Fraction(float(got_mu[k])) - mu2[k]) <= float(np.spacing(np.abs(got_mu[k]))) + 2.0 ** -45 * float(ref.A[v][k]) / m, (v, k)
        for q, (i, j) in enumerate(pm.PAIRS):
            tol = float(np.spacing(np.abs(got_c[i, j]))) + 2.0 ** -40 * float(ref.A[v][3 + q]) / (m - 1)      # + the double sums' own rounding, amplified by the cancellation
            assert abs(Fraction(float(got_c[i, j])) - cov[q]) <= tol, (v, q, float(got_c[i, j]), float(cov[q]))


def test_model_matches_the_oracle_trace_on_the_golden_frames(frames):
    from oracle import pyoracle as po
    a, b = frames
    tr = po.solve(a, b, runlen=1, trace=True, mode=po.DEVICE_ARITH)["trace"]
    kf = pm.keyframe_tables(tr)
    _check_against_trace(pm.reference(b, kf, 24, 75), kf, tr, 25)


def test_model_matches_the_oracle_trace_at_a_nonzero_pose():
    """X != 0: the model's float32 transform gives the trace's counts; and scan 2 moved on the host by that transform gives, at X = 0, the trace's moments."""
    from oracle import pyoracle as po
    a, b, xt = _synthetic()
    tr = po.solve(a, b, x0=xt, runlen=1, trace=True, mode=po.DEVICE_ARITH, **GRID)["trace"]
    kf = pm.keyframe_tables(tr, GRID["n"])
    cnt = pm.reference(b, kf, 24, 75, X=xt, sums=False)
    act = kf["active"]
    assert np.array_equal(cnt.n2[act], tr["n2_raw"][0][act])
    gate = act & (tr["n2_raw"][0] > GRID["n"])
    assert np.array_equal(cnt.m[gate], tr["n2_in"][0][gate]) and int(cnt.m.sum()) > 10000
    _check_against_trace(pm.reference(_move(b, xt), kf, 24, 75), kf, tr, GRID["n"])


def test_fma32_is_a_single_rounding():
    rng = np.random.default_rng(3)
    a = rng.normal(size=3000).astype(np.float32); b = rng.normal(size=3000).astype(np.float32); c = (rng.normal(size=3000) * 10.0 ** rng.integers(-6, 3, 3000)).astype(np.float32)
    got = pm.fma32(a, b, c)
    for x, y, z, r in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        lo, hi = np.nextafter(np.float32(r), np.float32(-np.inf)), np.nextafter(np.float32(r), np.float32(np.inf))
        assert abs(exact - Fraction(r)) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi))))
    # the case a float64 detour gets wrong: c = 1 + 2^-23 (odd mantissa), a b = 2^-24 (1 - 2^-46).  The float64 sum is exactly c + half an ulp, a tie that goes
    # UP to the even neighbour; the true sum lies below the tie and rounds DOWN to c.
    x = np.float32(1.0) + np.float32(2.0 ** -23)
    a1 = np.float32(2.0 ** -12) * (np.float32(1.0) + np.float32(2.0 ** -23)); b1 = np.float32(2.0 ** -12) * (np.float32(1.0) - np.float32(2.0 ** -23))
    assert np.float32(np.float64(a1) * np.float64(b1) + np.float64(x)) != x    # (the detour)
    assert pm.fma32(np.float32([a1, -a1]), np.float32([b1, b1]), np.float32([x, -x])).tolist() == [float(x), -float(x)]


@pytest.mark.parametrize("name", SUM_CASES)
def test_float_partial_sums_of_up_to_seven_terms_stay_inside_the_bound(name):
    """The bound against the reference alone: float32 partial sums over random groups of <= 7 points, each rounded to the 2^-36 grid (NumPy emulation of the
    device's arithmetic), stay within 8 u sum |terms| + m 2^-37 of the exact sums on every case the GPU tests use."""
    ref = _oracle_ref(name)
    rng = np.random.default_rng(17)
    assert len(ref.S) > 0
    worst = 0.0
    for v, d in ref.d.items():
        words = pm.emulate_words(d, rng)
        for k in range(9):
            err = abs(Fraction(words[k], 1 << pm.FIX_BITS) - ref.S[v][k]); bnd = ref.bound(v, k)
            worst = max(worst, float(err / bnd))
            assert err <= bnd, (name, v, k, float(err), float(bnd))
    print("%s: emulated partial sums reach %.3f of the bound over %d voxels" % (name, worst, len(ref.d)))


def test_the_comparison_catches_a_lost_run_and_a_wrong_bias_count():
    """The checker itself: records built from the emulation pass; one suffix point lost from one sum, or one conversion bias too many in one word, fails."""
    from icet_amd import api
    ref = _oracle_ref("synthetic")
    rng = np.random.default_rng(5)
    rec = np.zeros(ref.V, api.POINT_SUMS_DTYPE)
    rec["n2"] = ref.n2; rec["m"] = ref.m
    for v, d in ref.d.items():
        rec["sums"][v] = pm.emulate_words(d, rng)
    bad, worst = pm.compare(rec, ref)
    assert not bad and 0.0 < worst <= 1.0
    v = max(ref.d, key=lambda u: ref.m[u])
    lost = rec.copy(); lost["sums"][v][0] -= pm.fix_of(ref.d[v][np.abs(ref.d[v][:, 0]).argmax(), 0])      # one point's dx missing from sum dx
    assert any("voxel %d word 0" % v in s for s in pm.compare(lost, ref)[0])
    w = (int(rec["sums"][v][8]) + pm.FIX_BIAS) % (1 << 64)                    # one conversion bias left in (mod 2^64, as a two's-complement word)
    biased = rec.copy(); biased["sums"][v][8] = w - (1 << 64) if w >= (1 << 63) else w
    assert any("voxel %d word 8" % v in s for s in pm.compare(biased, ref)[0])
    cnt = rec.copy(); cnt["m"][v] += 1
    assert any("counts" in s for s in pm.compare(cnt, ref)[0])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------

def _params(g, runlen=1, flags=0):
    from icet_amd import api
    return api.Params(runlen, g["bins_phi"], g["bins_theta"], g["n"], g["thresh"], g["buff"], flags)


class _DeviceRefs:
    """Per case the exact reference on the keyframe tables the DEVICE built: computed once per module, shared by the tests, never modified."""

    def __init__(self, ctx):
        self.ctx = ctx; self._kf = {}; self._ref = {}

    def kf(self, key, a, g):
        """The keyframe tables of scan 1 from the aux output of a one-iteration solve."""
        if key not in self._kf:
            ax = self.ctx.solve(a, a[:1024], 1, np.zeros(6), g["bins_phi"], g["bins_theta"], g["n"], g["thresh"], g["buff"], aux=True)["aux"]
            self._kf[key] = pm.keyframe_tables(ax, g["n"])
        return self._kf[key]

    def __call__(self, name):
        """Case `name` -> (scan 1, scan 2, grid, keyframe tables, reference)."""
        if name not in self._ref:
            a, b, g = _case(name)
            kf = self.kf(name, a, g)
            self._ref[name] = (a, b, g, kf, pm.reference(b, kf, g["bins_phi"], g["bins_theta"]))
        return self._ref[name]


@pytest.fixture(scope="module")
def device_ref(gpu_ctx):
    return _DeviceRefs(gpu_ctx)


def _scan_dev(rows, ld=None, shift=0):
    """N x 3 rows -> (device tensor that owns the memory, descriptor (ptr, n, ld)): x | y | z at leading dimension ld (default: n rounded up to 4, + 4: ld > n),
    the padding NaN; shift: the scan starts `shift` floats into the allocation."""
    n = rows.shape[0]
    ld = ((n + 3) // 4 * 4 + 4) if ld is None else ld
    buf = np.full(3 * ld + shift + 4, np.nan, np.float32)
    for k in range(3):
        buf[shift + k * ld: shift + k * ld + n] = rows[:, k]
    t = torch.from_numpy(buf).to("cuda:0")
    return t, (t.data_ptr() + 4 * shift, n, ld)


def _dump(ctx, kf_scans, g, kf_index, scans2, layout=None):
    """Park the keyframes, run ONE point pass of every scan 2 at X = 0 and return the records (n_regs, V) of POINT_SUMS_DTYPE."""
    kf = [_scan_dev(s) for s in kf_scans]
    ctx.keyframe_device([d for _, d in kf], _params(g))
    return _dump_parked(ctx, g, kf_index, scans2, layout)


def _dump_parked(ctx, g, kf_index, scans2, layout=None):
    from icet_amd import api
    prm = _params(g)
    V = g["bins_phi"] * g["bins_theta"]
    s2 = [_scan_dev(s, **(layout or {})) for s in scans2]
    k = len(s2)
    X = torch.zeros((k, 6), dtype=torch.float32, device="cuda:0")
    out = torch.full((k, V, 20), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.debug_point_sums(kf_index, [d for _, d in s2], prm, X.data_ptr(), out.data_ptr())
    ctx.sync()
    return np.frombuffer(out.cpu().numpy().tobytes(), api.POINT_SUMS_DTYPE).reshape(k, V)


def _hold(rec, ref, label):
    bad, worst = pm.compare(rec, ref, label)
    print("%s: worst |error| / bound = %.3f over %d voxels with points" % (label, worst, len(ref.S)))
    assert not bad, "%d failures, first: %s" % (len(bad), bad[:6])
    return worst


@pytest.mark.gpu
def test_conversions_round_half_even_and_agree(gpu_ctx):
    """to_fix_biased, to_fix_wide_biased and to_fix against Python's exact round-half-even of v * 2^36 (+ kFixBias where biased)."""
    rng = np.random.default_rng(1)
    t = 2.0 ** -36
    ties = [(k + 0.5) * t for k in (0, 1, 2, 3, 100, 101, 2 ** 20, 2 ** 20 + 1)]
    vals = [0.0, -0.0, 2.0 ** -37, -2.0 ** -37, 1.5 * t, -1.5 * t, 2.5 * t, -2.5 * t, 0.5 * t, np.nextafter(np.float32(0.5 * t), np.float32(1)), np.nextafter(np.float32(0.5 * t), np.float32(0)),
            1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, 2.0 ** -126, 2.0 ** -60, 1.0, -1.0, 1.0 + 2.0 ** -23, 0.1, -0.1, 1234.5678, -1234.5678, 2.0 ** 26, -2.0 ** 26, 2.0 ** 26 + 8.0, 1e5, -1e5, 65536.0 + 2.0 ** -7]
    vals += ties + [-x for x in ties]
    for p in (14, 15):
        e = np.float32(2.0 ** p)
        vals += [np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(np.inf)), -np.nextafter(e, np.float32(0)), -e, -np.nextafter(e, np.float32(np.inf))]
    vals += list(rng.normal(size=400) * 10.0 ** rng.uniform(-12, 4, 400)) + list(rng.uniform(-32768, 32768, 200)) + list(rng.uniform(-2.0 ** 26, 2.0 ** 26, 200))
    v = np.asarray(vals, np.float32)
    got = gpu_ctx.debug_fix(v)
    M = 1 << 64
    for x, (b, w, u) in zip(v.tolist(), got.tolist()):
        want = pm.fix_of(x)
        assert int(w) == (want + pm.FIX_BIAS) % M, (x, "wide", int(w), want)
        assert int(u) == want % M, (x, "unbiased", int(u), want)
        if abs(x) < 32768.0:                                                   # where the two-instruction form is defined: the same word, ties included
            assert int(b) == (want + pm.FIX_BIAS) % M and int(b) == int(w), (x, "biased", int(b), want)
    fast = np.abs(v) < 32768.0
    n = int(fast.sum())
    total = sum(int(b) for b in got[fast, 0].tolist()) % M
    assert (total - n * pm.FIX_BIAS) % M == sum(pm.fix_of(x) for x in v[fast].tolist()) % M      # n biased words - n bias = the sum of the integers


@pytest.mark.gpu
def test_ring_major_and_shuffled_streams_against_one_reference(device_ref):
    """The same scan-2 point set ring-major (long runs, suffix runs handed from lane to lane) and in a seeded random order (runs of one, nothing handed on)."""
    import icet_amd
    a, b, g, kf, ref = device_ref("synthetic")
    assert int((ref.m > 0).sum()) > 100 and int(ref.m.sum()) > 10000
    perm = np.random.default_rng(5).permutation(b.shape[0])
    ctx = icet_amd.Context(0)
    rec = _dump(ctx, [a], g, [0, 0], [b, b[perm]])
    ctx.close()
    _hold(rec[0], ref, "ring-major")
    _hold(rec[1], ref, "shuffled")


def _two_busy_voxels(b, kf, ref, g, need):
    vox, inb = pm.membership(pm.transform(b), kf, g["bins_phi"], g["bins_theta"])
    busy = [int(v) for v in np.argsort(-ref.m)[:2]]
    assert ref.m[busy[1]] >= need
    return [b[np.nonzero((vox == v) & inb)[0][:need]] for v in busy]


@pytest.mark.gpu
def test_two_voxels_alternating_with_periods_1_to_7(device_ref):
    """Runs of length p of two voxels in turn, p = 1, 2, 3, 4, 5, 7: the A / Z / middle-run branches of phase C, all against the one reference of the point set."""
    import icet_amd
    a, b, g, kf, _ = device_ref("synthetic")
    pa, pb = _two_busy_voxels(b, kf, device_ref("synthetic")[4], g, 84)
    streams = []
    for p in (1, 2, 3, 4, 5, 7):
        streams.append(np.concatenate([np.concatenate([pa[i:i + p], pb[i:i + p]]) for i in range(0, 84, p)]))
    ref = pm.reference(streams[0], kf, g["bins_phi"], g["bins_theta"])
    assert sorted(ref.m[ref.m > 0].tolist()) == [84, 84]
    ctx = icet_amd.Context(0)
    rec = _dump(ctx, [a], g, [0] * 6, streams)
    ctx.close()
    for k, p in enumerate((1, 2, 3, 4, 5, 7)):
        _hold(rec[k], ref, "period %d" % p)


@pytest.mark.gpu
def test_a_stretch_shifted_across_group_lane_and_block_boundaries(device_ref):
    """One voxel's points as a contiguous stretch of 90 rows behind 0..7 and 250..257 filler rows of another voxel: its runs cross the group-of-4, the lane-63
    and the aligned-256 boundaries at every phase."""
    import icet_amd
    a, b, g, kf, _ = device_ref("synthetic")
    pa, pb = _two_busy_voxels(b, kf, device_ref("synthetic")[4], g, 90)
    streams, refs = [], []
    for base in (0, 250):
        for s in range(8):
            fill = np.repeat(pb[:1], base + s, 0)
            streams.append(np.concatenate([fill, pa, np.repeat(pb[1:2], 9, 0)]))
            refs.append(pm.reference(streams[-1], kf, g["bins_phi"], g["bins_theta"]))
    ctx = icet_amd.Context(0)
    rec = _dump(ctx, [a], g, [0] * len(streams), streams)
    ctx.close()
    for k, ref in enumerate(refs):
        assert 90 in ref.m.tolist() and int((ref.m > 0).sum()) == 2
        _hold(rec[k], ref, "stretch behind %d filler rows" % (250 * (k // 8) + k % 8))


LENGTHS = (1, 3, 4, 5, 255, 256, 257, 2047, 2049)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["vec4", "odd_ld", "pointer_off_by_one_float"])
def test_lengths_and_layouts(device_ref, layout):
    """Prefixes of n2 rows, ld > n2; with an odd ld or a pointer one float off the 16-byte grid the scalar-load form of the kernel runs (kVec4 false)."""
    import icet_amd
    a, b, g, kf, _ = device_ref("synthetic")
    start = int(np.nonzero(pm.membership(pm.transform(b), kf, g["bins_phi"], g["bins_theta"])[1])[0][0])      # begin at an in-bounds row: even n2 = 1 carries a sum
    scans = [b[start:start + n] for n in LENGTHS]
    refs = [pm.reference(s, kf, g["bins_phi"], g["bins_theta"]) for s in scans]
    assert all(int(r.m.sum()) > 0 for r in refs)
    lay = {"vec4": None, "odd_ld": dict(ld=2053), "pointer_off_by_one_float": dict(ld=2056, shift=1)}[layout]
    ctx = icet_amd.Context(0)
    rec = _dump(ctx, [a], g, [0] * len(scans), scans, lay)
    ctx.close()
    for k, n in enumerate(LENGTHS):
        _hold(rec[k], refs[k], "%s n2 = %d" % (layout, n))


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["lds_slots=32", "acc_blocks=7,acc_pts=4", "guard_scale=16", "force_exact=1"])
def test_launch_shapes_against_the_same_reference(device_ref, knob):
    """lds_slots 32: the HBM spill path (more than 32 active voxels); acc_blocks / acc_pts: several blocks per pair -- the global combination and the per-block
    bias removal; guard_scale 16: the LDS near queue; force_exact: every point parked, the overflow list drained by the dump kernel."""
    import icet_amd
    a, b, g, kf, ref = device_ref("synthetic")
    assert int(kf["active"].sum()) > 32
    perm = np.random.default_rng(6).permutation(b.shape[0])
    ctx = icet_amd.Context(0)
    for kv in knob.split(","):
        k, v = kv.split("=")
        ctx.set_option(k, float(v))
    rec = _dump(ctx, [a], g, [0, 0], [b, b[perm]])
    ctx.close()
    _hold(rec[0], ref, knob + " ring-major")
    _hold(rec[1], ref, knob + " shuffled")


@pytest.mark.gpu
def test_one_registration_against_forty_with_two_keyframes(device_ref):
    """n_regs 1 (the small-batch instantiation) against n_regs 40 (the throughput instantiation) of the same scans, two keyframes, kf_index not the identity:
    every copy is identical, and each matches its keyframe's reference."""
    import icet_amd
    a, b, g, kf, ref = device_ref("synthetic")
    a1, b1, xt1 = _synthetic(1, 512)
    b1 = _move(b1, xt1)
    kf1 = device_ref.kf("synthetic1", a1, g)
    ref1 = pm.reference(b1, kf1, g["bins_phi"], g["bins_theta"])
    assert int(ref1.m.sum()) > 3000
    kf_index = [1, 0, 0, 1, 1] * 8                                            # 40 registrations
    ctx = icet_amd.Context(0)
    many = _dump(ctx, [a, a1], g, kf_index, [b1 if k else b for k in kf_index])
    one1 = _dump_parked(ctx, g, [1], [b1])
    one0 = _dump_parked(ctx, g, [0], [b])
    ctx.close()
    _hold(one0[0], ref, "1 registration, keyframe 0"); _hold(one1[0], ref1, "1 registration, keyframe 1")
    first = {0: kf_index.index(0), 1: kf_index.index(1)}
    _hold(many[first[0]], ref, "40 registrations, keyframe 0"); _hold(many[first[1]], ref1, "40 registrations, keyframe 1")
    for r, k in enumerate(kf_index):
        assert many[r].tobytes() == many[first[k]].tobytes(), r


@pytest.mark.gpu
def test_coarse_grid_long_range_takes_the_wide_conversion(device_ref):
    """90-degree voxels at 260 m, ~2048 points each: single points with d^2 beyond 2^14 m^2 (their flush takes flush_wide whatever the grouping) next to
    points whose runs stay below it whatever the grouping."""
    import icet_amd
    a, b, g, kf, ref = device_ref("coarse")
    assert max(float(S[3]) for S in ref.S.values()) > 2.0 ** 14 and max(float(S[6]) for S in ref.S.values()) > 2.0 ** 14      # the reference's sum d^2, per voxel
    d2 = np.concatenate([np.square(d.astype(np.float64)).max(1) for d in ref.d.values()])
    assert (d2 > 2.0 ** 14).any() and (7 * d2 < 2.0 ** 14).any()                 # single points beyond the fast range, and runs that stay inside it whatever their grouping
    ctx = icet_amd.Context(0)
    rec = _dump(ctx, [a], g, [0, 0], [b, b[np.random.default_rng(8).permutation(b.shape[0])]])
    ctx.close()
    _hold(rec[0], ref, "coarse ring-major"); _hold(rec[1], ref, "coarse shuffled")


@pytest.mark.gpu
def test_hostile_rows_count_exactly_and_leave_the_sums_alone(device_ref):
    """Exact-zero rows of every sign pattern, NaN / inf rows, 1e18 magnitudes among ordinary rows: every count as the reference's, every sum inside the bound --
    and, the hostile rows never being in bounds, m and the exact sums are those of the ordinary rows."""
    import icet_amd
    a, b, g, kf, ref = device_ref("hostile")
    clean = device_ref("synthetic")[4]
    kept = np.ones(b.shape[0], bool); kept[np.arange(5, b.shape[0], 37)] = False
    only = pm.reference(b[kept], kf, g["bins_phi"], g["bins_theta"])
    assert np.array_equal(ref.m, only.m) and all(ref.S[v] == only.S[v] for v in only.S) and int(ref.n2.sum()) >= int(only.n2.sum())
    assert int(ref.m.sum()) < int(clean.m.sum())
    ctx = icet_amd.Context(0)
    rec = _dump(ctx, [a], g, [0, 0], [b, b[np.random.default_rng(9).permutation(b.shape[0])]])
    ctx.close()
    _hold(rec[0], ref, "hostile ring-major"); _hold(rec[1], ref, "hostile shuffled")


def _lambda_min_error(rec, ref, kf, g_n):
    """Worst relative error of cov2's smallest eigenvalue (device sums against exact sums, same formulas), over the voxels a solve would use (m > n)."""
    worst = (0.0, -1, 0.0)
    for v in ref.S:
        m = int(ref.m[v])
        if m <= g_n:
            continue
        dev = [Fraction(int(w), 1 << pm.FIX_BITS) for w in rec["sums"][v]]
        ce = pm.sym3([float(c) for c in pm.moments(ref.S[v], m, kf["mu1"][v])[1]]); cd = pm.sym3([float(c) for c in pm.moments(dev, m, kf["mu1"][v])[1]])
        le, ld = np.linalg.eigvalsh(ce)[0], np.linalg.eigvalsh(cd)[0]
        rel = abs(ld - le) / abs(le)
        if rel > worst[0]:
            db = np.array([float(ref.S[v][k]) / m for k in range(3)])
            worst = (float(rel), v, float(np.linalg.norm(db)))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["coarse1", "coarse3", "wall0.5", "wall1", "wall2", "wall3"])
def test_large_offsets_between_the_means_keep_the_bound(device_ref, name):
    """Scan 2 moved so that |mu2 - mu1| reaches metres inside long-range voxels (coarse grid; a planar wall at 80 m: thin voxels).  The bound holds as everywhere
    else; the relative error of cov2's smallest eigenvalue is printed, not asserted (LABNOTES)."""
    import icet_amd
    a, b, g, kf, ref = device_ref(name)
    off = max(float(np.linalg.norm([float(ref.S[v][k]) / int(ref.m[v]) for k in range(3)])) for v in ref.S if ref.m[v] > 25)
    assert off > 0.4 * float(name.replace("coarse", "").replace("wall", ""))   # |mu2 - mu1| does reach the offset asked for
    ctx = icet_amd.Context(0)
    rec = _dump(ctx, [a], g, [0], [b])
    ctx.close()
    _hold(rec[0], ref, name)
    rel, v, dist = _lambda_min_error(rec[0], ref, kf, g["n"])
    print("%s: largest |mu2 - mu1| %.2f m; worst relative error of cov2's smallest eigenvalue %.3g (voxel %d, |mu2 - mu1| = %.2f m)" % (name, off, rel, v, dist))


@pytest.mark.gpu
def test_a_dump_leaves_the_workspace_as_a_solve_does(device_ref):
    """Two dumps in a row give equal records (the accumulators and the overflow count were left at zero); a registration after a dump gives the bits of a
    fresh context.  force_exact: the overflow list is in use."""
    import icet_amd
    a, b, g, kf, ref = device_ref("synthetic")
    prm = _params(g, runlen=4)
    outs = []
    for dump_first, exact in ((True, 0), (False, 0), (True, 1), (False, 1)):
        ctx = icet_amd.Context(0)
        ctx.set_option("force_exact", exact)
        s1 = _scan_dev(a); s2 = _scan_dev(b)
        ctx.keyframe_device([s1[1]], prm)
        if dump_first:
            r1 = _dump_parked(ctx, g, [0], [b]); r2 = _dump_parked(ctx, g, [0], [b])
            assert r1.tobytes() == r2.tobytes()
            _hold(r1[0], ref, "dump, force_exact %d" % exact)
        out = torch.full((1, 48), float("nan"), dtype=torch.float32, device="cuda:0")
        ctx.register_indexed_device([0], [s2[1]], prm, out.data_ptr())
        ctx.sync()
        outs.append(out.cpu().numpy().copy())
        ctx.close()
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[2].view(np.uint32), outs[3].view(np.uint32))
