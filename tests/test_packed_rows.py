"""Packed rows (option "packed_rows", LaunchCfg::packed_rows): pred[] and src[] carry each row's voxel word in their spare bits, so the
swap loop gathers bin16[] for run heads only and the voxel split reads one word per position.  Everything touched is an integer
permutation or an integer count, so the layout must not show in a single bit: every case below is solved once with packed_rows = 0 and
once with packed_rows = 1, and the 48 outputs per pair, src[] and -- for single pairs -- the per-voxel counts and row lists are compared
with array_equal (floats by their bit patterns).

Shapes: scan-1 sizes around the wave (64) and tile (2048) boundaries, the flagship grid 75 x 24 and a 4 x 2 grid (three id bits, hundreds of
rows per voxel at these sizes), batches of 1, 3 and 65 pairs (k_exec_flags up to 63 pairs, k_exec_flags_pair from 64), scans built to stress
one path each, a recorded scan whose keyframe has fits for the loop to work on, and a call whose bits do not fit (150 x 48 with 131 073
rows: 18 + 13 + 2 = 33), which packed_rows = 1 refuses."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 2047, 2048, 2049]
GRIDS = [(24, 75), (2, 4)]               # (bins_phi, bins_theta)
RUNLEN = 7


def _cloud(n, seed):
    """n points on the walls of a 16 x 12 x 4 m room around the sensor, noisy: every voxel of a 4 x 2 grid holds a surface."""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-np.pi, np.pi, n); el = rng.uniform(-0.5, 0.5, n)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    with np.errstate(divide="ignore"):
        t = np.minimum.reduce([8.0 / np.abs(d[:, 0]), 6.0 / np.abs(d[:, 1]), 2.0 / np.abs(d[:, 2])])
    return (d * (t + rng.normal(0, 0.01, n))[:, None]).astype(np.float32)


def _moved(a, seed):
    rng = np.random.default_rng(seed + 77)
    return (a + np.float32([0.05, -0.03, 0.01]) + rng.normal(0, 0.005, a.shape)).astype(np.float32)


def _one_voxel(n, seed):
    """every row inside one voxel of the 75 x 24 grid (a patch of 1 degree by 1 degree)"""
    rng = np.random.default_rng(seed)
    az = 0.30 + rng.uniform(0, 0.017, n); el = 0.05 + rng.uniform(0, 0.017, n); r = rng.uniform(4.0, 6.0, n)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32)


def _with_zeros(n, seed):
    """a third of the rows exactly zero, signed zeros mixed in (the zero bucket, kRowZeroBit), the rest a cloud (rows near voxel edges: kRowNearBit)"""
    a = _cloud(n, seed); rng = np.random.default_rng(seed + 1)
    z = rng.choice(n, n // 3, replace=False); a[z] = 0.0; a[z[::3], 1] = -0.0; a[z[::5], 0] = -0.0
    return a


def _descending(n, seed):
    """r strictly descending in the row index: the sorted order is the reverse of the input, heads and long chains dominate the swap loop"""
    a = _cloud(n, seed).astype(np.float64)
    a *= (np.linspace(9.0, 3.0, n) / np.linalg.norm(a, axis=1))[:, None]
    a = a.astype(np.float32)
    r = np.sqrt((a.astype(np.float32) ** 2).sum(1, dtype=np.float32))
    assert (np.diff(r) < 0).all()
    return a


def _long_shift(m, seed):
    """rank(i) = i + 1 (mod m): descending chains of length ~m, beyond the bounded walk -- the pair goes to k_scramble_replay
    (the generator of tests/test_gpu_parity.py::test_rank_sort_and_scramble_corner_cases)"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, m); el = rng.uniform(-0.3, 0.3, m)
    rad = (5.0 + 1e-3 * ((np.arange(m) + 1) % m)).astype(np.float32)
    return np.stack([rad * np.cos(el) * np.cos(ang), rad * np.cos(el) * np.sin(ang), rad * np.sin(el)], 1).astype(np.float32)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


@pytest.fixture(scope="module")
def ctx():
    import icet_amd
    c = icet_amd.Context(0)
    c.set_option("batch_parts", 1)          # one part: the whole batch is one keyframe call, and src[] of all its pairs is in this context
    yield c
    c.close()


def _single(ctx, a, b, P, T, flags=0):
    """one pair through icet_solve with every side table: outputs, src[], per-voxel counts and row lists, the walk flag"""
    n = a.shape[0]
    r = ctx.solve(a, b, RUNLEN, np.zeros(6), P, T, aux="full", flags=flags)
    out = dict(X=r["X"], pred_stds=r["pred_stds"], cov=r["cov"], src=ctx.debug_fetch("src", n), flags=ctx.debug_fetch("flags", 1))
    for k in ("n1_raw", "cluster_bounds", "has_fit", "mu1", "sigma1", "point_index1", "bin_start1", "points1_spherical", "n2_raw", "n2_in", "x_hist"):
        out[k] = r["aux"][k]
    return out


def _batch(ctx, s1, s2, P, T):
    r = ctx.solve_batch(s1, s2, RUNLEN, None, P, T)
    out = dict(r)
    out["src"] = ctx.debug_fetch("src", sum(s.shape[0] for s in s1))
    out["flags"] = ctx.debug_fetch("flags", len(s1))
    return out


def _same(x, y):
    assert x.keys() == y.keys()
    for k in x:
        assert np.array_equal(_bits(x[k]), _bits(y[k])), k


def _packed_vs_plain(ctx, run, **opts):
    """run() with packed_rows = 0, then with packed_rows = 1 (and opts); the context's options are put back"""
    try:
        ctx.set_option("packed_rows", 0)
        plain = run()
        ctx.set_option("packed_rows", 1)
        for k, v in opts.items():
            ctx.set_option(k, v)
        packed = run()
    finally:
        ctx.set_option("packed_rows", -1)
        for k in opts:
            ctx.set_option(k, -1)
    _same(plain, packed)
    return plain


@pytest.mark.parametrize("P,T", GRIDS)
@pytest.mark.parametrize("n", SIZES)
def test_single_pair_sizes(ctx, n, P, T):
    a = _cloud(n, 100 + n); b = _moved(a, n)
    r = _packed_vs_plain(ctx, lambda: _single(ctx, a, b, P, T))
    assert np.array_equal(np.sort(r["src"]), np.arange(n))                   # unpacked rows come out of debug_fetch: a permutation
    assert int(r["n1_raw"].sum()) == n


@pytest.mark.parametrize("lds_rank", [0, 1])
@pytest.mark.parametrize("P,T", GRIDS)
@pytest.mark.parametrize("k", [1, 3, 65])
def test_ragged_batches(ctx, k, P, T, lds_rank):
    """ragged batches mixing every size; lds_rank on and off under packed_rows = 1 against the plain layout with the default"""
    sizes = [SIZES[(3 * j + 6) % len(SIZES)] for j in range(k)]
    s1 = [_cloud(n, 200 + j) for j, n in enumerate(sizes)]; s2 = [_moved(a, j) for j, a in enumerate(s1)]
    _packed_vs_plain(ctx, lambda: _batch(ctx, s1, s2, P, T), lds_rank=lds_rank)


SPECIAL = {"one_voxel": lambda: _one_voxel(2049, 5), "zeros": lambda: _with_zeros(2500, 6), "descending": lambda: _descending(2049, 7),
           "long_shift": lambda: _long_shift(20000, 8)}


@pytest.mark.parametrize("lds_rank", [0, 1])
@pytest.mark.parametrize("name", sorted(SPECIAL))
def test_special_scans_single(ctx, name, lds_rank):
    a = SPECIAL[name](); b = _moved(a, 9)
    r = _packed_vs_plain(ctx, lambda: _single(ctx, a, b, 24, 75), lds_rank=lds_rank)
    if name == "one_voxel":
        assert (r["n1_raw"] > 0).sum() == 1
    if name == "zeros":
        assert (np.abs(a).max(1) == 0).sum() == 2500 // 3
    if name == "long_shift":
        assert r["flags"][0] & 1                                             # the bounded walk overflowed: k_scramble_replay wrote src[]


@pytest.mark.parametrize("pairwise", [0, 1])
def test_special_scans_in_a_batch(ctx, pairwise):
    """the special scans among ordinary ones, 65 pairs, with the exec bits from the chain walks and from the per-pair recurrence"""
    names = sorted(SPECIAL)
    s1 = [SPECIAL[names[j % 8]]() if j % 8 < len(names) else _cloud(SIZES[j % len(SIZES)], 300 + j) for j in range(65)]
    s2 = [_moved(a, j) for j, a in enumerate(s1)]
    r = _packed_vs_plain(ctx, lambda: _batch(ctx, s1, s2, 24, 75), exec_pairwise=pairwise)
    assert all(r["flags"][j] & 1 for j in range(65) if j % 8 == names.index("long_shift"))


@pytest.mark.parametrize("lds_rank", [0, 1])
def test_real_scan(ctx, frames, lds_rank):
    """a recorded 64-ring scan (thousands of exact-zero rows, 86 fitted voxels): every kernel behind the voxel split has something to do"""
    a, b = frames
    r = _packed_vs_plain(ctx, lambda: _single(ctx, a, b, 24, 75), lds_rank=lds_rank)
    assert r["has_fit"].sum() > 0 and np.abs(r["X"]).max() > 0


def test_true_sort_path(ctx):
    """ICET_FLAG_TRUE_SORT: src[] is the sorted order, packed by k_bin_hist"""
    from icet_amd import api
    a = _with_zeros(2049, 11); b = _moved(a, 12)
    _packed_vs_plain(ctx, lambda: _single(ctx, a, b, 2, 4, flags=api.FLAG_TRUE_SORT))


def test_bits_that_do_not_fit(ctx):
    """150 x 48 with 131 073 rows: 18 + 13 + 2 bits.  packed_rows = 1 is refused; the automatic setting runs the plain layout."""
    import icet_amd
    from icet_amd import api
    n = 131073
    a = _cloud(n, 13); b = _moved(a[:20000], 14)
    try:
        ctx.set_option("packed_rows", 0)
        plain = _single(ctx, a, b, 48, 150)
        ctx.set_option("packed_rows", -1)
        auto = _single(ctx, a, b, 48, 150)
        ctx.set_option("packed_rows", 1)
        with pytest.raises(icet_amd.IcetError) as e:
            ctx.solve(a, b, RUNLEN, np.zeros(6), 48, 150)
        assert e.value.status == api.ICET_ERR_UNSUPPORTED
        # one row fewer, or the flagship grid: fits (17 + 13 + 2 and 18 + 11 + 2)
        fit_rows = _single(ctx, a[:n - 1], b, 48, 150)
        fit_grid = _single(ctx, a, b, 24, 75)
        ctx.set_option("packed_rows", 0)
        _same(fit_rows, _single(ctx, a[:n - 1], b, 48, 150))
        _same(fit_grid, _single(ctx, a, b, 24, 75))
    finally:
        ctx.set_option("packed_rows", -1)
    _same(plain, auto)
