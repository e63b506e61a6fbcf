"""The deskewer on the GPU (include/icet_hip.h icet_deskew_*) against the NumPy model of tests/deskew_model.py, BIT FOR BIT: the rows,
the untouched padding, the counts.  Only the twists taken from poses on the device have a tolerance (two math libraries)."""
import ctypes as C

import numpy as np
import pytest
import torch

import deskew_model as dm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = np.array([0xC5A5F00D], np.uint32).view(np.float32)[0]      # what a destination holds before a call: a finite float no rule produces here
SIZES = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)      # lane groups of 4, wave, trip and block boundaries


@pytest.fixture(scope="module")
def dk(gpu_ctx):
    from icet_amd import api
    d = api.Deskewer(gpu_ctx)
    yield d
    d.close()


class Case:
    """One scan of a call: rows, times, the motion, and where its buffers lie (offsets in floats from a 16-byte boundary; pad: ld - n)."""

    def __init__(self, rows, time, twist, mode=dm.TIME_ARRAY, period=0, t0=0.0, inv_span=1.0, ref=1.0, src_off=0, dst_off=0, time_off=0, pad=5, in_place=False):
        self.rows = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 3))
        self.time = None if time is None else np.asarray(time, np.float32).reshape(-1)
        self.twist = np.asarray(twist, np.float64).reshape(6)
        self.kw = dict(mode=mode, period=period, t0=t0, inv_span=inv_span, ref=ref)
        self.src_off, self.dst_off, self.time_off, self.pad, self.in_place = src_off, dst_off, time_off, pad, in_place
        self.n = self.rows.shape[0]; self.ld = self.n + pad

    def model(self):
        return dm.deskew(self.rows, self.twist, self.time, **self.kw)

    def upload(self):
        """src: NaN everywhere but the rows (the padding must not be read); dst: the sentinel everywhere; time: NaN around the n values."""
        n, ld = self.n, self.ld
        h = np.full(self.src_off + 3 * ld + 4, np.nan, np.float32)
        for a in range(3):
            h[self.src_off + a * ld: self.src_off + a * ld + n] = self.rows[:, a]
        self.h_src = h
        self.d_src = torch.from_numpy(h).to(DEV)
        self.d_dst = self.d_src if self.in_place else torch.from_numpy(np.full(self.dst_off + 3 * ld + 4, SENTINEL, np.float32)).to(DEV)
        ht = np.full(self.time_off + n + 4, np.nan, np.float32)
        if self.time is not None:
            ht[self.time_off: self.time_off + n] = self.time
        self.d_time = torch.from_numpy(ht).to(DEV)
        assert self.d_src.data_ptr() % 16 == 0 and self.d_dst.data_ptr() % 16 == 0 and self.d_time.data_ptr() % 16 == 0
        self.dst_off_eff = self.src_off if self.in_place else self.dst_off

    def record(self, twist=None):
        from icet_amd import api
        k = self.kw
        return api.DeskewScan(self.d_src.data_ptr() + 4 * self.src_off, self.n, self.ld, self.d_dst.data_ptr() + 4 * self.dst_off_eff, self.ld,
                              self.d_time.data_ptr() + 4 * self.time_off if self.time is not None else None, k["mode"], k["period"], float(k["t0"]), float(k["inv_span"]),
                              float(k["ref"]), (C.c_double * 6)(*[float(v) for v in (self.twist if twist is None else twist)]))

    def check(self, what=""):
        """The destination against the model: the rows' bits, and every other word as it was."""
        got = self.d_dst.cpu().numpy()
        want, cls = self.model()
        exp = self.h_src.copy() if self.in_place else np.full(got.shape[0], SENTINEL, np.float32)
        for a in range(3):
            exp[self.dst_off_eff + a * self.ld: self.dst_off_eff + a * self.ld + self.n] = want[:, a]
        differ = got.view(np.uint32) != exp.view(np.uint32)
        differ &= ~(np.isnan(got) & np.isnan(exp) & (got.view(np.uint32) != SENTINEL.view(np.uint32)))      # a NaN the arithmetic made (a NaN in rho): its sign and payload are the machine's
        bad = np.nonzero(differ)[0]
        assert bad.size == 0, (what, self.n, self.src_off, self.dst_off, bad[:8], got[bad[:8]], exp[bad[:8]])
        if not self.in_place:
            assert np.array_equal(self.d_src.cpu().numpy().view(np.uint32), self.h_src.view(np.uint32)), what      # the source is only read
        return dm.counts(cls)


def run(ctx, dk, cases, device_twists=False, counts=True, what=""):
    """One call over the cases; everything checked against the model.  device_twists: the twists go through HBM and the records carry zeros instead."""
    for c in cases:
        c.upload()
    cnt = torch.full((max(len(cases), 1), 8), 77, dtype=torch.int64, device=DEV) if counts else None      # (the call zeroes the records itself)
    tw = torch.from_numpy(np.stack([c.twist for c in cases]).reshape(-1, 6)).to(DEV) if device_twists else None
    torch.cuda.synchronize(DEV)
    dk.deskew_device([c.record(np.zeros(6) if device_twists else None) for c in cases], tw, cnt.data_ptr() if counts else None)
    ctx.sync()
    got = cnt.cpu().numpy() if counts else None
    for k, c in enumerate(cases):
        want = c.check("%s scan %d" % (what, k))
        if counts:
            assert dict(zip(dm.CLASS_NAMES, [int(v) for v in got[k, :5]])) == want and (got[k, 5:] == 0).all(), (what, k, got[k], want)
    return got


def _rows(rs, n, spread=(40, 40, 4)):
    r = (rs.randn(n, 3) * spread).astype(np.float32)
    r[::7] = 0.0
    if n > 5:
        r[5, 1] = np.nan; r[3, 0] = np.inf
    return r


def _twist(rs, scale=1.0):
    return np.concatenate([rs.uniform(-2, 2, 3), rs.uniform(-0.3, 0.3, 3)]) * scale


# ---- 1. sizes and alignment ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_off", [0, 1, 2, 3])
def test_sizes_and_alignment(gpu_ctx, dk, src_off):
    """Every size at which the kernel takes another path, source and destination each 0 .. 3 floats off a 16-byte boundary, independently; ld = n + 5 with NaN in
    the source's padding; the destination prefilled: its padding and everything past row n untouched.  All scans of one source offset go in ONE call."""
    rs = np.random.RandomState(100 + src_off)
    cases = []
    for n in SIZES:
        for dst_off in range(4):
            time = rs.uniform(-0.1, 1.1, n).astype(np.float32)
            if n > 9:
                time[9] = np.nan
            cases.append(Case(_rows(rs, n), time, _twist(rs), t0=0.1, inv_span=1.0 / 0.9, ref=float(rs.choice([0.0, 1.0])), src_off=src_off, dst_off=dst_off,
                              time_off=(src_off + dst_off) % 4))
    got = run(gpu_ctx, dk, cases, what="sizes")
    assert got[:, 0].sum() > 20000 and got[:, 1].sum() > 3000 and got[:, 2].sum() >= 80 and got[:, 3].sum() > 30
    # ld = n: no padding at all, columns back to back
    run(gpu_ctx, dk, [Case(_rows(rs, n), rs.uniform(0, 1, n).astype(np.float32), _twist(rs), src_off=src_off, dst_off=(src_off + 1) % 4, pad=0) for n in SIZES], what="ld = n")
    # without a counts pointer
    run(gpu_ctx, dk, cases[-8:], counts=False, what="no counts")


# ---- 2. the class table -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_twists", [False, True])
def test_class_table_with_host_and_device_twists(gpu_ctx, dk, device_twists):
    cases = [Case(rows, time, twist, **kw) for rows, time, twist, kw, _ in dm.class_table()]
    got = run(gpu_ctx, dk, cases, device_twists=device_twists, what="class table")
    for k, (_, _, _, _, exp) in enumerate(dm.class_table()):
        assert [int(v) for v in got[k, :5]] == [exp.count(c) for c in range(5)]
    assert got[2, 4] == 1 and got[2, 0] == 0                         # the NaN twist: out of range, on the host and in HBM alike


# ---- 3. the three time modes --------------------------------------------------------------------------------------------------------------------------------------
def test_time_modes_agree_bit_for_bit(gpu_ctx, dk):
    from icet_amd import lidar_sim as ls
    scene = ls.make_scene(2000)
    start = (np.zeros(3), np.eye(3))
    ring, _ = ls.make_sweep(scene, start, dm.TWIST, 3, 16, 64, 0.0, drop=False)
    azim, _ = ls.make_sweep(scene, start, dm.TWIST, 3, 16, 64, 0.0, order="azimuth", drop=False)
    ring = ring.numpy().T.copy(); azim = azim.numpy().T.copy()
    n = 16 * 64
    zero = (ring == 0).all(1)
    assert ring.shape == (n, 3) and 0 < zero.sum() < n
    i = np.arange(n)
    kw = dict(t0=0.0, inv_span=1.0 / 64, ref=1.0)
    cases = [Case(ring, None, dm.TWIST, dm.TIME_COLUMN_FAST, 64, **kw), Case(ring, (i % 64 + 0.5).astype(np.float32), dm.TWIST, **kw),
             Case(azim, None, dm.TWIST, dm.TIME_COLUMN_SLOW, 16, dst_off=1, **kw), Case(azim, (i // 16 + 0.5).astype(np.float32), dm.TWIST, src_off=2, **kw)]
    got = run(gpu_ctx, dk, cases, what="time modes")
    out = [c.d_dst.cpu().numpy()[c.dst_off_eff:] for c in cases]
    rows = [np.stack([o[a * c.ld: a * c.ld + n] for a in range(3)], 1) for o, c in zip(out, cases)]
    assert np.array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32)) and np.array_equal(rows[2].view(np.uint32), rows[3].view(np.uint32))
    assert np.array_equal(rows[0][zero].view(np.uint32), np.zeros((int(zero.sum()), 3), np.uint32))      # the zero rows stay zero, bit for bit
    assert [int(v) for v in got[:, 1]] == [int(zero.sum())] * 2 + [int((azim == 0).all(1).sum())] * 2
    # the two layouts hold the same points
    assert np.allclose(rows[2].reshape(64, 16, 3).transpose(1, 0, 2).reshape(-1, 3), rows[0], atol=2e-5)


# ---- 4. batching --------------------------------------------------------------------------------------------------------------------------------------------------
def _batch(rs_seed=7):
    rs = np.random.RandomState(rs_seed)
    lens = (300, 2049, 1, 0, 4500, 17, 2048, 777)                     # an empty scan in the middle
    return [Case(_rows(rs, n), rs.uniform(0, 1, n).astype(np.float32), _twist(rs), ref=float(k % 2), src_off=k % 4, dst_off=(3 * k) % 4) for k, n in enumerate(lens)]


def _out_rows(c):
    o = c.d_dst.cpu().numpy()[c.dst_off_eff:]
    return np.stack([o[a * c.ld: a * c.ld + c.n] for a in range(3)], 1)


def test_one_call_equals_separate_calls_and_the_reversed_order(gpu_ctx, dk):
    together = _batch(); run(gpu_ctx, dk, together, what="one call")
    alone = _batch()
    for k, c in enumerate(alone):
        run(gpu_ctx, dk, [c], what="alone %d" % k)
    rev = _batch(); run(gpu_ctx, dk, rev[::-1], what="reversed")
    for a, b, c in zip(together, alone, rev):
        assert np.array_equal(_out_rows(a).view(np.uint32), _out_rows(b).view(np.uint32)) and np.array_equal(_out_rows(a).view(np.uint32), _out_rows(c).view(np.uint32))


def test_in_place_equals_out_of_place(gpu_ctx, dk):
    out = _batch(); run(gpu_ctx, dk, out, what="out of place")
    inp = _batch()
    for c in inp:
        c.in_place = True
    run(gpu_ctx, dk, inp, what="in place")
    for a, b in zip(out, inp):
        assert np.array_equal(_out_rows(a).view(np.uint32), _out_rows(b).view(np.uint32))


def test_host_form_equals_the_model(gpu_ctx, dk):
    rs = np.random.RandomState(8)
    scans = [_rows(rs, n) for n in (0, 5, 2049, 600)]
    times = [rs.uniform(0.2, 1.4, s.shape[0]).astype(np.float32) for s in scans]
    twists = np.stack([_twist(rs) for _ in scans])
    outs, cnts = dk.deskew(scans, times, twists, ref=0.0, t0=0.2, span=1.2)
    for s, t, x, o, c in zip(scans, times, twists, outs, cnts):
        want, cls = dm.deskew(s, x, t, t0=0.2, inv_span=1.0 / 1.2, ref=0.0)
        assert np.array_equal(o.view(np.uint32), want.view(np.uint32)) and c == dm.counts(cls)


# ---- 5. twists on the device --------------------------------------------------------------------------------------------------------------------------------------
def test_device_twists_give_the_bits_of_the_host_path(gpu_ctx, dk):
    host = _batch(9); run(gpu_ctx, dk, host, what="host twists")
    dev = _batch(9); run(gpu_ctx, dk, dev, device_twists=True, what="device twists")
    for a, b in zip(host, dev):
        assert np.array_equal(_out_rows(a).view(np.uint32), _out_rows(b).view(np.uint32))


def test_twists_from_poses_on_the_device(gpu_ctx, dk):
    """A chain of float32 poses, one of them repeated: the twists agree with the model on the same float32 poses to 1e-10 (the two math libraries differ in the
    last bits of a double; the values are of order 1), and the twist between identical poses is exactly zero."""
    rs = np.random.RandomState(10)
    T = [dm.pose_from_twist(np.concatenate([rs.randn(3) * 30, rs.randn(3) * 0.7]))]
    steps = [np.concatenate([rs.uniform(-2, 2, 3), rs.uniform(-0.4, 0.4, 3)]) for _ in range(70)]
    steps[3] = np.zeros(6); steps[40] = np.array([1e-9, 0, 0, 1e-10, 0, 0]); steps[41] = np.array([0.5, 0, 0, 0, 0, 2.5])
    for x in steps:
        T.append(T[-1] @ dm.pose_from_twist(x))
    P = np.stack(T).astype(np.float32)
    assert np.array_equal(P[3], P[4])
    d_p = torch.from_numpy(P.reshape(-1, 16)).to(DEV); d_t = torch.full((70, 6), 7.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize(DEV)
    for scale in (1.0, 0.5):
        dk.twists_from_poses_device(d_p.data_ptr(), 70, d_t.data_ptr(), scale)
        gpu_ctx.sync()
        got = d_t.cpu().numpy()
        want = np.stack([dm.twist_between(P[k], P[k + 1], scale) for k in range(70)])
        err = float(np.abs(got - want).max())
        print("scale %g: max |device - model| = %.3g" % (scale, err))
        assert err <= 1e-10
        assert (got[3] == 0).all()
        assert np.abs(got / scale - np.stack(steps)).max() <= 1e-4       # float32 poses 30 m out
    # and straight into a deskew call: the bits of the host path with the same twists
    rs = np.random.RandomState(11)
    tw = d_t.cpu().numpy()[:8]
    a = [Case(_rows(rs, 500 + k), rs.uniform(0, 1, 500 + k).astype(np.float32), tw[k]) for k in range(8)]
    run(gpu_ctx, dk, a, device_twists=True, what="twists from poses")


# ---- 6. the pipeline ----------------------------------------------------------------------------------------------------------------------------------------------
def test_deskewed_buffers_go_straight_into_the_voxel_map(gpu_ctx, dk):
    from icet_amd import api
    raw, times, fixed, poses = dm.sharpness_inputs()
    want_skewed, want_deskewed = dm.sharpness_counts(0.5)
    cases = [Case(r, t, dm.TWIST, ref=0.0, pad=3) for r, t in zip(raw, times)]
    run(gpu_ctx, dk, cases, what="pipeline")
    cells = []
    for bufs in ([(c.d_src, c) for c in cases], [(c.d_dst, c) for c in cases]):
        m = api.VoxelMap(gpu_ctx, cell=0.5, table_log2=16)
        m.add_device([(b.data_ptr(), c.n, c.ld) for b, c in bufs], poses)
        cells.append(m.stats()["cells_occupied"])
        m.close()
    print("cells of 0.5 m on the device: %d skewed, %d deskewed" % tuple(cells))
    assert cells == [want_skewed, want_deskewed] and cells[1] < cells[0]
    for c, f in zip(cases, fixed):
        assert np.array_equal(_out_rows(c).view(np.uint32), f.view(np.uint32))


def test_a_deskewed_pair_registers(gpu_ctx, dk):
    """No accuracy bound (consecutive sweeps at constant velocity are skewed alike: raw and deskewed pairs register equally well): the deskewed pair goes through
    the solver and X is finite."""
    from icet_amd import lidar_sim as ls
    sweeps, _ = ls.make_sweep_sequence(2, dm.TWIST, 2000, 2001, 64, 512, 0.02)
    outs, cnts = dk.deskew([s.numpy().T for s, _ in sweeps], [t.numpy() for _, t in sweeps], [dm.TWIST] * 2, ref=0.0)
    assert all(c["moved"] == o.shape[0] for c, o in zip(cnts, outs))
    r = gpu_ctx.solve(outs[0], outs[1], 7, np.zeros(6, np.float32), 24, 75)
    print("X of the deskewed pair:", r["X"])
    assert np.isfinite(r["X"]).all()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(gpu_ctx, dk, frames):
    from icet_amd import api
    lib = api.load_library()
    a, b = frames
    before = gpu_ctx.solve(a, b, 7, np.zeros(6, np.float32), 24, 75)
    rs = np.random.RandomState(12)
    c = Case(_rows(rs, 300), rs.uniform(0, 1, 300).astype(np.float32), _twist(rs))
    c.upload()
    cnt = torch.full((2, 8), 77, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize(DEV)
    good = c.record()
    src, dst, tm, n, ld = good.src, good.dst, good.time, c.n, c.ld

    def rec(**kw):
        r = c.record()
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    bad = [rec(n=-1), rec(ld=n - 1), rec(ld_out=n - 1), rec(ld=1 << 30), rec(ld_out=1 << 30), rec(src=None), rec(dst=None), rec(time=None), rec(time_mode=3), rec(time_mode=-1),
           rec(time_mode=api.DESKEW_TIME_COLUMN_FAST, period=0), rec(time_mode=api.DESKEW_TIME_COLUMN_SLOW, period=-4), rec(dst=src + 4), rec(dst=src, ld_out=ld + 1),
           rec(dst=src + 4 * (2 * ld + n) - 4), rec(src=src + 2), rec(dst=dst + 1), rec(time=tm + 3)]
    for k, r in enumerate(bad):
        A = (api.DeskewScan * 2)(good, r)
        assert lib.icet_deskew_device(dk._h, 2, A, None, C.c_void_p(cnt.data_ptr())) == api.ICET_ERR_BAD_ARG, k
        assert lib.icet_deskewer_last_error(dk._h), k
    A = (api.DeskewScan * 1)(good)
    assert lib.icet_deskew_device(dk._h, -1, A, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_deskew_device(dk._h, 1, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_deskew_device(dk._h, 1, A, C.c_void_p(cnt.data_ptr() + 4), None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_deskew_device(dk._h, 1, A, None, C.c_void_p(cnt.data_ptr() + 4)) == api.ICET_ERR_BAD_ARG
    assert lib.icet_deskew_twists_from_poses_device(dk._h, -1, C.c_void_p(cnt.data_ptr()), 1.0, C.c_void_p(cnt.data_ptr())) == api.ICET_ERR_BAD_ARG
    assert lib.icet_deskew_twists_from_poses_device(dk._h, 1, None, 1.0, C.c_void_p(cnt.data_ptr())) == api.ICET_ERR_BAD_ARG
    assert lib.icet_deskew_twists_from_poses_device(dk._h, 1, C.c_void_p(cnt.data_ptr()), 1.0, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_deskewer_create(gpu_ctx._h, None) == api.ICET_ERR_BAD_ARG
    gpu_ctx.sync()
    assert (cnt.cpu().numpy() == 77).all()                           # the counts: not even zeroed
    assert (c.d_dst.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all() and np.array_equal(c.d_src.cpu().numpy().view(np.uint32), c.h_src.view(np.uint32))
    # non-finite parameters are NOT refused: the rule classes the rows
    ok = rec(t0=float("nan"))
    assert lib.icet_deskew_device(dk._h, 1, (api.DeskewScan * 1)(ok), None, C.c_void_p(cnt.data_ptr())) == api.ICET_OK
    gpu_ctx.sync()
    got = cnt.cpu().numpy()
    assert got[0, 0] == 0 and got[0, 4] > 200 and (got[1] == 77).all()
    # the identical in-place form and n = 0 are accepted; the context registers as before
    assert lib.icet_deskew_device(dk._h, 1, (api.DeskewScan * 1)(rec(dst=src)), None, None) == api.ICET_OK
    assert lib.icet_deskew_device(dk._h, 0, None, None, None) == api.ICET_OK
    gpu_ctx.sync()
    after = gpu_ctx.solve(a, b, 7, np.zeros(6, np.float32), 24, 75)
    for k in ("X", "pred_stds", "cov"):
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
