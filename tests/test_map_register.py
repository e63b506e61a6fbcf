"""The registration against a shaped voxel map on the GPU (include/icet_hip.h icet_voxel_map_register_*) against the NumPy model of
tests/map_register_model.py: the per-row terms BIT FOR BIT, the totals of a scored pose within the bound of their summation, the records identical whatever the
call's shape, the Gaussians rebuilt when they are stale, and the whole loop converging where the model converges."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import map_model as mm
import map_register_cases as cs
import map_register_model as rm
import map_shape_model as sm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LOG2 = 14
U = 2.0 ** -53


def _upload(scan, pad=3, off=1):
    """An N x 3 scan as a device buffer with leading dimension n + pad, NaN in the padding, and the first row `off` floats into the allocation (off 1: every column
    is aligned to 4 bytes and to nothing more, whatever n; off 0 and n + pad a multiple of 4: every column to 16 bytes): (buffer, (ptr, n, ld))."""
    s = np.asarray(scan, np.float32).reshape(-1, 3)
    n = s.shape[0]; ld = n + pad
    h = np.full(off + 3 * max(ld, 1), np.nan, np.float32)
    h[off:off + 3 * ld].reshape(3, ld)[:, :n] = s.T
    b = torch.from_numpy(h).to(DEV)
    return b, (b.data_ptr() + 4 * off, n, ld)


def _descs(scans, pad=3, off=1):
    bufs = [_upload(s, pad, off) for s in scans]
    torch.cuda.synchronize(DEV)
    return [b for b, _ in bufs], [d for _, d in bufs]


def _gpu_map(ctx, cell, scans, poses, remove=None, log2=LOG2):
    from icet_amd import api
    m = api.VoxelMap(ctx, cell=cell, table_log2=log2, shape=True)
    m.add(scans, np.asarray(poses, np.float32))
    if remove:
        m.remove(remove, np.asarray([mm.pose()] * len(remove), np.float32))
    return m


def _slab_map(ctx, cell):
    scans, poses = cs.base_map(cell)
    add, rem, _ = cs.special_cells(cell)
    return _gpu_map(ctx, cell, scans + add, poses + [mm.pose()] * len(add), remove=rem)


def _bytes(recs):
    return np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1)


def _same_records(a, b, what=""):
    bad = np.nonzero((_bytes(a) != _bytes(b)).any(axis=1))[0]
    assert bad.size == 0, (what, bad, a[bad[:1]], b[bad[:1]])


def test_refusals_change_nothing(gpu_ctx):
    from icet_amd import api
    lib = api.load_library()
    cell = 0.5
    m = _slab_map(gpu_ctx, cell)
    before = m.extract_shape(moments=True)
    rows = cs.term_rows(cell, 300)
    keep, descs = _descs([rows])
    A = api._dev_scans(descs)
    T = np.ascontiguousarray(cs.POSE.reshape(1, 16))
    out = torch.full((4 * api.MAP_REGISTRATION_DTYPE.itemsize + 8,), 0xAB, dtype=torch.uint8, device=DEV)
    dT = torch.from_numpy(np.concatenate([[0.0], T.reshape(16)]).astype(np.float32)).to(DEV)
    torch.cuda.synchronize(DEV)
    ok = api.map_register_params()
    P = lambda **kw: api.map_register_params(**kw)
    res = lambda a, b: api.MapRegisterParams(0.0, 0.0, 0.02, 11.3449, 1e-4, 1e-5, 1e-3, 5, 50, 20, 0, (C.c_int32 * 2)(a, b))
    plain = api.VoxelMap(gpu_ctx, cell=cell, table_log2=LOG2)
    bad_desc = api._dev_scans([(descs[0][0], 300, 299)])
    odd_desc = api._dev_scans([(descs[0][0] + 2, 300, 303)])
    calls = [
        (plain._h, 1, A, T.ctypes.data, C.byref(ok), out.data_ptr()),                                  # a map without shape
        (m._h, 1, None, T.ctypes.data, C.byref(ok), out.data_ptr()), (m._h, 1, A, None, C.byref(ok), out.data_ptr()), (m._h, 1, A, T.ctypes.data, C.byref(ok), None),
        (m._h, 0, A, T.ctypes.data, C.byref(ok), out.data_ptr()), (m._h, api.VOXEL_MAP_MAX_QUERIES + 1, A, T.ctypes.data, C.byref(ok), out.data_ptr()),
        (m._h, 1, bad_desc, T.ctypes.data, C.byref(ok), out.data_ptr()), (m._h, 1, odd_desc, T.ctypes.data, C.byref(ok), out.data_ptr()),
        (m._h, 1, A, T.ctypes.data, C.byref(ok), out.data_ptr() + 4),                                  # records at an address that is 4 modulo 8
    ]
    for kw in (dict(sigma_min=0.0), dict(sigma_min=-0.02), dict(sigma_min=math.nan), dict(sigma_min=math.inf), dict(scale=0.0), dict(scale=math.nan), dict(scale=math.inf),
               dict(max_iters=-1), dict(max_iters=65), dict(tol_t=-1e-9), dict(tol_r=-1e-9), dict(flags=1), dict(lambda0=0.0), dict(min_range=math.nan)):
        calls.append((m._h, 1, A, T.ctypes.data, C.byref(P(**kw)), out.data_ptr()))
    calls += [(m._h, 1, A, T.ctypes.data, C.byref(res(1, 0)), out.data_ptr()), (m._h, 1, A, T.ctypes.data, C.byref(res(0, 1)), out.data_ptr())]
    for k, a in enumerate(calls):
        h, n_q, sc, poses, par, recs = a
        assert lib.icet_voxel_map_register_device(h, n_q, sc, api._vp(poses), par, api._vp(recs)) == api.ICET_ERR_BAD_ARG, k
        assert lib.icet_voxel_map_last_error(h), k
    assert lib.icet_voxel_map_register_posed_device(m._h, 1, A, api._vp(dT.data_ptr() + 4 + 2), C.byref(ok), api._vp(out.data_ptr())) == api.ICET_ERR_BAD_ARG
    assert lib.icet_voxel_map_register_posed_device(m._h, 1, A, None, C.byref(ok), api._vp(out.data_ptr())) == api.ICET_ERR_BAD_ARG
    terms = torch.full((300 * 256 + 8,), 0xAB, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize(DEV)
    assert lib.icet_debug_voxel_map_register_terms(m._h, A, T.ctypes.data, C.byref(ok), None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_debug_voxel_map_register_terms(m._h, A, T.ctypes.data, C.byref(P(scale=-1.0)), api._vp(terms.data_ptr())) == api.ICET_ERR_BAD_ARG
    assert lib.icet_debug_voxel_map_register_terms(plain._h, A, T.ctypes.data, C.byref(ok), api._vp(terms.data_ptr())) == api.ICET_ERR_BAD_ARG
    assert lib.icet_debug_voxel_map_register_terms(m._h, A, T.ctypes.data, C.byref(ok), api._vp(terms.data_ptr() + 4)) == api.ICET_ERR_BAD_ARG
    gpu_ctx.sync()
    assert (out.cpu().numpy() == 0xAB).all() and (terms.cpu().numpy() == 0xAB).all()
    after = m.extract_shape(moments=True)
    for k in ("key", "count", "xyz", "moments", "cov"):
        assert np.array_equal(after[k], before[k]), k
    with pytest.raises(api.IcetError) as e:
        plain.score([rows], T)
    assert e.value.status == api.ICET_ERR_BAD_ARG and "shape" in str(e.value)
    # the accepted forms of the same arguments, NULL params (the defaults) among them: the same record
    assert lib.icet_voxel_map_register_device(m._h, 1, A, T.ctypes.data, None, api._vp(out.data_ptr())) == api.ICET_OK
    gpu_ctx.sync()
    a = out.cpu().numpy()[:328].copy()
    assert lib.icet_voxel_map_register_posed_device(m._h, 1, A, api._vp(dT.data_ptr() + 4), C.byref(ok), api._vp(out.data_ptr() + 328)) == api.ICET_OK
    gpu_ctx.sync()
    assert np.array_equal(a, out.cpu().numpy()[328:656]) and (out.cpu().numpy()[656:] == 0xAB).all()
    plain.close(); m.close()


@pytest.mark.parametrize("cell", [0.1, 0.5])
def test_row_terms_equal_the_model_bit_for_bit(gpu_ctx, cell):
    """icet_debug_voxel_map_register_terms runs the production row pass: for every row count around the lane trip and the chunk, columns aligned to 4 bytes only
    and to 16, NaN in the padding, NaN / infinite / zero rows, rows outside the range and outside the grid, a row in an empty cell, in a cell below min_points, in
    an emptied and in a negative-count cell, at a pose that is not axis-aligned: every word of every record equals the model's."""
    from icet_amd import api
    m = _slab_map(gpu_ctx, cell)
    G = rm.Gaussians(cs.model_map(cell))
    R, t = rm.pose64(cs.POSE)
    seen = set()
    for n in cs.ROW_COUNTS:
        rows = cs.term_rows(cell, n)
        for pad, off in ((3, 1), ((-n) % 4, 0)):
            buf, desc = _upload(rows, pad, off)
            torch.cuda.synchronize(DEV)
            assert (desc[0] % 16 == 0 and desc[2] % 4 == 0) if off == 0 else desc[0] % 8 == 4
            for mn, mx in ((0.05, 30.0), (0.0, 0.0)):
                out = torch.zeros(n * 256, dtype=torch.uint8, device=DEV)
                torch.cuda.synchronize(DEV)
                m.register_terms_device(desc, cs.POSE, out.data_ptr(), min_range=mn, max_range=mx)
                gpu_ctx.sync()
                got = out.cpu().numpy().view(api.MAP_REGISTER_TERM_DTYPE)
                tm = rm.row_terms(rows, R, t, G, rm.DEFAULTS["scale"], mn, mx)
                what = (cell, n, pad, off, mn, mx)
                assert np.array_equal(got["cls"], tm["cls"]), what
                assert np.array_equal(got["key"], tm["key"]), what
                assert np.array_equal(got["matched"], tm["matched"].astype(np.int32)), what
                for k in ("s", "omega", "rho"):
                    assert np.array_equal(got[k].view(np.uint64), tm[k].view(np.uint64)), (what, k)
                assert np.array_equal(got["g"].view(np.uint64), np.ascontiguousarray(tm["v"][:, 1:7]).view(np.uint64)), what
                assert np.array_equal(got["H"].view(np.uint64), np.ascontiguousarray(tm["v"][:, 7:]).view(np.uint64)), what
                seen |= set(int(c) for c in tm["cls"])
                if n >= 255:
                    assert not tm["matched"][:4].any() and tm["matched"].sum() > n // 3      # the empty, the few, the emptied and the negative cell; the slab
                    assert (tm["rho"][:4] == rm.DEFAULTS["scale"]).all() and not tm["v"][:4].any()
    assert seen == {mm.KEPT, mm.NONFINITE, mm.RANGE, mm.OUTSIDE}
    m.close()


@pytest.mark.parametrize("cell", [0.1, 0.5])
def test_totals_of_a_scored_pose(gpu_ctx, cell):
    """max_iters = 0, one query per row count in ONE call: rows_scored and rows_matched are exact; cost, g and info lie within gamma_(N-1) sum |term| of the exact
    sum (math.fsum) of the per-row terms, gamma_k = k u / (1 - k u), u = 2^-53, N the rows scored -- the bound of ANY order of N - 1 additions of the N terms
    (the cost adds scale x the counted misses: one product and one addition in place of the misses' own additions)."""
    m = _slab_map(gpu_ctx, cell)
    G = rm.Gaussians(cs.model_map(cell))
    R, t = rm.pose64(cs.POSE)
    scans = [cs.term_rows(cell, n) for n in cs.ROW_COUNTS]
    keep, descs = _descs(scans)
    recs = m.register_records(descs, np.stack([cs.POSE] * len(scans)), max_iters=0, min_matched=0, min_range=0.05, max_range=30.0)
    for rows, r in zip(scans, recs):
        tm = rm.row_terms(rows, R, t, G, rm.DEFAULTS["scale"], 0.05, 30.0)
        exact, ns, nm = rm.totals(tm, "exact")
        assert (r["rows_scored"], r["rows_matched"]) == (ns, nm) and r["iterations"] == 0 and r["accepted"] == 0 and r["status"] == rm.ITERATION_CAP
        assert np.array_equal(r["pose"].view(np.uint32), cs.POSE.reshape(16).view(np.uint32)) and r["cost"] == r["cost_start"]
        v = tm["v"][tm["scored"]].copy(); v[:, 0] = tm["rho"][tm["scored"]]
        k = max(ns - 1, 0)
        bound = (k * U / (1.0 - k * U)) * np.array([math.fsum(np.abs(v[:, j])) for j in range(rm.SUMS)])
        got = np.concatenate([[r["cost"]], r["g"], r["info"]])
        err = np.abs(got - exact)
        print("cell %.1f rows %d scored %d: largest error / bound %.3f" % (cell, rows.shape[0], ns, float(np.max(err / np.maximum(bound, 1e-300))) if ns > 1 else 0.0))
        assert (err <= bound).all(), (rows.shape[0], err, bound)
    m.close()


def _scene_map(ctx):
    s = cs.scene()
    return s, _gpu_map(ctx, s["cell"], s["scans"], s["poses"], log2=15)


def test_records_do_not_depend_on_the_shape_of_the_call(gpu_ctx):
    """The same call twice; Q queries in one call against Q calls of one; the queries in another order; host poses against device poses; and a query that is
    terminal after a few passes beside one that runs ten times as long: every record has the same bytes wherever it was computed."""
    s, m = _scene_map(gpu_ctx)
    keep, descs = _descs([h[0] for h in s["held"]])
    of = [i for i, _ in s["starts"]]
    T = np.stack([T0 for _, T0 in s["starts"]])
    kw = dict(max_iters=30)
    d = [descs[i] for i in of]
    a = m.register_records(d, T, **kw)
    _same_records(a, m.register_records(d, T, **kw), "the same call twice")
    solo = np.concatenate([m.register_records([d[k]], T[k:k + 1], **kw) for k in range(len(d))])
    _same_records(a, solo, "one call of Q against Q calls of one")
    perm = [4, 0, 5, 2, 1, 3]
    _same_records(a[perm], m.register_records([d[k] for k in perm], T[perm], **kw), "another order")
    dT = torch.from_numpy(T.copy()).to(DEV)
    torch.cuda.synchronize(DEV)
    _same_records(a, m.register_records(d, dT, **kw), "device poses")
    # a start at the pose the first query ended at is terminal at once or soon; beside a query that runs on, it gives its solo bytes
    assert a["iterations"][0] >= 10
    T2 = np.stack([a["pose"][0].reshape(4, 4), T[0], a["pose"][3].reshape(4, 4)])
    d2 = [d[0], d[0], d[3]]
    b = m.register_records(d2, T2, **kw)
    assert b["iterations"][0] < b["iterations"][1] and b["status"][0] != rm.ITERATION_CAP and b["iterations"][1] == a["iterations"][0]
    solo = np.concatenate([m.register_records([d2[k]], T2[k:k + 1], **kw) for k in range(3)])
    _same_records(b, solo, "a short query beside a long one")
    _same_records(b[1:2], a[0:1], "the long one, again")
    m.close()


def test_stale_gaussians_are_rebuilt(gpu_ctx):
    """An add between two calls, and another sigma_min (or min_points) in the second call: the records of a map built afresh."""
    from icet_amd import api
    cell = 0.5
    scans, poses = cs.base_map(cell)
    rows = cs.term_rows(cell, 2500)
    T = mm.pose(t=(0.4, -0.2, 0.12), r=(0.02, -0.015, 0.41))[None]
    keep, descs = _descs([rows])
    kw = dict(max_iters=4)
    m = _gpu_map(gpu_ctx, cell, scans[:1], poses[:1])
    first = m.register_records(descs, T, **kw)
    m.add(scans[1:], np.asarray(poses[1:], np.float32))
    second = m.register_records(descs, T, **kw)
    fresh = _gpu_map(gpu_ctx, cell, scans, poses)
    _same_records(second, fresh.register_records(descs, T, **kw), "after an add")
    assert (_bytes(first) != _bytes(second)).any()
    wide = m.register_records(descs, T, sigma_min=0.05, **kw)
    fresh2 = _gpu_map(gpu_ctx, cell, scans, poses)
    _same_records(wide, fresh2.register_records(descs, T, sigma_min=0.05, **kw), "another sigma_min")
    assert (_bytes(wide) != _bytes(second)).any()
    _same_records(m.register_records(descs, T, min_points=12, **kw), fresh2.register_records(descs, T, min_points=12, **kw), "another min_points")
    _same_records(m.register_records(descs, T, **kw), second, "and back")
    m.remove(scans[1:], np.asarray(poses[1:], np.float32))
    _same_records(m.register_records(descs, T, **kw), first, "after a remove")
    m.clear()
    assert m.register_records(descs, T, **kw)["status"][0] == api.VOXEL_MAP_REG_NO_OVERLAP
    for x in (m, fresh, fresh2):
        x.close()


def test_the_loop_converges_where_the_model_converges(gpu_ctx):
    """lidar_sim.make_scene(3100), eight scans of rings=16, steps=512 fused at cell 0.5, two held-out scans, three starts each, 0.1 .. 0.2 m and 0.02 .. 0.03 rad
    off (tests/map_register_cases.py scene()).  The model alone is CONVERGED from every start (checked here, on the CPU), and so is every device query.  The
    device and the model differ in the order of their sums only, so the device's pose is held to the model's within 4 x the largest difference between the model
    and the same model summing its rows in REVERSE order -- measured here: 8.9e-16 over the six starts, the bound 3.6e-15 -- plus the rounding of the record's
    float32 entries (half a float32 spacing of the model's entry).  The pose error against the truth is held to 1.5 x the model's own (5 mm here: the cell size
    over a hundred)."""
    s, m = _scene_map(gpu_ctx)
    model, rev = cs.scene_model("forward"), cs.scene_model("reverse")
    assert all(r["status"] == rm.CONVERGED for r in model) and all(r["status"] == rm.CONVERGED for r in rev)
    measured = max(cs.pose_diff(a["pose64"], b["pose64"]) for a, b in zip(model, rev))
    print("model forward against reverse: largest pose difference %.3e" % measured)
    assert measured > 0.0
    got = m.register([h[0] for h in s["held"]], np.stack([T0 for _, T0 in s["starts"]]), scan_of=[i for i, _ in s["starts"]], **s["params"])
    for k, (g, w) in enumerate(zip(got, model)):
        Tt = np.asarray(s["held"][s["starts"][k][0]][1], np.float64)
        assert g["status"] == rm.CONVERGED, (k, g)
        want = np.eye(4); want[:3, :3] = w["pose64"][0]; want[:3, 3] = w["pose64"][1]
        half_ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) / 2
        diff = np.abs(g["pose"].astype(np.float64) - want)
        print("start %d: device %d passes, model %d; |device - model| largest %.3e; cost %.6f against %.6f" % (k, g["iterations"], w["iterations"], diff.max(), g["cost"], w["cost"]))
        assert (diff <= 4 * measured + half_ulp).all(), (k, diff, 4 * measured)
        err = lambda P: (float(np.linalg.norm(P[:3, 3] - Tt[:3, 3])), float(np.linalg.norm(P[:3, :3] - Tt[:3, :3])))
        (et, er), (mt, mr) = err(g["pose"].astype(np.float64)), err(want)
        assert et <= 1.5 * mt and er <= 1.5 * mr, (k, et, mt, er, mr)
        assert g["cost"] < g["cost_start"] and g["rows_matched"] == w["rows_matched"] and g["rows_scored"] == w["rows_scored"]
    m.close()


def test_no_overlap_bad_pose_and_an_empty_scan(gpu_ctx):
    from icet_amd import api
    cell = 0.5
    m = _slab_map(gpu_ctx, cell)
    rows = cs.term_rows(cell, 2500)
    far = mm.pose(t=(1000.0, 0.0, 0.0), r=(0.0, 0.0, 0.3))
    bad = cs.POSE.copy(); bad[1, 3] = np.nan
    inf = cs.POSE.copy(); inf[0, 0] = np.inf
    T = np.stack([cs.POSE, far, bad, cs.POSE, inf, cs.POSE])
    r = m.register([rows, rows[:0]], T, scan_of=[0, 0, 0, 1, 0, 0], max_iters=5)
    solo = m.register([rows], cs.POSE[None], max_iters=5)[0]
    n_scored = int(rm.row_terms(rows, *rm.pose64(far), rm.Gaussians(cs.model_map(cell)))["scored"].sum())
    assert r[1]["status"] == api.VOXEL_MAP_REG_NO_OVERLAP and np.array_equal(r[1]["pose"].view(np.uint32), far.view(np.uint32))
    assert r[1]["rows_matched"] == 0 and r[1]["rows_scored"] == n_scored > 2400 and r[1]["cost"] == rm.DEFAULTS["scale"] * n_scored and r[1]["iterations"] == 0
    assert not r[1]["g"].any() and not r[1]["info"].any()
    for k in (2, 4):
        assert r[k]["status"] == api.VOXEL_MAP_REG_BAD_POSE and r[k]["iterations"] == 0 and r[k]["rows_matched"] == 0
        assert np.array_equal(r[k]["pose"].view(np.uint32), T[k].view(np.uint32))
    assert r[3]["status"] == api.VOXEL_MAP_REG_NO_OVERLAP and r[3]["rows_scored"] == 0 and r[3]["cost"] == 0.0
    assert np.array_equal(r[3]["pose"].view(np.uint32), cs.POSE.view(np.uint32))
    for k in (0, 5):                                                  # the neighbours of the bad poses are the query alone
        assert r[k]["status"] == solo["status"] and r[k]["cost"] == solo["cost"] and np.array_equal(r[k]["pose"], solo["pose"]) and r[k]["rows_matched"] > 1000
    only = m.register([rows[:0]], cs.POSE[None])[0]                   # a call of nothing but an empty scan
    assert only["status"] == api.VOXEL_MAP_REG_NO_OVERLAP and only["rows_scored"] == 0
    assert len(m.register_terms(rows[:0], cs.POSE)) == 0
    sc = m.score([rows], cs.POSE[None])[0]
    assert sc["iterations"] == 0 and sc["cost"] == sc["cost_start"] == solo["cost_start"]
    cov = api.registration_cov(sc)
    assert np.isfinite(cov).all() and np.allclose(cov @ api.info_matrix(sc["info"]), np.eye(6), atol=1e-6)
    assert np.isnan(api.registration_cov(r[1])).all()
    Rm = sc["pose"][:3, :3].astype(np.float64)
    body = api.info_body_from_world(sc["info"], Rm)
    assert np.allclose(body[:3, :3], Rm.T @ api.info_matrix(sc["info"])[:3, :3] @ Rm) and np.allclose(body, body.T)
    m.close()
