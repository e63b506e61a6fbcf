"""The neighbourhoods of the registration against a shaped voxel map on the GPU (include/icet_hip.h ICET_VOXEL_MAP_REG_NEIGHBOURS_7 / _27)
against the NumPy model of tests/map_register_neighbours_model.py: the flags that are accepted and refused, the per-row terms and the winner's place BIT FOR BIT,
the totals of a scored pose within the bound of their summation, the records identical whatever the call's shape and untouched by centre-only calls in between,
the Gaussians rebuilt when they are stale, and the loop under 27 cells taking the model's passes to the model's pose."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import map_model as mm
import map_register_cases as cs
import map_register_model as rm
import map_register_neighbours_cases as nc
import map_register_neighbours_model as nm
import test_map_register as tr

pytestmark = pytest.mark.gpu
DEV = tr.DEV
U = 2.0 ** -53
NBS = (7, 27)


def _nb_map(ctx, cell):
    """The slab map with its special cells (test_map_register's) and the points of the edge case: nc.model_map on the device."""
    scans, poses = cs.base_map(cell)
    add, rem, _ = cs.special_cells(cell)
    edge = nc.edge_case(cell)[0]
    return tr._gpu_map(ctx, cell, scans + add + edge, poses + [mm.pose()] * (len(add) + len(edge)), remove=rem)


def test_the_flags_that_name_a_neighbourhood_and_the_ones_that_do_not(gpu_ctx):
    """flags 2 and 4 are accepted by all three entry points; 6 (both bits), 8, 3 and 1 are refused with ICET_ERR_BAD_ARG, the sentinel-filled buffers and the map
    untouched."""
    from icet_amd import api
    lib = api.load_library()
    cell = 0.5
    m = _nb_map(gpu_ctx, cell)
    before = m.extract_shape(moments=True)
    rows = cs.term_rows(cell, 300)
    keep, descs = tr._descs([rows])
    A = api._dev_scans(descs)
    T = np.ascontiguousarray(cs.POSE.reshape(1, 16))
    out = torch.full((api.MAP_REGISTRATION_DTYPE.itemsize + 8,), 0xAB, dtype=torch.uint8, device=DEV)
    terms = torch.full((300 * 256 + 8,), 0xAB, dtype=torch.uint8, device=DEV)
    dT = torch.from_numpy(T.reshape(16).copy()).to(DEV)
    torch.cuda.synchronize(DEV)
    for fl in (6, 8, 3, 1, -1, 2 | 16, 4 | 1):
        P = api.map_register_params(flags=fl, max_iters=2)
        assert lib.icet_voxel_map_register_device(m._h, 1, A, T.ctypes.data, C.byref(P), api._vp(out.data_ptr())) == api.ICET_ERR_BAD_ARG, fl
        assert lib.icet_voxel_map_last_error(m._h), fl
        assert lib.icet_voxel_map_register_posed_device(m._h, 1, A, api._vp(dT.data_ptr()), C.byref(P), api._vp(out.data_ptr())) == api.ICET_ERR_BAD_ARG, fl
        assert lib.icet_debug_voxel_map_register_terms(m._h, A, T.ctypes.data, C.byref(P), api._vp(terms.data_ptr())) == api.ICET_ERR_BAD_ARG, fl
    gpu_ctx.sync()
    assert (out.cpu().numpy() == 0xAB).all() and (terms.cpu().numpy() == 0xAB).all()
    after = m.extract_shape(moments=True)
    for k in ("key", "count", "xyz", "moments", "cov"):
        assert np.array_equal(after[k], before[k]), k
    with pytest.raises(ValueError):
        m.score([rows], T, neighbours=9)
    recs = {}
    for fl, nb in ((0, 1), (2, 7), (4, 27)):
        P = api.map_register_params(flags=fl, max_iters=2)
        assert lib.icet_voxel_map_register_device(m._h, 1, A, T.ctypes.data, C.byref(P), api._vp(out.data_ptr())) == api.ICET_OK, fl
        gpu_ctx.sync()
        a = out.cpu().numpy()[:328].copy()
        assert (out.cpu().numpy()[328:] == 0xAB).all()
        assert lib.icet_voxel_map_register_posed_device(m._h, 1, A, api._vp(dT.data_ptr()), C.byref(P), api._vp(out.data_ptr())) == api.ICET_OK, fl
        assert lib.icet_debug_voxel_map_register_terms(m._h, A, T.ctypes.data, C.byref(P), api._vp(terms.data_ptr())) == api.ICET_OK, fl
        gpu_ctx.sync()
        assert np.array_equal(a, out.cpu().numpy()[:328]) and (terms.cpu().numpy()[300 * 256:] == 0xAB).all()
        recs[nb] = a.view(api.MAP_REGISTRATION_DTYPE)[0]
        by_kw = m.register_records(descs, T, neighbours=nb, max_iters=2)      # the keyword names the same call
        assert np.array_equal(tr._bytes(by_kw)[0], a)
    assert recs[1]["rows_matched"] < recs[7]["rows_matched"] < recs[27]["rows_matched"] and recs[1]["rows_scored"] == recs[27]["rows_scored"]
    assert recs[27]["cost_start"] < recs[7]["cost_start"] < recs[1]["cost_start"]
    m.close()


def _check_terms(got, tm, what):
    assert np.array_equal(got["cls"], tm["cls"]), what
    assert np.array_equal(got["key"], tm["key"]), what
    assert np.array_equal(got["matched"], (tm["place"] + 1).astype(np.int32)), what
    for k in ("s", "omega", "rho"):
        assert np.array_equal(got[k].view(np.uint64), tm[k].view(np.uint64)), (what, k)
    assert np.array_equal(got["g"].view(np.uint64), np.ascontiguousarray(tm["v"][:, 1:7]).view(np.uint64)), what
    assert np.array_equal(got["H"].view(np.uint64), np.ascontiguousarray(tm["v"][:, 7:]).view(np.uint64)), what


def _terms(ctx, m, desc, n, pose, **kw):
    from icet_amd import api
    out = torch.zeros(max(n, 1) * 256, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize(DEV)
    m.register_terms_device(desc, pose, out.data_ptr(), **kw)
    ctx.sync()
    return out.cpu().numpy().view(api.MAP_REGISTER_TERM_DTYPE)[:n]


@pytest.mark.parametrize("cell", [0.1, 0.5])
def test_row_terms_and_the_winner_equal_the_model_bit_for_bit(gpu_ctx, cell):
    """icet_debug_voxel_map_register_terms runs the production row pass of the neighbourhood: for 7 and 27 cells, every row count around the lane trip and the
    chunk, columns aligned to 4 bytes only and to 16, the named rows of term_rows at a pose that is not axis-aligned, and the rows in the last cells of the grid:
    every word of every record equals the model's, `matched` is 1 + the winner's place, `key` the row's own cell."""
    m = _nb_map(gpu_ctx, cell)
    G = rm.Gaussians(nc.model_map(cell))
    R, t = rm.pose64(cs.POSE)
    places = {nb: set() for nb in NBS}
    for n in cs.ROW_COUNTS:
        rows = cs.term_rows(cell, n)
        for pad, off in ((3, 1), ((-n) % 4, 0)):
            buf, desc = tr._upload(rows, pad, off)
            torch.cuda.synchronize(DEV)
            assert (desc[0] % 16 == 0 and desc[2] % 4 == 0) if off == 0 else desc[0] % 8 == 4
            for nb in NBS:
                for mn, mx in ((0.05, 30.0), (0.0, 0.0)):
                    got = _terms(gpu_ctx, m, desc, n, cs.POSE, neighbours=nb, min_range=mn, max_range=mx)
                    tm = nm.row_terms(rows, R, t, G, nb, rm.DEFAULTS["scale"], mn, mx)
                    _check_terms(got, tm, (cell, n, pad, off, nb, mn, mx))
                    places[nb] |= set(int(p) for p in tm["place"])
                if n >= 255:
                    assert (tm["place"][:4] == -1).all() and (tm["rho"][:4] == rm.DEFAULTS["scale"]).all()      # the named cells stand alone: still misses
                    assert (tm["place"] > 0).sum() > n // 20 and set(tm["cls"]) == {mm.KEPT, mm.NONFINITE, mm.RANGE, mm.OUTSIDE}
    assert places[7] == set(range(-1, 7)) and places[27] == set(range(-1, 27))      # every place wins somewhere, and somewhere none does
    rows = nc.edge_case(cell)[1]
    for pad, off in ((3, 1), (1, 0)):
        buf, desc = tr._upload(rows, pad, off)
        for nb, want in ((7, [3, 2, 5, 4, 7, 6, 0]), (27, [23, 6, 17, 12, 15, 14, 0])):
            got = _terms(gpu_ctx, m, desc, len(rows), mm.pose(), neighbours=nb)
            _check_terms(got, nm.row_terms(rows, *rm.pose64(mm.pose()), G, nb), (cell, "edge", nb))
            assert list(got["matched"]) == want and list(got["cls"]) == [mm.KEPT] * 6 + [mm.OUTSIDE]
    m.close()


def test_a_tie_goes_to_the_earlier_cell_on_the_device(gpu_ctx):
    pts, rows, want = nc.tie_case()
    m = tr._gpu_map(gpu_ctx, 0.5, pts, [mm.pose()])
    G = rm.Gaussians(nc.tie_map(), **nc.TIE_PARAMS)
    buf, desc = tr._upload(rows)
    for col, nb in enumerate(NBS):
        got = _terms(gpu_ctx, m, desc, len(rows), mm.pose(), neighbours=nb, **nc.TIE_PARAMS)
        _check_terms(got, nm.row_terms(rows, *rm.pose64(mm.pose()), G, nb), ("tie", nb))
        assert list(got["matched"]) == [w[col] + 1 for w in want] and list(got["s"]) == [64.0, 64.0, 16.0]
    m.close()


@pytest.mark.parametrize("cell", [0.1, 0.5])
def test_totals_of_a_scored_pose(gpu_ctx, cell):
    """max_iters = 0, one query per row count in ONE call, per neighbourhood: rows_scored and rows_matched are exact; cost, g and info lie within
    gamma_(N-1) sum |term| of the exact sum (math.fsum) of the model's per-row terms, gamma_k = k u / (1 - k u), u = 2^-53, N the rows scored."""
    m = _nb_map(gpu_ctx, cell)
    G = rm.Gaussians(nc.model_map(cell))
    R, t = rm.pose64(cs.POSE)
    scans = [cs.term_rows(cell, n) for n in cs.ROW_COUNTS]
    keep, descs = tr._descs(scans)
    for nb in NBS:
        recs = m.register_records(descs, np.stack([cs.POSE] * len(scans)), neighbours=nb, max_iters=0, min_matched=0, min_range=0.05, max_range=30.0)
        for rows, r in zip(scans, recs):
            tm = nm.row_terms(rows, R, t, G, nb, rm.DEFAULTS["scale"], 0.05, 30.0)
            exact, ns, nmatch = rm.totals(tm, "exact")
            assert (r["rows_scored"], r["rows_matched"]) == (ns, nmatch) and r["iterations"] == 0 and r["accepted"] == 0 and r["status"] == rm.ITERATION_CAP
            assert np.array_equal(r["pose"].view(np.uint32), cs.POSE.reshape(16).view(np.uint32)) and r["cost"] == r["cost_start"]
            v = tm["v"][tm["scored"]].copy(); v[:, 0] = tm["rho"][tm["scored"]]
            k = max(ns - 1, 0)
            bound = (k * U / (1.0 - k * U)) * np.array([math.fsum(np.abs(v[:, j])) for j in range(rm.SUMS)])
            got = np.concatenate([[r["cost"]], r["g"], r["info"]])
            err = np.abs(got - exact)
            print("cell %.1f, %d cells, rows %d scored %d matched %d: largest error / bound %.3f" %
                  (cell, nb, rows.shape[0], ns, nmatch, float(np.max(err / np.maximum(bound, 1e-300))) if ns > 1 else 0.0))
            assert (err <= bound).all(), (nb, rows.shape[0], err, bound)
    m.close()


@pytest.mark.parametrize("neighbours", NBS)
def test_records_do_not_depend_on_the_shape_of_the_call(gpu_ctx, neighbours):
    """The same call twice; Q queries in one call against Q calls of one; host poses against device poses; and a centre-only call between two calls of the
    neighbourhood, which changes neither them nor itself: every record has the same bytes wherever it was computed."""
    s, m = tr._scene_map(gpu_ctx)
    keep, descs = tr._descs([h[0] for h in s["held"]])
    of = [i for i, _ in s["starts"]]
    T = np.stack([T0 for _, T0 in s["starts"]])
    kw = dict(max_iters=30, neighbours=neighbours)
    d = [descs[i] for i in of]
    own = m.register_records(d, T, max_iters=30)
    a = m.register_records(d, T, **kw)
    tr._same_records(own, m.register_records(d, T, max_iters=30), "centre only, with a neighbourhood call in between")
    tr._same_records(a, m.register_records(d, T, **kw), "the same call twice, with a centre-only call in between")
    assert (tr._bytes(a) != tr._bytes(own)).any(axis=1).all()
    solo = np.concatenate([m.register_records([d[k]], T[k:k + 1], **kw) for k in range(len(d))])
    tr._same_records(a, solo, "one call of Q against Q calls of one")
    dT = torch.from_numpy(T.copy()).to(DEV)
    torch.cuda.synchronize(DEV)
    tr._same_records(a, m.register_records(d, dT, **kw), "device poses")
    out = torch.zeros(len(d) * 328, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize(DEV)
    m.register_posed_device(d, dT, out.data_ptr(), **kw)
    gpu_ctx.sync()
    from icet_amd import api
    tr._same_records(a, out.cpu().numpy().view(api.MAP_REGISTRATION_DTYPE), "register_posed_device")
    m.close()


@pytest.mark.parametrize("neighbours", NBS)
def test_stale_gaussians_are_rebuilt(gpu_ctx, neighbours):
    """An add or a remove between two calls, and another sigma_min in the second call: the records of a map built afresh.  The neighbourhood itself is no part of
    what makes the Gaussians stale: calls of different neighbourhoods in a row share them."""
    cell = 0.5
    scans, poses = cs.base_map(cell)
    rows = cs.term_rows(cell, 2500)
    T = mm.pose(t=(0.4, -0.2, 0.12), r=(0.02, -0.015, 0.41))[None]
    keep, descs = tr._descs([rows])
    kw = dict(max_iters=4, neighbours=neighbours)
    m = tr._gpu_map(gpu_ctx, cell, scans[:1], poses[:1])
    first = m.register_records(descs, T, **kw)
    m.add(scans[1:], np.asarray(poses[1:], np.float32))
    second = m.register_records(descs, T, **kw)
    fresh = tr._gpu_map(gpu_ctx, cell, scans, poses)
    tr._same_records(second, fresh.register_records(descs, T, **kw), "after an add")
    assert (tr._bytes(first) != tr._bytes(second)).any()
    wide = m.register_records(descs, T, sigma_min=0.05, **kw)
    fresh2 = tr._gpu_map(gpu_ctx, cell, scans, poses)
    tr._same_records(wide, fresh2.register_records(descs, T, sigma_min=0.05, **kw), "another sigma_min")
    assert (tr._bytes(wide) != tr._bytes(second)).any()
    m.register_records(descs, T, max_iters=4)                         # a centre-only call, then the other neighbourhood, then this one again
    m.register_records(descs, T, max_iters=4, neighbours=34 - neighbours)
    tr._same_records(m.register_records(descs, T, **kw), second, "and back")
    m.remove(scans[1:], np.asarray(poses[1:], np.float32))
    tr._same_records(m.register_records(descs, T, **kw), first, "after a remove")
    for x in (m, fresh, fresh2):
        x.close()


def test_27_cells_take_the_passes_of_the_model_to_the_pose_of_the_model(gpu_ctx):
    """scene() under 27 cells: every start is CONVERGED, in the number of passes the model takes (fewer than centre-only's: test_map_register_neighbours_model.py),
    and the device's pose lies within 4 x the largest difference between the model and the same model summing its rows in REVERSE order, measured here, plus the
    rounding of the record's float32 entries -- the device and the model differ in the order of their sums only."""
    s, m = tr._scene_map(gpu_ctx)
    model, rev = nc.scene_model(27, "forward"), nc.scene_model(27, "reverse")
    assert all(r["status"] == rm.CONVERGED for r in model) and all(r["status"] == rm.CONVERGED for r in rev)
    measured = max(cs.pose_diff(a["pose64"], b["pose64"]) for a, b in zip(model, rev))
    print("27 cells, model forward against reverse: largest pose difference %.3e" % measured)
    assert measured > 0.0
    got = m.register([h[0] for h in s["held"]], np.stack([T0 for _, T0 in s["starts"]]), scan_of=[i for i, _ in s["starts"]], neighbours=27, **s["params"])
    for k, (g, w) in enumerate(zip(got, model)):
        want = np.eye(4); want[:3, :3] = w["pose64"][0]; want[:3, 3] = w["pose64"][1]
        half_ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) / 2
        diff = np.abs(g["pose"].astype(np.float64) - want)
        print("start %d: device %d passes (%d accepted), model %d (%d); |device - model| largest %.3e; cost %.6f against %.6f" %
              (k, g["iterations"], g["accepted"], w["iterations"], w["accepted"], diff.max(), g["cost"], w["cost"]))
        assert g["status"] == rm.CONVERGED, (k, g)
        assert g["iterations"] == w["iterations"] and g["accepted"] == w["accepted"], (k, g["iterations"], w["iterations"])
        assert (diff <= 4 * measured + half_ulp).all(), (k, diff, 4 * measured)
        assert g["cost"] < g["cost_start"] and g["rows_matched"] == w["rows_matched"] and g["rows_scored"] == w["rows_scored"]
    m.close()
