"""The keyframe store (include/icet_hip.h: icet_keyframe_store_*): keyframes built once into slots the caller chooses,
kept bit for bit whatever else runs on the context, and registered / scored against through the indexed kernels.  Every registration must carry
the bits icet_solve_batch_device gives for the expanded pair (the scan put into the slot, scan2[r], x0[r])."""
import ctypes as C

import numpy as np
import pytest
import torch

NEW_SYMBOLS = ("icet_keyframe_store_create", "icet_keyframe_store_destroy", "icet_keyframe_store_last_error", "icet_keyframe_store_reserve",
               "icet_keyframe_store_put_device", "icet_keyframe_store_register_device", "icet_keyframe_store_register_scored_device",
               "icet_keyframe_store_score_device", "icet_keyframe_store_debug_fetch")


def test_store_entry_points_are_exported_and_refuse_a_null_store_or_context():
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "icet_keyframe_store_last_error" in api._NON_STATUS
    p = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    h = C.c_void_p(1234)
    assert lib.icet_keyframe_store_create(None, C.byref(p), 4, C.byref(h)) == api.ICET_ERR_BAD_ARG
    assert not h.value                                                  # *out is cleared even on refusal
    idx = (C.c_int32 * 1)(0)
    assert lib.icet_keyframe_store_destroy(None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_last_error(None) == b"null store"
    assert lib.icet_keyframe_store_reserve(None, 8) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_put_device(None, 1, idx, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_register_device(None, C.byref(p), 1, idx, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_register_scored_device(None, C.byref(p), 1, idx, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_keyframe_store_score_device(None, C.byref(p), 1, idx, None, None, None) == api.ICET_ERR_BAD_ARG
    out = np.zeros(4, np.int32)
    assert lib.icet_keyframe_store_debug_fetch(None, 0, 0, out.ctypes.data, 1) == api.ICET_ERR_BAD_ARG


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

DEV = torch.device("cuda", 0)


def _dev(a):
    """numpy N x 3 -> float32 (3, N) on the device (column-major N x 3, ld = N)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).to(DEV)


def _desc(t, n=None):
    return (t.data_ptr(), t.shape[1] if n is None else int(n), t.shape[1])


def _keyframes(frames, sample_pc):
    """Four keyframes of three sizes (two synthetic batch pairs, the real frame pair, the reference's sample pair) and each one's partner scan."""
    from icet_amd import lidar_sim as ls
    p0, p1 = ls.make_batch_pair(0, device=DEV), ls.make_batch_pair(1, device=DEV)
    kf = [p0[0], p1[0], _dev(frames[0]), _dev(sample_pc[0])]
    partner = [p0[1], p1[1], _dev(frames[1]), _dev(sample_pc[1])]
    return kf, partner


def _registrations(partner, kf_index, seed):
    """Registration r: the partner of keyframe kf_index[r] -- every third one only its first part (n < ld) -- from a small random X0."""
    rng = np.random.default_rng(seed)
    d2 = []
    for r, k in enumerate(kf_index):
        t = partner[k]
        d2.append(_desc(t, t.shape[1] * 2 // 3 if r % 3 == 2 else None))
    x0 = np.zeros((len(kf_index), 6), np.float32)
    x0[:, 0] = rng.uniform(-0.05, 0.05, len(kf_index)); x0[:, 1] = rng.uniform(-0.03, 0.03, len(kf_index)); x0[:, 5] = rng.uniform(-0.005, 0.005, len(kf_index))
    x0[0] = 0.0
    return d2, x0


def _mapping(n_regs, n_kf, seed):
    """Every keyframe used, repeats, out of order."""
    rng = np.random.default_rng(seed)
    m = np.concatenate([np.arange(n_kf)[::-1], rng.integers(0, n_kf, max(0, n_regs - n_kf))])[:n_regs]
    return [int(v) for v in m]


def _expanded(d1, d2, x0, prm):
    """icet_solve_batch_device on the expanded pairs (scan-1 descriptors d1[r]), in a context of its own."""
    import icet_amd
    ref = icet_amd.Context(0)
    out = torch.zeros((len(d1), 48), dtype=torch.float32, device=DEV)
    xd = torch.from_numpy(x0).to(DEV)
    torch.cuda.synchronize()
    ref.solve_batch_device(d1, d2, prm, out.data_ptr(), xd.data_ptr())
    ref.sync(); ref.close()
    return out


def _store_regs(store, slots, d2, x0, prm):
    out = torch.full((len(slots), 48), float("nan"), dtype=torch.float32, device=DEV)
    xd = torch.from_numpy(x0).to(DEV)
    torch.cuda.synchronize()
    store.register_device(slots, d2, prm, out.data_ptr(), xd.data_ptr())
    store._ctx.sync()
    return out


def _bytes(store, slot):
    return (store.debug_fetch(slot, "n_slots"), store.debug_fetch(slot, "hot").copy(), store.debug_fetch(slot, "fit").copy(),
            store.debug_fetch(slot, "slot_of_voxel").copy())


def _same_bytes(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


SCATTER = [7, 0, 130, 199]                                              # slot of keyframe k


def _filled_store(ctx, kf, flags=0, capacity=200):
    import icet_amd
    st = icet_amd.KeyframeStore(ctx, capacity, flags=flags)
    st.put_device([SCATTER[0]], [_desc(kf[0])])                         # two puts: 1 scan, then 3
    st.put_device(SCATTER[1:], [_desc(t) for t in kf[1:]])
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("store_flag,call_flag,n_regs", [("", "", 5), ("", "", 300), ("", "REJECT_MOVING", 6), ("", "DOUBLE_W", 6), ("", "ROUNDTRIP_SCAN2", 6),
                                                         ("", "ROUNDTRIP_SCAN2", 70), ("TRUE_SORT", "", 6), ("HALF_GAP_BOUNDS", "", 6), ("HALF_GAP_BOUNDS", "", 80)])
def test_store_registrations_carry_the_bits_of_the_expanded_batch(frames, sample_pc, store_flag, call_flag, n_regs):
    import icet_amd
    from icet_amd import api
    kf, partner = _keyframes(frames, sample_pc)
    sf = getattr(api, "FLAG_" + store_flag) if store_flag else 0
    cf = getattr(api, "FLAG_" + call_flag) if call_flag else 0
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, sf | cf)
    kf_index = _mapping(n_regs, 4, 11 + n_regs)
    d2, x0 = _registrations(partner, kf_index, 12)
    ref = _expanded([_desc(kf[k]) for k in kf_index], d2, x0, prm)
    assert bool(torch.isfinite(ref).all())
    ctx = icet_amd.Context(0)
    st = _filled_store(ctx, kf, flags=sf)
    slots = [SCATTER[k] for k in kf_index]
    for _ in range(3):                                                  # eager, captured + replayed, replayed (small batches)
        assert torch.equal(_store_regs(st, slots, d2, x0, prm), ref)
    st.close(); ctx.close()


def _check_tables(st, slot, aux, n=25):
    """The slot's records against the side tables of Context.solve(..., aux=True) on the same scan 1, bit for bit."""
    b, n1, hf = aux["cluster_bounds"], aux["n1_raw"], aux["has_fit"]
    vox = np.nonzero((n1 > n) & (b[:, 5] > 1) & (hf != 0))[0]           # the active voxels, in voxel order
    ns, hot, fit, sov = _bytes(st, slot)
    assert ns == vox.size and ns > 0
    expect_sov = np.full(n1.size, -1, np.int16); expect_sov[vox] = np.arange(vox.size)
    assert np.array_equal(sov, expect_sov)
    hotf, hoti = hot.view(np.float32), hot.view(np.int32)
    assert np.array_equal(hotf[:, 0:6], b[vox]) and np.array_equal(hotf[:, 6:9], aux["mu1"][vox]) and np.array_equal(hoti[:, 9], vox)
    fitf, fiti = fit.view(np.float32), fit.view(np.int32)
    assert np.array_equal(fitf[:, 0:3], aux["mu1"][vox])
    sig = aux["sigma1"].reshape(-1, 9)[vox][:, [0, 1, 2, 4, 5, 8]]
    assert np.array_equal(fitf[:, 3:9], sig / (n1[vox] - 1).astype(np.float32)[:, None])
    M = (aux["l_diag"][vox][:, :, None] * aux["evecs1"][vox]).reshape(-1, 9)     # diag(l_diag) . evecs1, row-major
    assert np.array_equal(fitf[:, 9:18], M)
    assert np.array_equal(fiti[:, 18], n1[vox]) and np.array_equal(fiti[:, 19], vox)


@pytest.mark.gpu
def test_store_tables_are_the_keyframe_tables(gpu_ctx, frames, sample_pc):
    import icet_amd
    kf, _ = _keyframes(frames, sample_pc)
    ctx = icet_amd.Context(0)
    st = icet_amd.KeyframeStore(ctx, 200)
    st.put_device([3], [_desc(kf[2])]); st.put_device([5], [_desc(kf[3])])
    # the same scans as one of 64 (the four keyframes 16 times over, in slots 100 .. 163)
    st.put_device(list(range(100, 164)), [_desc(kf[k % 4]) for k in range(64)])
    for slot, (a, b) in ((3, frames), (5, sample_pc)):
        aux = gpu_ctx.solve(a, b, 1, np.zeros(6, np.float32), 24, 75, aux=True)["aux"]
        _check_tables(st, slot, aux)
    alone = {2: _bytes(st, 3), 3: _bytes(st, 5)}
    for s in range(100, 164):
        if s % 4 in (2, 3):
            assert _same_bytes(_bytes(st, s), alone[s % 4]), s
    st.close(); ctx.close()


@pytest.mark.gpu
def test_slots_survive_everything_else_on_the_context(frames, sample_pc):
    import icet_amd
    from icet_amd import api
    kf, partner = _keyframes(frames, sample_pc)
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    kf_index = _mapping(5, 4, 41)
    d2, x0 = _registrations(partner, kf_index, 42)
    ref = _expanded([_desc(kf[k]) for k in kf_index], d2, x0, prm)
    ctx = icet_amd.Context(0)
    st = _filled_store(ctx, kf)
    slots = [SCATTER[k] for k in kf_index]
    before = {s: _bytes(st, s) for s in SCATTER}
    assert torch.equal(_store_regs(st, slots, d2, x0, prm), ref)

    def unchanged(what):
        for s in SCATTER:
            assert _same_bytes(_bytes(st, s), before[s]), (what, s)
        assert torch.equal(_store_regs(st, slots, d2, x0, prm), ref), what

    out = torch.zeros((4, 48), dtype=torch.float32, device=DEV)
    ctx.solve_batch_device([_desc(t) for t in kf], [_desc(t) for t in partner], prm, out.data_ptr()); ctx.sync()
    unchanged("whole solve")
    ctx.keyframe_device([_desc(t) for t in kf[:2]], prm)
    ctx.register_indexed_device([1, 0, 1], [_desc(partner[1]), _desc(partner[0]), _desc(partner[1])], prm, out.data_ptr()); ctx.sync()
    unchanged("keyframe + indexed call")
    st.put_device([50, 51], [_desc(kf[3]), _desc(kf[0])]); ctx.sync()
    unchanged("put into other slots")
    ctx.reserve(api.Params(7, 48, 150, 25, 0.1, 0.1, 0), 8, 2_000_000, 0)  # a finer grid and more scan-1 points: the keyframe side grows
    unchanged("icet_reserve")
    st.reserve(1000)
    unchanged("store reserve")
    st2 = icet_amd.KeyframeStore(ctx, 16)
    st2.put_device([0, 1, 2, 3], [_desc(t) for t in kf[::-1]]); st2.put_device([15], [_desc(kf[2])]); ctx.sync()
    unchanged("a second store's puts")
    st2.close(); st.close(); ctx.close()


@pytest.mark.gpu
def test_replace_and_device_row_counts(frames, sample_pc):
    import icet_amd
    from icet_amd import api
    kf, partner = _keyframes(frames, sample_pc)
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    ctx = icet_amd.Context(0)
    st = _filled_store(ctx, kf)
    # a put over an occupied slot: slot 7 held keyframe 0, now keyframe 3
    st.put_device([7], [_desc(kf[3])])
    d2, x0 = _registrations(partner, [3, 3, 3], 51)
    assert torch.equal(_store_regs(st, [7, 199, 7], d2, x0, prm), _expanded([_desc(kf[3])] * 3, d2, x0, prm))
    # device-side row counts: the put of the truncated scan
    m = kf[2].shape[1] * 2 // 3
    rows = torch.tensor([m, kf[3].shape[1] // 2], dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st.put_device([9, 11], [_desc(kf[2]), _desc(kf[3])], d_rows_ptr=rows.data_ptr())
    st.put_device([10, 12], [_desc(kf[2], m), _desc(kf[3], kf[3].shape[1] // 2)])
    assert _same_bytes(_bytes(st, 9), _bytes(st, 10)) and _same_bytes(_bytes(st, 11), _bytes(st, 12))
    d2, x0 = _registrations(partner, [2, 2], 52)
    assert torch.equal(_store_regs(st, [9, 10], d2, x0, prm), _expanded([_desc(kf[2], m)] * 2, d2, x0, prm))
    st.close(); ctx.close()


@pytest.mark.gpu
def test_graph_replays_follow_the_keyframe_source(frames, sample_pc):
    """Calls of the same shapes and buffers alternate between the context's parked keyframe, store A, store B and store A after it grew: with option
    "graph" on (captures and replays) every call gives the bits of the same call with "graph" 0 and of the expanded batch."""
    import icet_amd
    from icet_amd import api
    kf, partner = _keyframes(frames, sample_pc)
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    d2, x0 = _registrations(partner, [0, 1, 2, 3], 61)
    order = {"ctx": [0, 1, 2, 3], "A": [0, 1, 2, 3], "B": [3, 2, 1, 0]}  # the keyframe that slot / index r holds
    refs = {k: _expanded([_desc(kf[j]) for j in v], d2, x0, prm) for k, v in order.items()}
    seq = ["ctx", "ctx", "ctx", "A", "A", "A", "B", "B", "B", "ctx", "A", "B", "A", "grow", "A", "A", "A", "ctx", "B", "A"]
    results = {}
    for graph in (-1, 0):
        ctx = icet_amd.Context(0)
        ctx.set_option("graph", graph)
        a, b = icet_amd.KeyframeStore(ctx, 8), icet_amd.KeyframeStore(ctx, 8)
        a.put_device([0, 1, 2, 3], [_desc(t) for t in kf]); b.put_device([0, 1, 2, 3], [_desc(t) for t in kf[::-1]])
        ctx.keyframe_device([_desc(t) for t in kf], prm)
        out = torch.zeros((4, 48), dtype=torch.float32, device=DEV)
        xd = torch.from_numpy(x0).to(DEV)
        got = []
        for src in seq:
            if src == "grow":
                a.reserve(64); continue
            out.fill_(float("nan")); torch.cuda.synchronize()
            if src == "ctx":
                ctx.register_indexed_device([0, 1, 2, 3], d2, prm, out.data_ptr(), xd.data_ptr())
            else:
                (a if src == "A" else b).register_device([0, 1, 2, 3], d2, prm, out.data_ptr(), xd.data_ptr())
            ctx.sync()
            got.append(out.clone())
            assert torch.equal(got[-1], refs[src]), (graph, len(got), src)
        # puts of <= 8 scans with the same scan buffers into different slots (the build replays its graph): each lands in its own slots
        for s0 in (10, 12, 14):
            a.put_device([s0, s0 + 1], [_desc(kf[0]), _desc(kf[1])])
        for s0 in (12, 14):
            assert _same_bytes(_bytes(a, s0), _bytes(a, 10)) and _same_bytes(_bytes(a, s0 + 1), _bytes(a, 11))
        assert not _same_bytes(_bytes(a, 14), _bytes(a, 15))
        dd, xx = _registrations(partner, [0, 1], 62)
        assert torch.equal(_store_regs(a, [14, 15], dd, xx, prm), _expanded([_desc(kf[0]), _desc(kf[1])], dd, xx, prm))
        results[graph] = got
        a.close(); b.close(); ctx.close()
    assert all(torch.equal(x, y) for x, y in zip(results[-1], results[0]))


def _score_rec(t):
    from icet_amd import api
    return np.frombuffer(t.cpu().numpy().tobytes(), api.SCORE_DTYPE)


@pytest.mark.gpu
def test_store_scores_and_best_match(frames, sample_pc):
    import icet_amd
    from icet_amd import api
    kf, partner = _keyframes(frames, sample_pc)
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, api.FLAG_REJECT_MOVING)
    kf_index = _mapping(7, 4, 71)
    d2, x0 = _registrations(partner, kf_index, 72)
    xd = torch.from_numpy(x0).to(DEV)
    ctx = icet_amd.Context(0)
    st = _filled_store(ctx, kf)
    ctx.keyframe_device([_desc(t) for t in kf], prm)                   # (after the puts: a put un-parks the context's keyframe)
    slots = [SCATTER[k] for k in kf_index]
    for rep in range(2):                                                # eager, then captured
        o1 = torch.zeros((7, 48), dtype=torch.float32, device=DEV); s1 = torch.zeros((7, 8), dtype=torch.int32, device=DEV)
        o2 = torch.zeros_like(o1); s2 = torch.zeros_like(s1); s3 = torch.zeros_like(s1); s4 = torch.zeros_like(s1)
        torch.cuda.synchronize()
        ctx.register_indexed_scored_device(kf_index, d2, prm, o1.data_ptr(), s1.data_ptr(), xd.data_ptr())
        st.register_scored_device(slots, d2, prm, o2.data_ptr(), s2.data_ptr(), xd.data_ptr())
        ctx.score_indexed_device(kf_index, d2, prm, xd.data_ptr(), s3.data_ptr())
        st.score_device(slots, d2, prm, xd.data_ptr(), s4.data_ptr())
        ctx.sync()
        assert torch.equal(o1, o2) and torch.equal(s1, s2) and torch.equal(s3, s4)
        assert int(_score_rec(s2)["voxels"].min()) > 0
    # the loop-closure check: the sample pair's scan 2 against slots holding the real scan 1, the sample scan 1 and a synthetic one, four starts each
    a, b = sample_pc
    cand = [SCATTER[2], SCATTER[3], SCATTER[0]]
    slot_index = [s for s in cand for _ in range(4)]
    X0 = np.zeros((12, 6), np.float32); X0[:, 0] = [0.0, 0.2, 0.4, 0.6] * 3
    res = st.best_match(b, slot_index, X0, 12)
    host = api.select_best(res["score"], np.zeros(12, np.int32), 1)[0]
    sc = np.zeros(12, api.SCORE_DTYPE)
    for k in ("chi2", "chi2_per_voxel", "voxels", "points_in", "points", "overlap"):
        sc[k] = res["score"][k]
    d_sc = torch.from_numpy(sc.view(np.int32).reshape(12, 8).copy()).to(DEV)
    d_best = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.select_best_device(np.zeros(12, np.int32), 1, d_sc.data_ptr(), d_best.data_ptr()); ctx.sync()
    assert res["best"] == host == int(d_best.cpu()[0]) and res["best"] >= 0
    assert res["slot"] == slot_index[res["best"]] and np.array_equal(res["X"], res["X_all"][res["best"]])
    # each registration of the query carries the bits of the single-pair solve from its start
    single = ctx.solve_indexed([frames[0], a, kf[0].T.cpu().numpy()], [b] * 12, [k // 4 for k in range(12)], 12, X0=X0)
    assert np.array_equal(res["X_all"], single["X"])
    st.close(); ctx.close()


@pytest.mark.gpu
def test_refusals_leave_slots_and_parked_keyframe_alone(frames, sample_pc):
    import icet_amd
    from icet_amd import api
    lib = api.load_library()
    kf, partner = _keyframes(frames, sample_pc)
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    ctx = icet_amd.Context(0)
    st = _filled_store(ctx, kf)
    ctx.keyframe_device([_desc(t) for t in kf[:3]], prm)
    xd = torch.zeros((3, 6), dtype=torch.float32, device=DEV); xd[:, 0] = torch.tensor([0.0, 0.02, -0.01], device=DEV)

    def register():
        out = torch.zeros((3, 48), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        ctx.register_device([_desc(t) for t in partner[:3]], prm, out.data_ptr(), xd.data_ptr()); ctx.sync()
        return out

    parked = register()
    before = {s: _bytes(st, s) for s in SCATTER}
    out = torch.zeros((2, 48), dtype=torch.float32, device=DEV); sc = torch.zeros((2, 8), dtype=torch.int32, device=DEV)
    d2 = [_desc(partner[0]), _desc(partner[1])]

    def refused(status, fn, *a, **k):
        with pytest.raises(icet_amd.IcetError) as e:
            fn(*a, **k)
        assert e.value.status == status, (e.value, fn)

    B = api.ICET_ERR_BAD_ARG
    refused(B, st.put_device, [200], [_desc(kf[0])])                    # slot out of range
    refused(B, st.put_device, [-1], [_desc(kf[0])])
    refused(B, st.put_device, [5, 5], [_desc(kf[0]), _desc(kf[1])])     # a slot named twice
    refused(B, st.put_device, [7, 8], [_desc(kf[0]), (kf[1].data_ptr(), kf[1].shape[1] + 1, kf[1].shape[1])])     # n > ld: a bad descriptor
    one = (C.c_int32 * 1)(3)
    assert lib.icet_keyframe_store_put_device(st._h, -1, one, None, None) == B                        # n < 0
    refused(B, st.register_device, [7, 8], d2, prm, out.data_ptr())      # slot 8 is empty
    refused(B, st.register_device, [7, 200], d2, prm, out.data_ptr())    # out of range
    refused(B, st.register_device, [7, 0], d2, api.Params(7, 48, 150, 25, 0.1, 0.1, 0), out.data_ptr())     # shape: grid
    refused(B, st.register_device, [7, 0], d2, api.Params(7, 24, 75, 20, 0.1, 0.1, 0), out.data_ptr())     # shape: n
    refused(B, st.register_scored_device, [7, 0], d2, api.Params(7, 24, 75, 25, 0.1, 0.1, api.FLAG_TRUE_SORT), out.data_ptr(), sc.data_ptr())
    refused(B, st.score_device, [7, 9], d2, prm, xd.data_ptr(), sc.data_ptr())
    refused(B, st.debug_fetch, 8, "n_slots")
    ctx.set_option("keep", 1)
    refused(api.ICET_ERR_UNSUPPORTED, st.register_device, [7, 0], d2, prm, out.data_ptr())
    ctx.set_option("keep", 0)
    with pytest.raises(icet_amd.IcetError) as e:                        # a grid above the voxel limit
        icet_amd.KeyframeStore(ctx, 4, num_bins_phi=101, num_bins_theta=100)
    assert e.value.status == api.ICET_ERR_UNSUPPORTED
    assert lib.icet_keyframe_store_register_device(st._h, C.byref(prm), -1, one, None, None, None) == B
    st.put_device([], [])                                                # n == 0: nothing
    st.register_device([], [], prm, out.data_ptr())
    st.reserve(100)                                                      # smaller: nothing
    for s in SCATTER:
        assert _same_bytes(_bytes(st, s), before[s]), s
    assert torch.equal(register(), parked)                              # the context's parked keyframe is still parked, with its bits
    st.close(); ctx.close()


def _node_results(node, seq, between=None):
    res = []
    for k, s in enumerate(seq):
        res.append(node.push(s))
        if between:
            between(k)
    return res


@pytest.mark.gpu
def test_store_beside_a_pipelined_node_and_a_second_grid(frames, sample_pc):
    import icet_amd
    from icet_amd import api
    from icet_amd import lidar_sim as ls
    seq = [s.T.contiguous().numpy() for s in ls.make_sequence(6, motion=(0.25, 0.02, 0.005, 0.001, -0.001, 0.006))]
    kf, partner = _keyframes(frames, sample_pc)
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    alone_ctx = icet_amd.Context(0)
    nd = api.Node(alone_ctx, **api.ODOMETRY_NODE)
    alone = _node_results(nd, seq)
    nd.close(); alone_ctx.close()
    ctx = icet_amd.Context(0)
    st = icet_amd.KeyframeStore(ctx, 32)
    nd = api.Node(ctx, **api.ODOMETRY_NODE)
    d2, x0 = _registrations(partner, [0, 1, 2, 3, 2], 81)
    ref = _expanded([_desc(kf[k]) for k in [0, 1, 2, 3, 2]], d2, x0, prm)

    def between(k):
        st.put_device([4 * k + j for j in range(4)], [_desc(t) for t in kf])
        base = 4 * k
        assert torch.equal(_store_regs(st, [base, base + 1, base + 2, base + 3, base + 2], d2, x0, prm), ref), k

    shared = _node_results(nd, seq, between)
    for r, (a, b) in enumerate(zip(alone, shared)):
        for key in ("X", "pred_stds", "pose", "quat"):
            assert np.array_equal(a[key], b[key]), (r, key)
        assert a["solved"] == b["solved"] and a["n_kept"] == b["n_kept"]
    nd.close(); st.close()
    # two stores on one context, 75 x 24 and 150 x 48, calls interleaved
    fine = api.Params(7, 48, 150, 25, 0.1, 0.1, 0)
    ref_fine = _expanded([_desc(kf[k]) for k in [0, 1, 2, 3, 2]], d2, x0, fine)
    s1, s2 = icet_amd.KeyframeStore(ctx, 8), icet_amd.KeyframeStore(ctx, 8, num_bins_phi=48, num_bins_theta=150)
    for it in range(2):
        s1.put_device([0, 1, 2, 3], [_desc(t) for t in kf])
        s2.put_device([4, 5, 6, 7], [_desc(t) for t in kf])
        for _ in range(2):
            assert torch.equal(_store_regs(s1, [0, 1, 2, 3, 2], d2, x0, prm), ref), it
            assert torch.equal(_store_regs(s2, [4, 5, 6, 7, 6], d2, x0, fine), ref_fine), it
    s1.close(); s2.close(); ctx.close()
