"""The four ways into the store's closure pipeline -- icet_keyframe_store_close_device, _close_appearance_device, _close_coarse_device with poses and
without (include/icet_hip.h; DESIGN.md sections 16 - 18) -- held to the same three cases at one small shape: a store without any keyframe, a store with
fewer eligible slots than K (every query carries a padding candidate; the records against the calls a caller would chain by hand, byte for byte; a padding
registration's x0 and result rows zero and its score the one of a registration without voxels: zeros and chi2_per_voxel = +inf), and
the refusals they share, after which a correct call still gives the same records."""
import numpy as np
import pytest
import torch

import closure_model as cm
import coarse_model as co

DEV = torch.device("cuda", 0)
VARIANTS = ["pose", "appearance", "coarse_pose", "coarse_appearance"]
BINS_PHI, BINS_THETA, N_MIN = 8, 16, 5
Q, K, S, RUNLEN = 2, 3, 2, 2
SLOTS = [2, 0]
KF_STAMPS = np.array([10, 20], np.int64)
Q_STAMPS = np.array([500, 510], np.int64)
OFFSETS = np.array([[0, 0, 0, 0, 0, 0], [0.05, -0.02, 0, 0, 0, 0.005]], np.float32)
RADIUS = 50.0                                                           # metres by pose (both keyframes in reach); by appearance the bound is +inf
YAW_STEP = np.pi / 120


def _desc(t):
    return (t.data_ptr(), t.shape[1], t.shape[1])


def _recs(t):
    from icet_amd import api
    return np.frombuffer(t.cpu().numpy().tobytes(), api.CLOSURE_DTYPE).copy()


def _scores(t):
    from icet_amd import api
    return np.frombuffer(t.cpu().numpy().tobytes(), api.SCORE_DTYPE).copy()


@pytest.fixture(scope="module")
def small():
    """Two keyframes 1.5 m apart in scene 2000 and two revisits near them, at 16 x 128 rays (about 2k points each), on the device."""
    import icet_amd
    from icet_amd import lidar_sim as ls
    scene = ls.make_scene(2000)
    kf_T = [cm.pose_yaw((-5.0 + 1.5 * k, -1.0 + 0.1 * k, 0.0), 0.05 * k) for k in range(2)]
    live_T = [cm.pose_yaw((kf_T[k][0, 3] + o[0], kf_T[k][1, 3] + o[1], 0.0), 0.05 * k + o[2]) for k, o in enumerate([(0.35, 0.20, 0.30), (-0.30, 0.30, 0.45)])]
    scan = lambda T, seed: ls.make_scan(scene, (T[:3, 3].astype(np.float64), T[:3, :3].astype(np.float64)), seed, rings=16, steps=128, device=DEV)
    d = dict(ctx=icet_amd.Context(0), kf=[scan(T, 100 + k) for k, T in enumerate(kf_T)], live=[scan(T, 200 + k) for k, T in enumerate(live_T)],
             kf_T=np.stack(kf_T), live_T=np.stack(live_T))
    torch.cuda.synchronize()
    yield d
    d["ctx"].close()


def _store(d, variant, filled):
    import icet_amd
    st = icet_amd.KeyframeStore(d["ctx"], 4, BINS_PHI, BINS_THETA, N_MIN)
    if variant != "pose" and variant != "coarse_pose":
        st.enable_appearance()
    if variant.startswith("coarse"):
        st.enable_coarse(64, 0.5)
    if filled:
        st.put_device(SLOTS, [_desc(t) for t in d["kf"]])
        if variant.endswith("pose"):
            st.set_pose(SLOTS, d["kf_T"], KF_STAMPS)
        else:
            st.set_stamp(SLOTS, KF_STAMPS)
    return st


def _search(st):
    return st.coarse_search(12, 1, YAW_STEP, True)


def _query(variant, n_starts=S):
    from icet_amd import api
    return api.ClosureQuery(RADIUS if variant.endswith("pose") else float("inf"), K, 0, n_starts, float("inf"), 0, 0)


def _call(d, st, variant, rec_ptr, params=None, query=None, descs=None, offsets=OFFSETS, cand=None, x0=None, out=None, sc=None, match=None):
    """The variant's one-call query, asynchronous."""
    params = st._params(RUNLEN, 0) if params is None else params
    query = _query(variant) if query is None else query
    descs = [_desc(t) for t in d["live"]] if descs is None else descs
    ptr = lambda t: t.data_ptr() if t is not None else None
    by_pose = variant.endswith("pose")
    poses, stamps = (d["live_T"], Q_STAMPS) if by_pose else (None, None)
    if variant == "pose":
        st.close_device(descs, poses, stamps, params, query, rec_ptr, offsets, ptr(cand), ptr(x0), ptr(out), ptr(sc))
    elif variant == "appearance":
        st.close_appearance_device(descs, stamps, params, query, rec_ptr, offsets, ptr(cand), ptr(x0), ptr(out), ptr(sc))
    else:
        st.close_coarse_device(descs, poses, stamps, params, query, _search(st), rec_ptr, offsets, ptr(cand), ptr(x0), ptr(out), ptr(sc), ptr(match))


def _close(d, st, variant, fill=0):
    """One call with every output asked for, the caller's buffers pre-filled with the byte `fill` (cand with -7)."""
    from icet_amd import api
    R = Q * K * S
    rec = torch.full((Q, api.CLOSURE_DTYPE.itemsize), 0x55, dtype=torch.uint8, device=DEV)
    cand = torch.full((Q, K), -7, dtype=torch.int32, device=DEV)
    x0 = torch.full((R, 24), fill, dtype=torch.uint8, device=DEV).view(torch.float32)
    out = torch.full((R, 192), fill, dtype=torch.uint8, device=DEV).view(torch.float32)
    sc = torch.full((R, 32), fill, dtype=torch.uint8, device=DEV).view(torch.int32)
    match = torch.full((Q * K, 32), 0x77, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    _call(d, st, variant, rec.data_ptr(), cand=cand, x0=x0, out=out, sc=sc, match=match)
    d["ctx"].sync()
    return dict(rec=_recs(rec), cand=cand.cpu().numpy(), x0=x0.cpu().numpy(), out=out.cpu().numpy(), score=_scores(sc),
                match=np.frombuffer(match.cpu().numpy().tobytes(), api.COARSE_MATCH_DTYPE).reshape(Q, K))


def _manual(d, st, variant):
    """What a caller chains by hand: candidates_*_device, coarse_align_device for the coarse variants, register_scored_device on the real candidates,
    icet_select_best_device, and the record filled in on the host.  Returns (records, cand, x0 of every registration, live registrations, out, score)."""
    from icet_amd import api
    ctx = d["ctx"]
    by_pose, coarse = variant.endswith("pose"), variant.startswith("coarse")
    descs = [_desc(t) for t in d["live"]]
    cand_t = torch.full((Q, K), -7, dtype=torch.int32, device=DEV)
    base_t = torch.full((Q, K, 6), float("nan"), dtype=torch.float32, device=DEV)
    dist_t = torch.zeros((Q, K), dtype=torch.float32, device=DEV); shift_t = torch.full((Q, K), -7, dtype=torch.int32, device=DEV)
    x0c_t = torch.full((Q, K, 6), float("nan"), dtype=torch.float32, device=DEV)
    match_t = torch.full((Q * K, 32), 0x77, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    query = _query(variant, 1)
    if by_pose:
        st.candidates_device(d["live_T"], Q_STAMPS, query, cand_t.data_ptr(), base_t.data_ptr())
    else:
        st.candidates_appearance_device(descs, None, query, cand_t.data_ptr(), dist_t.data_ptr(), shift_t.data_ptr(), base_t.data_ptr())
    if coarse:
        st.coarse_align_device(descs, K, cand_t.data_ptr(), base_t.data_ptr(), _search(st), x0c_t.data_ptr(), match_t.data_ptr())
    ctx.sync()
    cand = cand_t.cpu().numpy()
    start = (x0c_t if coarse else base_t).cpu().numpy()
    match = np.frombuffer(match_t.cpu().numpy().tobytes(), api.COARSE_MATCH_DTYPE).reshape(Q, K)
    x0 = np.zeros((Q * K * S, 6), np.float32)
    for r in range(Q * K * S):
        if cand.reshape(-1)[r // S] >= 0:
            x0[r] = start.reshape(-1, 6)[r // S] + OFFSETS[r % S]         # one float32 add
    live = [r for r in range(Q * K * S) if cand.reshape(-1)[r // S] >= 0]
    xl = torch.from_numpy(x0[live]).to(DEV)
    out2 = torch.zeros((len(live), 48), dtype=torch.float32, device=DEV); sc2 = torch.zeros((len(live), 8), dtype=torch.int32, device=DEV)
    best = torch.full((Q,), -9, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st.register_scored_device([int(cand.reshape(-1)[r // S]) for r in live], [descs[r // (K * S)] for r in live], st._params(RUNLEN, 0), out2.data_ptr(), sc2.data_ptr(),
                              xl.data_ptr())
    ctx.select_best_device(np.array([r // (K * S) for r in live], np.int32), Q, sc2.data_ptr(), best.data_ptr())
    ctx.sync()
    out2, sc2, best = out2.cpu().numpy(), _scores(sc2), best.cpu().numpy()
    want = np.zeros(Q, api.CLOSURE_DTYPE)
    for i in range(Q):
        want[i]["n_candidates"] = int((cand[i] >= 0).sum())
        b = int(best[i])
        if b < 0:
            want[i]["slot"] = -1; want[i]["reg"] = -1
            continue
        r = live[b]; k = (r // S) % K
        slot = int(cand[i, k])
        want[i]["slot"] = slot; want[i]["reg"] = r; want[i]["accepted"] = 1; want[i]["stamp"] = st.debug_fetch(slot, "stamp")
        if by_pose:
            want[i]["d2"] = cm.dist2(d["live_T"][i][:3, 3], d["kf_T"][SLOTS.index(slot)][:3, 3].reshape(1, 3))[0]
        else:
            want[i]["d2"] = dist_t.cpu().numpy()[i, k]; want[i]["reserved0"] = shift_t.cpu().numpy()[i, k]
        want[i]["x0"] = x0[r]; want[i]["out"] = out2[b]; want[i]["score"] = sc2[b]
        if coarse:
            mk = match[i, k]
            want[i]["reserved1"] = (mk["score"], co.shift_code(int(mk["a"]), int(mk["b"]), int(mk["h"])))
    return want, cand, x0, live, out2, sc2


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_empty_store_padding_and_refusals_are_the_same_from_every_entry(small, variant):
    import icet_amd
    from icet_amd import api
    d = small
    ctx = d["ctx"]
    # 1 a store without any keyframe: ICET_OK, every record "none", the caller's out and score zeroed
    st = _store(d, variant, filled=False)
    res = _close(d, st, variant, fill=0x5A)
    rec = res["rec"]
    assert (rec["slot"] == -1).all() and (rec["reg"] == -1).all() and (rec["accepted"] == 0).all() and (rec["n_candidates"] == 0).all()
    assert not rec["out"].any() and not rec["x0"].any() and rec["score"].tobytes() == bytes(rec["score"].nbytes)
    assert res["out"].tobytes() == bytes(res["out"].nbytes) and res["score"].tobytes() == bytes(res["score"].nbytes)
    assert (res["cand"] == -1).all()
    st.close()
    # 2 two eligible slots, K = 3: every query has a padding candidate; the records are the manual path's, byte for byte
    st = _store(d, variant, filled=True)
    res = _close(d, st, variant, fill=0x5A)
    want, cand, x0, live, out2, sc2 = _manual(d, st, variant)
    rec = res["rec"]
    print(variant, "cand", res["cand"].tolist(), "slot", rec["slot"], "reg", rec["reg"], "voxels", res["score"]["voxels"])
    assert np.array_equal(res["cand"], cand) and (cand[:, :2] >= 0).all() and (cand[:, 2] == -1).all()
    assert res["x0"].tobytes() == x0.tobytes()
    assert np.array_equal(res["out"][live].view(np.uint32), out2.view(np.uint32)) and res["score"][live].tobytes() == sc2.tobytes()
    assert (want["slot"] >= 0).any()
    assert rec.tobytes() == want.tobytes(), [(n, rec[n], want[n]) for n in rec.dtype.names if rec[n].tobytes() != want[n].tobytes()]
    pad = [r for r in range(Q * K * S) if r not in live]
    assert len(pad) == Q * S
    for name in ("x0", "out"):
        assert res[name][pad].tobytes() == bytes(res[name][pad].nbytes), (name, res[name][pad])
    no_voxel = np.zeros(len(pad), api.SCORE_DTYPE); no_voxel["chi2_per_voxel"] = np.inf      # the score of a registration without voxels (include/icet_hip.h)
    assert res["score"][pad].tobytes() == no_voxel.tobytes(), res["score"][pad]
    # 3 the refusals every entry shares: the pose call's status from each; a refused call moved nothing, so a correct one still gives the records of 2
    rec_t = torch.zeros((Q, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    t0 = d["live"][0]
    refused = [(dict(query=_query(variant, 0), offsets=None), api.ICET_ERR_BAD_ARG),
               (dict(params=api.Params(RUNLEN, BINS_PHI + 1, BINS_THETA, N_MIN, 0.1, 0.1, 0)), api.ICET_ERR_BAD_ARG),
               (dict(descs=[(t0.data_ptr(), t0.shape[1], t0.shape[1] - 1), _desc(d["live"][1])]), api.ICET_ERR_BAD_ARG)]
    for kw, status in refused:
        with pytest.raises(icet_amd.IcetError) as e:
            _call(d, st, variant, rec_t.data_ptr(), **kw)
        assert e.value.status == status, (kw, e.value)
    ctx.set_option("keep", 1)
    try:
        with pytest.raises(icet_amd.IcetError) as e:
            _call(d, st, variant, rec_t.data_ptr())
        assert e.value.status == api.ICET_ERR_UNSUPPORTED
    finally:
        ctx.set_option("keep", 0)
    ctx.sync()
    assert not rec_t.cpu().numpy().any()                                # (no refused call wrote a record)
    again = _close(d, st, variant, fill=0x5A)
    assert again["rec"].tobytes() == rec.tobytes() and again["x0"].tobytes() == res["x0"].tobytes()
    assert again["out"].tobytes() == res["out"].tobytes() and again["score"].tobytes() == res["score"].tobytes()
    st.close()
