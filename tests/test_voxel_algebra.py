"""The middle of a Gauss-Newton iteration -- int64 words to moments, R_noise, dz, Rp, W, H_z, W H_z, the 21 + 6 sums and their reduction over slots, waves and
virtual blocks (gn_solve_body, icet_amd/csrc/icet_solve_body.h; the same expressions in k_gn_score) -- held to tests/solve_model.py, a restatement of the device's
own expression order fed with the device's own integer words and SlotFit records (icet_debug_gn_terms_device):
    one voxel per registration           H^T W H and H^T W dz are the model's terms BIT FOR BIT, under both weights, at X = 0 and at a pose with six non-zero components
    whole scans                          within  D 2^-24 sum |term|  of the exact sum of the model's terms (D from the source: the model's docstring), in the 256-thread
                                         form and the three launch forms of the canonical 512-slot tree, which agree with each other bit for bit
    the other consumers of the sums      the fused small-batch solve carries the hook's bits; X, pred_stds and cov are the oracle's 6 x 6 tail of the hook's sums; the
                                         score's voxels / points_in exactly and chi2 within one float32 ulp of the exact sum of the model's double terms
    the transform record                 sines and cosines correctly rounded, every R / J entry within 3 x 2^-24 sum |products|
    the moving-object gate               a kept axis beyond the cutoff contributes nothing, a pruned axis the model's bits
The CPU tests tie the model to the oracle's trace, to a float64 evaluation of the same formulas and to its own bounds, and check that the comparison catches a
dropped voxel, a doubled voxel, exchanged counts and a transposed index.

Measured on an MI355X (LABNOTES): see the notes' table of worst ratios; the assertions here are the derived bounds, not those figures."""
import functools

import numpy as np
import pytest
import torch

from tests import point_pass_model as pm
from tests import solve_model as sm
from tests import test_point_pass as tpp

GRID = tpp.GRID                                                       # 24 x 75, n = 10: ~350 active voxels, the 256-thread form
# V = 7200 > 4096: the canonical 512-slot form.  The scan covers 12 of the 48 polar bins: ~1500 active voxels (three virtual blocks) with n = 5; 40 x 110 (V = 4400)
# leaves 939 slots, and n = 10 on 48 x 150 fewer than 1024.
FINE = dict(bins_phi=48, bins_theta=150, n=5, thresh=0.3, buff=0.3)
GRIDS = dict(coarse=GRID, fine=FINE)
CASES = ("coarse@pose", "coarse@zero", "fine@pose")                    # grid @ where the solve is evaluated: the pair's true motion (six non-zero components), or X = 0 on the moved scan


def _pose(name):
    return np.asarray(tpp._synthetic()[2], np.float32) if name.endswith("@pose") else np.zeros(6, np.float32)


def _scans(name):
    """(scan 1, scan 2 as handed to the solve, pose X, grid): at `@pose` scan 2 is the raw scan and X the true motion; at `@zero` scan 2 was moved on the host."""
    a, b, xt = tpp._synthetic()
    g = GRIDS[name.split("@")[0]]
    return (a, b, _pose(name), g) if name.endswith("@pose") else (a, tpp._move(b, xt), _pose(name), g)


# ---- CPU: the cases as the model alone sees them (oracle keyframe, exact sums, emulated words) ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cpu_case(name):
    from oracle import pyoracle as po
    a, b, X, g = _scans(name)
    tr = po.solve(a, b, x0=X, runlen=1, trace=True, mode=po.DEVICE_ARITH, **g)["trace"]
    return _model_on_trace(tr, tpp._move(b, X) if X.any() else b, X, g)


def _model_on_trace(tr, moved, X, g):
    """The model on an oracle trace: words emulated from the exact point-pass reference of the moved scan 2, fit records from the trace's keyframe tables."""
    kf = pm.keyframe_tables(tr, g["n"])
    ref = pm.reference(moved, kf, g["bins_phi"], g["bins_theta"])
    act = np.nonzero(kf["active"])[0]
    rng = np.random.default_rng(23)
    words = np.zeros((act.size, 9), np.int64)
    for i, v in enumerate(act.tolist()):
        if v in ref.d:
            words[i] = pm.emulate_words(ref.d[v], rng)
    fit = sm.fit_from_tables(tr["mu1"], tr["sigma1"], tr["evecs1"], tr["Ldiag"], tr["n1_raw"], act)
    J = sm.xf_record(X)[16:43]
    args = (words, ref.n2[act], ref.m[act], fit, J)
    res = sm.voxel_terms(*args, flags=0, n=g["n"], iter=0)
    return dict(tr=tr, act=act, args=args, res=res, g=g, form=sm.form_of(g["bins_phi"] * g["bins_theta"]))


def _against_trace(c):
    tr, res = c["tr"], c["res"]
    used = c["act"][res["used"]]
    assert used.size > 50 and np.array_equal(used, np.nonzero(tr["used"][0])[0])
    H, gv = sm.mirror(sm.emulate_total(res["terms"], c["form"]))
    dH = float(np.abs(H - tr["HTWH"][0]).max() / np.abs(tr["HTWH"][0]).max()); dg = float(np.abs(gv - tr["HTWdz"][0]).max() / np.abs(tr["HTWdz"][0]).max())
    print("model against the trace: H^T W H %.2e, H^T W dz %.2e of the largest entry (%d voxels)" % (dH, dg, used.size))
    assert dH <= 2e-3 and dg <= 2e-3


def test_model_matches_the_oracle_trace_on_the_golden_frames(frames):
    from oracle import pyoracle as po
    a, b = frames
    g = dict(bins_phi=24, bins_theta=75, n=25, thresh=0.1, buff=0.1)
    tr = po.solve(a, b, runlen=1, trace=True, mode=po.DEVICE_ARITH, **g)["trace"]
    _against_trace(_model_on_trace(tr, b, np.zeros(6, np.float32), g))


@pytest.mark.parametrize("name", ["coarse@pose", "fine@pose"])
def test_model_matches_the_oracle_trace_at_a_nonzero_pose(name):
    """Signs and layout of J included: at the pair's true motion every one of the 27 Jacobian entries that can be non-zero is."""
    c = _cpu_case(name)
    assert np.count_nonzero(c["args"][4]) == 27 - len([k for k in sm.XF_ZERO if k >= 16])
    _against_trace(c)


@pytest.mark.parametrize("name", CASES)
def test_float32_terms_against_the_same_formulas_in_float64(name):
    """W held fixed to the model's own W9: the float32 terms lie within c 2^-24 sum |products| of the float64 evaluation, c = 19 / 16 (derived in the model)."""
    c = _cpu_case(name); res = c["res"]; u = res["used"]
    val, P = sm.terms_float64(res["db"][u], res["mu2"][u], res["M"][u], res["W9"][u], c["args"][4])
    err = np.abs(res["terms"][u].astype(np.float64) - val)
    cc = np.asarray([sm.C_HTWH] * 21 + [sm.C_HTWDZ] * 6, np.float64)
    lim = cc * sm.U32 * P * (1.0 + 2.0 ** -40)                              # (+ the float64 evaluation's own roundings)
    ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))
    print("%s: float32 terms against float64, worst |difference| / bound = %.3f over %d voxels" % (name, float(ratio.max()), int(u.sum())))
    assert u.sum() > 100 and (err <= lim).all()


@pytest.mark.parametrize("name", CASES)
def test_the_reduction_bound_holds_for_both_trees_and_any_slot_order(name):
    """emulate_total over both forms and random slot orders stays inside bound on every case the GPU tests use."""
    c = _cpu_case(name); T = c["res"]["terms"]; ns = T.shape[0]
    rng = np.random.default_rng(31)
    for form in ("256", "512"):
        worst = 0.0
        for trial in range(6):
            order = np.arange(ns) if trial == 0 else rng.permutation(ns)
            w, bad = sm.compare_total(sm.emulate_total(T[order], form), T, ns, form)
            assert not bad, (name, form, trial, bad)
            worst = max(worst, w)
        print("%s: %s-slot tree, D = %d, emulated total reaches %.3f of the bound over 6 slot orders" % (name, form, sm.depth(ns, form), worst))
        assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("name", CASES)
def test_the_comparison_catches_a_dropped_a_doubled_a_swapped_and_a_transposed_voxel(name):
    """The checker itself, on records built from the model.  A voxel whose term exceeds 4 x bound in some entry cannot be dropped or added twice unnoticed: the
    faulty total is at least |term| - 2 bound' away from the exact one (bound' <= 5 / 4 bound of the total with or without the voxel).  That set is at least 90 % of
    the contributing voxels on every case; every voxel in it is tried."""
    c = _cpu_case(name); res = c["res"]; T = res["terms"]; ns = T.shape[0]; form = c["form"]
    ex = sm.exact_total(T); S, A = ex
    assert not sm.compare_total(sm.emulate_total(T, form), T, ns, form, ex)[1]
    B = np.asarray([float(x) for x in sm.bound(A, ns, form)])
    used = np.nonzero(res["used"])[0]
    big = [i for i in used.tolist() if (np.abs(T[i].astype(np.float64)) > 4.0 * B).any()]
    share = len(big) / used.size
    print("%s: %d of %d contributing voxels (%.1f %%) exceed 4 x bound in some entry" % (name, len(big), used.size, 100.0 * share))
    assert share >= 0.9
    tot = sm.emulate_total(T, form)
    for i in big:                                                         # (the faulty total from the sound one: +- one float32 term, one more rounding)
        assert sm.compare_total((tot - T[i]).astype(np.float32), T, ns, form, ex)[1], ("dropped", i)
        assert sm.compare_total((tot + T[i]).astype(np.float32), T, ns, form, ex)[1], ("doubled", i)
    for i in big[:: max(1, len(big) // 8)]:                                 # the whole tree again, for a sample
        drop = T.copy(); drop[i] = 0
        assert sm.compare_total(sm.emulate_total(drop, form), T, ns, form, ex)[1], ("dropped", i)
        twice = np.concatenate([T, T[i:i + 1]])
        assert sm.compare_total(sm.emulate_total(twice, form), T, ns, form, ex)[1], ("doubled", i)
    words, n2, m, fit, J = c["args"]
    cand = [i for i in big if n2[i] != m[i] and min(n2[i], m[i]) > c["g"]["n"]]
    assert cand
    for kind, i in (("swap_counts", cand[0]), ("swap_counts", cand[-1]), ("transpose_hz", big[0]), ("transpose_hz", big[-1])):
        bad = sm.voxel_terms(words, n2, m, fit, J, flags=0, n=c["g"]["n"], iter=0, _fault=(kind, i))["terms"]
        assert not np.array_equal(bad[i].view(np.uint32), T[i].view(np.uint32)), (kind, i)              # the one-voxel comparison is bit for bit
        assert sm.compare_total(sm.emulate_total(bad, form), T, ns, form, ex)[1], (kind, i)                  # and the whole-scan comparison fails as well


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------------

def _bits_equal_or_zero(got, want):
    """Bit for bit where `want` is non-zero, == where it is zero."""
    got = np.ascontiguousarray(got, np.float32); want = np.ascontiguousarray(want, np.float32)
    return bool(np.all((got == want) & ((want == 0) | (got.view(np.uint32) == want.view(np.uint32)))))


def _same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


class _Device:
    """Per grid what the DEVICE built from scan 1, fetched once per module and never modified: the SlotFit records in slot order (a keyframe store's raw words),
    n_slots, and the aux tables of a one-iteration solve."""

    def __init__(self, ctx):
        self.ctx = ctx; self._info = {}

    def info(self, grid):
        if grid not in self._info:
            from icet_amd import api
            a = tpp._synthetic()[0]; g = GRIDS[grid]
            store = api.KeyframeStore(self.ctx, 1, g["bins_phi"], g["bins_theta"], g["n"], g["thresh"], g["buff"])
            t, d = tpp._scan_dev(a)
            store.put_device([0], [d]); self.ctx.sync()
            ns = store.debug_fetch(0, "n_slots"); fit = sm.fit_from_words(store.debug_fetch(0, "fit")); sov = store.debug_fetch(0, "slot_of_voxel").copy()
            store.close()
            ax = self.ctx.solve(a, a[:1024], 1, np.zeros(6), g["bins_phi"], g["bins_theta"], g["n"], g["thresh"], g["buff"], aux=True)["aux"]
            assert ns == fit.shape[0] and np.array_equal(sov[fit["v"]], np.arange(ns))
            self._info[grid] = dict(a=a, g=g, n_slots=int(ns), fit=fit, act=fit["v"].astype(np.int64), aux=ax, kf=pm.keyframe_tables(ax, g["n"]),
                                    form=sm.form_of(g["bins_phi"] * g["bins_theta"]))
        return self._info[grid]

    def park(self, ctx, grid):
        i = self.info(grid)
        t, d = tpp._scan_dev(i["a"])
        ctx.keyframe_device([d], tpp._params(i["g"]))
        ctx.sync()
        return i


@pytest.fixture(scope="module")
def device(gpu_ctx):
    return _Device(gpu_ctx)


def _terms(ctx, g, scans2, X, flags=0, runlen=1):
    """One hook call: every scan 2 against parked keyframe 0 at pose X (one pose, or one per scan)."""
    from icet_amd import api
    prm = tpp._params(g, runlen, flags)
    V = g["bins_phi"] * g["bins_theta"]
    s2 = [tpp._scan_dev(s) for s in scans2]
    k = len(s2)
    Xh = np.ascontiguousarray(np.broadcast_to(np.asarray(X, np.float32).reshape(-1, 6), (k, 6)))
    Xd = torch.from_numpy(Xh.copy()).to("cuda:0")
    sums = torch.full((k, V, 20), -1, dtype=torch.int32, device="cuda:0")
    xf, H, gv, out = (torch.full((k, w), float("nan"), dtype=torch.float32, device="cuda:0") for w in (48, 36, 6, 48))
    torch.cuda.synchronize()
    ctx.debug_gn_terms([0] * k, [d for _, d in s2], prm, Xd.data_ptr(), sums.data_ptr(), xf.data_ptr(), H.data_ptr(), gv.data_ptr(), out.data_ptr())
    ctx.sync()
    return dict(rec=np.frombuffer(sums.cpu().numpy().tobytes(), api.POINT_SUMS_DTYPE).reshape(k, V), xf=xf.cpu().numpy(), H=H.cpu().numpy().reshape(k, 6, 6),
                g=gv.cpu().numpy(), out=out.cpu().numpy(), X=Xh)


def _model(info, rec, xf, flags=0, it=0):
    """The model on one registration's dumped records (V,), in the device's slot order, with the device's own J."""
    act = info["act"]
    return sm.voxel_terms(rec["sums"][act], rec["n2"][act].astype(np.int64), rec["m"][act].astype(np.int64), info["fit"], xf[16:43], flags=flags, n=info["g"]["n"], iter=it)


def _hold_total(label, r, k, res, info):
    H = r["H"][k]
    assert np.array_equal(H.view(np.uint32), H.T.view(np.uint32)), label + ": the lower triangle is not the mirrored upper one"
    got = sm.pack(H, r["g"][k])
    worst, bad = sm.compare_total(got, res["terms"], info["n_slots"], info["form"])
    emu = sm.emulate_total(res["terms"], info["form"])
    print("%s: %d contributing voxels of %d slots, D = %d, worst |error| / bound = %.3f; the emulated tree in slot order gives %s"
          % (label, int(res["used"].sum()), info["n_slots"], sm.depth(info["n_slots"], info["form"]), worst, "the same bits" if _bits_equal_or_zero(got, emu) else "other bits"))
    assert not bad, (label, bad, got, emu)
    return worst


@pytest.mark.gpu
def test_fit_records_rebuilt_from_the_aux_tables_are_the_raw_slot_records(device):
    """s1n = sigma1 / float32(n1_raw - 1), M = diag(l_diag) evecs1 from a solve's aux outputs against the raw SlotFit words of a keyframe store, a whole keyframe."""
    for grid in ("coarse", "fine"):
        i = device.info(grid); ax = i["aux"]
        assert np.array_equal(np.sort(i["act"]), np.nonzero(i["kf"]["active"])[0])
        re = sm.fit_from_tables(ax["mu1"], ax["sigma1"], ax["evecs1"], ax["l_diag"], ax["n1_raw"], i["act"])
        assert i["n_slots"] > 100 and re.tobytes() == i["fit"].tobytes(), grid
    f = device.info("fine")
    assert f["g"]["bins_phi"] * f["g"]["bins_theta"] > 4096 and f["n_slots"] > 1024


def _rows_by_voxel(scan2, X, info):
    g = info["g"]
    vox, inb = pm.membership(pm.transform(scan2, X), info["kf"], g["bins_phi"], g["bins_theta"])
    return vox, inb


def _pick_voxels(info, res, rec):
    """At least 64 voxels (slot indices): every count of kept axes, the thinnest and the thickest Rp, the largest |mu2 - mu1|, and voxels that fail a count gate."""
    n = info["g"]["n"]
    kept = (info["fit"]["M"].reshape(-1, 3, 3) != 0).any(2).sum(1)
    used = res["used"]
    pick = []
    for k in (1, 2, 3):
        idx = np.nonzero(used & (kept == k))[0]
        assert idx.size > 0, "no contributing voxel with %d kept axes" % k
        pick += idx[:: max(1, idx.size // 18)][:18].tolist()
    tr = res["Rp"][:, [0, 3, 5]].astype(np.float64)
    small = np.where(tr > 0, tr, np.inf).min(1); large = tr.max(1)
    u = np.nonzero(used)[0]
    pick += [int(u[small[u].argmin()]), int(u[large[u].argmax()]), int(u[np.linalg.norm(res["db"][u].astype(np.float64), axis=1).argmax()])]
    n2 = rec["n2"][info["act"]].astype(np.int64); m = rec["m"][info["act"]].astype(np.int64)
    gated = np.nonzero((n2 > 0) & ~((n2 > n) & (m > n)))[0]
    assert gated.size > 0
    pick += gated[:8].tolist()
    pick = list(dict.fromkeys(pick))
    extra = [int(x) for x in u if int(x) not in set(pick)]
    pick += extra[: max(0, 64 - len(pick))]
    assert len(pick) >= 64
    return pick, set(gated[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["coarse@pose", "coarse@zero"])
def test_one_voxel_per_registration_gives_the_models_bits_and_whole_scans_keep_the_bound(gpu_ctx, device, name):
    """(a) 64+ registrations, each the rows of one voxel: H^T W H and H^T W dz are that voxel's 27 model terms added to +0, bit for bit, under the default weight and
    under FLAG_DOUBLE_W; a voxel that fails a count gate gives zeros.  (b) the whole scan in the same calls: within D 2^-24 sum |term| of the exact sum (256-thread form)."""
    a, b, X, g = _scans(name)
    info = device.park(gpu_ctx, "coarse")
    whole = _terms(gpu_ctx, g, [b], X)
    res = _model(info, whole["rec"][0], whole["xf"][0])
    assert int(res["used"].sum()) > 250
    _hold_total(name + " whole scan", whole, 0, res, info)
    pick, gated = _pick_voxels(info, res, whole["rec"][0])
    vox, _ = _rows_by_voxel(b, X, info)
    scans = [b[vox == int(info["act"][s])] for s in pick]
    for flags, label in ((0, "default W"), (sm.FLAG_DOUBLE_W, "FLAG_DOUBLE_W")):
        r = _terms(gpu_ctx, g, scans + [b], X, flags=flags)
        assert all(_same_bits(r["xf"][k][:43], whole["xf"][0][:43]) for k in range(len(scans) + 1))      # (write_xf leaves the five floats behind J[27] alone)
        n_used = 0
        for k, s in enumerate(pick):
            rec = r["rec"][k]
            one = _model(info, rec, r["xf"][k], flags=flags)
            assert int(one["used"].sum()) <= 1 and (not one["used"].any() or one["used"][s]), (label, k, s)
            want = (one["terms"][s] + np.float32(0)).astype(np.float32)
            Hw, gw = sm.mirror(want)
            assert _bits_equal_or_zero(r["H"][k], Hw) and _bits_equal_or_zero(r["g"][k], gw), (name, label, "slot %d voxel %d" % (s, info["act"][s]), r["H"][k], Hw, r["g"][k], gw)
            if s in gated:
                assert not one["used"].any() and not r["H"][k].any() and not r["g"][k].any()
            n_used += int(one["used"].any())
        assert n_used >= 50
        full = _model(info, r["rec"][-1], r["xf"][-1], flags=flags)
        _hold_total("%s whole scan, %s" % (name, label), r, len(scans), full, info)
        print("%s, %s: %d single-voxel registrations carry the model's bits (%d of them contribute)" % (name, label, len(pick), n_used))


@pytest.mark.gpu
def test_fine_grid_three_launch_forms_keep_the_bound_and_agree_bit_for_bit(gpu_ctx, device):
    """V = 7200: the canonical 512-slot tree as two stages (n_regs = 1), as one block of 512 (n_regs = 5) and as the stage-2 block doing the whole solve because
    stage 1 declined (force_exact: the overflow list is not empty when the production solve of ctx.solve starts).  Same sums, same bits; each within the bound."""
    import icet_amd
    a, b, X, g = _scans("fine@pose")
    info = device.park(gpu_ctx, "fine")
    one = _terms(gpu_ctx, g, [b], X)
    res = _model(info, one["rec"][0], one["xf"][0])
    vb = np.unique(np.nonzero(res["used"])[0] // 512)
    assert info["n_slots"] > 1024 and vb.size >= 2, (info["n_slots"], vb)
    _hold_total("fine grid, two stages", one, 0, res, info)
    five = _terms(gpu_ctx, g, [b] * 5, X)
    for k in range(5):
        assert five["rec"][k].tobytes() == one["rec"][0].tobytes()
        assert _same_bits(five["H"][k], one["H"][0]) and _same_bits(five["g"][k], one["g"][0]) and _same_bits(five["out"][k], one["out"][0]), k
    _hold_total("fine grid, one block of 512", five, 4, res, info)
    ctx = icet_amd.Context(0)
    try:
        ctx.set_option("force_exact", 1)
        device.park(ctx, "fine")
        fe1 = _terms(ctx, g, [b], X)
        fres = _model(info, fe1["rec"][0], fe1["xf"][0])
        _hold_total("fine grid, force_exact, two stages behind the hook's drain", fe1, 0, fres, info)
        fe5 = _terms(ctx, g, [b] * 5, X)
        assert fe5["rec"][4].tobytes() == fe1["rec"][0].tobytes() and _same_bits(fe5["H"][4], fe1["H"][0]) and _same_bits(fe5["g"][4], fe1["g"][0])
        ax = ctx.solve(a, b, 1, X, g["bins_phi"], g["bins_theta"], g["n"], g["thresh"], g["buff"], aux=True)["aux"]      # stage 1 declines: the list is full
        act = info["kf"]["active"]
        assert np.array_equal(ax["n2_raw"][0][act], fe1["rec"][0]["n2"][act].astype(np.int32)) and np.array_equal(ax["n2_in"][0][act], fe1["rec"][0]["m"][act].astype(np.int32))
        assert _same_bits(ax["htwh"][0], fe1["H"][0]) and _same_bits(ax["htwdz"][0], fe1["g"][0])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_the_fused_solve_carries_the_hooks_bits_and_the_tail_closes_the_chain(device):
    """(c) option fuse_solve: ctx.solve(runlen = 1, x0 = X) runs the solve inside the point pass's launch, a guest block wider than kT: the hook's H^T W H and
    H^T W dz bit for bit.  With gn_cond_bound 0 (the literal tail) the hook's X, pred_stds and cov are the oracle's gn_tail of the hook's own sums, bit for bit."""
    import icet_amd
    from oracle import pyoracle as po
    a, b, X, g = _scans("coarse@pose")
    ctx = icet_amd.Context(0)
    try:
        ctx.set_option("fuse_solve", 1); ctx.set_option("gn_cond_bound", 0)
        device.park(ctx, "coarse")
        r = _terms(ctx, g, [b], X)
        tail = po.gn_tail(r["H"][0], r["g"][0])
        out = r["out"][0]
        assert _same_bits(out[:6], (X + tail["dx"]).astype(np.float32)), (out[:6], X + tail["dx"])
        assert _same_bits(out[6:12], tail["pred_stds"]) and _same_bits(out[12:48], tail["cov"].reshape(36))
        s = ctx.solve(a, b, 1, X, g["bins_phi"], g["bins_theta"], g["n"], g["thresh"], g["buff"], aux=True)
        assert _same_bits(s["aux"]["htwh"][0], r["H"][0]) and _same_bits(s["aux"]["htwdz"][0], r["g"][0])
        assert _same_bits(s["X"], out[:6]) and _same_bits(s["pred_stds"], out[6:12]) and _same_bits(s["cov"].reshape(36), out[12:48])
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["coarse@pose", "coarse@zero", "fine@pose"])
def test_the_score_counts_exactly_and_sums_the_models_chi2(gpu_ctx, device, name):
    """(d) score_indexed_device at the hook's poses: voxels and points_in are the model's, chi2 within one float32 ulp of the float32 of the exact sum of the model's
    float64 terms dz^T W dz, chi2_per_voxel consistent with both; default weight and FLAG_DOUBLE_W."""
    import math
    from icet_amd import api
    a, b, X, g = _scans(name)
    info = device.park(gpu_ctx, name.split("@")[0])
    for flags in (0, sm.FLAG_DOUBLE_W):
        r = _terms(gpu_ctx, g, [b], X, flags=flags)
        res = _model(info, r["rec"][0], r["xf"][0], flags=flags)
        t, d = tpp._scan_dev(b)
        Xd = torch.from_numpy(r["X"].copy()).to("cuda:0"); sc = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        gpu_ctx.score_indexed_device([0], [d], tpp._params(g, 1, flags), Xd.data_ptr(), sc.data_ptr())
        gpu_ctx.sync()
        s = np.frombuffer(sc.cpu().numpy().tobytes(), api.SCORE_DTYPE)[0]
        used = res["used"]; m = r["rec"][0]["m"][info["act"]].astype(np.int64)
        assert int(s["voxels"]) == int(used.sum()) > 100 and int(s["points_in"]) == int(m[used].sum()) and int(s["points"]) == b.shape[0]
        exact = math.fsum(res["q"][used].tolist())
        want = np.float32(exact); ulp = float(np.spacing(want))
        dist = abs(float(s["chi2"]) - float(want)) / ulp
        wpv = np.float32(exact / int(used.sum()))
        dpv = abs(float(s["chi2_per_voxel"]) - float(wpv)) / float(np.spacing(wpv))
        print("%s flags %d: chi2 %.9g, %.2f ulp from the exact sum of the model's terms; chi2 per voxel %.2f ulp" % (name, flags, float(s["chi2"]), dist, dpv))
        assert dist <= 1.0 and dpv <= 1.0


def _poses_for_the_record():
    rng = np.random.default_rng(41)
    P = [np.zeros(6)]
    for e in (1e-7, 1e-5, 1e-3):
        P += [np.r_[rng.normal(size=3), rng.choice([-1, 1], 3) * e * rng.uniform(0.5, 1.5, 3)] for _ in range(8)]
    for c in (np.pi / 2, -np.pi / 2, np.pi, -np.pi):
        P += [np.r_[rng.normal(size=3), c + rng.normal(0, 1e-3, 3)] for _ in range(8)] + [np.r_[0, 0, 0, c, c, c]]
    P += [np.r_[rng.uniform(-0.6, 0.6), rng.uniform(-0.05, 0.05), rng.uniform(-0.02, 0.02), rng.uniform(-0.005, 0.005, 2), rng.uniform(-0.02, 0.02)] for _ in range(60)]      # the bench's range
    P += [np.r_[rng.normal(size=3), a_, 0.0, c_] for a_, c_ in rng.uniform(-np.pi, np.pi, (40, 2))]     # theta = 0: R shows sin / cos of phi and psi themselves
    P += [np.r_[rng.normal(size=3), rng.uniform(-np.pi, np.pi, 3)] for _ in range(40)]
    return np.asarray(P, np.float32)


@pytest.mark.gpu
def test_the_transform_record(gpu_ctx, device):
    """(e) ~200 poses: t and the angles are copied; every R / J entry lies within 3 x 2^-24 sum |products| of the float64 value of write_xf's formula on the
    float32-rounded sines and cosines (two products and a sum, fused or not); where an entry IS a sine or cosine (R[2][0] = sin theta, J[15] = cos theta, and at
    theta = 0 the first column and the last row of R) it is the correctly rounded float32 of the double value; the entries the source sets to zero are zero."""
    info = device.park(gpu_ctx, "coarse")
    P = _poses_for_the_record()
    assert 180 <= P.shape[0] <= 260
    b = tpp._synthetic()[1][:8]
    r = _terms(gpu_ctx, info["g"], [b] * P.shape[0], P)
    worst = 0.0
    for k, X in enumerate(P):
        xf = r["xf"][k]
        sc, val, ab = sm.xf_reference(X)
        sph, cph, sth, cth, sps, cps = sc
        assert _same_bits(xf[0:3], X[0:3]) and _same_bits(xf[12:15], X[3:6])
        assert all(xf[z] == 0 for z in sm.XF_ZERO), (k, X)
        assert _same_bits(xf[9], sth) and _same_bits(xf[31], cth), (k, X, xf[9], sth, xf[31], cth)
        if X[4] == 0:
            assert _same_bits(xf[3], cps) and _same_bits(xf[11], cph) and xf[6] == -sps and xf[10] == -sph, (k, X)
        lim = 3.0 * sm.U32 * ab
        err = np.abs(xf.astype(np.float64) - val)
        idx = [i for i in range(48) if ab[i] > 0]
        assert (err[idx] <= lim[idx]).all(), (k, X, [(i, err[i], lim[i]) for i in idx if err[i] > lim[i]])
        worst = max(worst, float((err[idx] / lim[idx]).max()))
    print("transform record: worst |error| / (3 x 2^-24 sum |products|) = %.3f over %d poses" % (worst, P.shape[0]))


@pytest.mark.gpu
def test_the_moving_object_gate(gpu_ctx, device):
    """(f) FLAG_REJECT_MOVING, evaluated as iteration 4 (runlen = 5): one voxel's rows shifted by 0.4 m along a KEPT axis (|dz| beyond the 0.3 m cutoff) contribute
    nothing although both count gates pass; the same shift along the voxel's PRUNED axis leaves dz alone and contributes the model's bits.  Without the flag, and
    with the flag at iteration 0, the kept-axis shift contributes the model's bits as well."""
    a, b, X, g = _scans("coarse@zero")
    info = device.park(gpu_ctx, "coarse")
    n = g["n"]
    M = info["fit"]["M"].reshape(-1, 3, 3); E = info["aux"]["evecs1"].reshape(-1, 3, 3)[info["act"]]
    keptrow = (M != 0).any(2)
    vox, inb = _rows_by_voxel(b, X, info)
    found = None
    for s in np.nonzero(keptrow.sum(1) == 2)[0]:
        v = int(info["act"][s]); rows = b[(vox == v) & inb]
        if rows.shape[0] < 3 * n:
            continue
        kr = int(np.nonzero(keptrow[s])[0][0]); pr = int(np.nonzero(~keptrow[s])[0][0])
        for sign in (1.0, -1.0):
            mk = (rows + np.float32(sign * 0.4) * E[s][kr]).astype(np.float32); mp = (rows + np.float32(sign * 0.4) * E[s][pr]).astype(np.float32)
            ck = pm.membership(pm.transform(mk), info["kf"], g["bins_phi"], g["bins_theta"]); cp = pm.membership(pm.transform(mp), info["kf"], g["bins_phi"], g["bins_theta"])
            alone = all(np.bincount(c_[0][c_[0] != v], minlength=1).max() <= n for c_ in (ck, cp))      # no neighbouring bin collects enough rows to pass its own gates
            if alone and int(((ck[0] == v) & ck[1]).sum()) > 2 * n and int(((cp[0] == v) & cp[1]).sum()) > 2 * n:
                found = (int(s), v, mk, mp, rows); break
        if found:
            break
    assert found, "no voxel with one pruned axis keeps its points under both shifts"
    s, v, mk, mp, rows = found
    F = sm.FLAG_REJECT_MOVING
    gate = _terms(gpu_ctx, g, [mk, mp, rows], X, flags=F, runlen=5)
    early = _terms(gpu_ctx, g, [mk], X, flags=F, runlen=1)
    off = _terms(gpu_ctx, g, [mk], X, flags=0, runlen=5)

    def one(r, k, flags, it):
        res = _model(info, r["rec"][k], r["xf"][k], flags=flags, it=it)
        want = (res["terms"][s] + np.float32(0)).astype(np.float32)
        Hw, gw = sm.mirror(want)
        assert int(res["used"].sum()) <= 1 and _bits_equal_or_zero(r["H"][k], Hw) and _bits_equal_or_zero(r["g"][k], gw), (k, flags, it, r["H"][k], Hw)
        return res
    rk = one(gate, 0, F, 4)
    rec = gate["rec"][0][v]
    assert int(rec["n2"]) > n and int(rec["m"]) > n and float(np.abs(rk["dz"][s]).max()) > 0.3 and not rk["used"].any()
    assert not gate["H"][0].any() and not gate["g"][0].any()
    rp = one(gate, 1, F, 4)
    assert rp["used"][s] and float(np.abs(rp["dz"][s]).max()) <= 0.3 and gate["H"][1].any()
    assert one(gate, 2, F, 4)["used"][s]
    assert one(early, 0, F, 0)["used"][s] and early["H"][0].any()
    assert one(off, 0, 0, 4)["used"][s] and _same_bits(off["H"][0], early["H"][0])
    print("moving-object gate: voxel %d, |dz| = %s under the kept-axis shift, %s under the pruned-axis shift" % (v, np.abs(rk["dz"][s]).tolist(), np.abs(rp["dz"][s]).tolist()))
