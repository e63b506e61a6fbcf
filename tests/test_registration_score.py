"""The registration score (include/icet_hip.h: icet_score, icet_score_indexed_device, icet_register_indexed_scored_device, icet_solve_indexed_scored,
icet_score_indexed) and the device-side best-of-group selection (icet_select_best_device).  The score is chi2 = sum_v dz^T W dz over the voxels the
next Gauss-Newton iteration at X would use; it is checked against the CPU restatement's per-voxel trace, and scoring must leave results, the workspace
and the parked keyframe exactly as the unscored calls do."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("icet_score_indexed_device", "icet_register_indexed_scored_device", "icet_solve_indexed_scored", "icet_score_indexed", "icet_select_best_device")


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_score_entry_points_are_exported():
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("compiler,ext", [("gcc", "c"), ("g++", "cpp")])
def test_icet_score_is_32_bytes_in_c_and_cpp(tmp_path, compiler, ext):
    src = tmp_path / ("probe." + ext)
    assert_kw = "_Static_assert" if ext == "c" else "static_assert"
    src.write_text('#include "icet_hip.h"\n#include <stddef.h>\n'
                   '%s(sizeof(icet_score) == 32, "size");\n'
                   '%s(offsetof(icet_score, chi2_per_voxel) == 4 && offsetof(icet_score, voxels) == 8 && offsetof(icet_score, points_in) == 12, "layout");\n'
                   '%s(offsetof(icet_score, points) == 16 && offsetof(icet_score, overlap) == 20 && offsetof(icet_score, reserved) == 24, "layout");\n'
                   'int main(void) { return 0; }\n' % (assert_kw, assert_kw, assert_kw))
    subprocess.check_call([compiler, "-std=c11" if ext == "c" else "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "probe.o")])
    from icet_amd import api
    assert api.SCORE_DTYPE.itemsize == 32
    assert [api.SCORE_DTYPE.fields[k][1] for k in ("chi2", "chi2_per_voxel", "voxels", "points_in", "points", "overlap", "reserved")] == [0, 4, 8, 12, 16, 20, 24]


def test_score_entry_points_refuse_a_null_context_and_bad_arguments():
    import icet_amd
    from icet_amd import api
    lib = api.load_library()
    p = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    idx = (C.c_int32 * 1)(0)
    assert lib.icet_score_indexed_device(None, C.byref(p), 1, idx, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_register_indexed_scored_device(None, C.byref(p), 1, idx, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_solve_indexed_scored(None, C.byref(p), 1, None, None, 1, idx, None, None, None, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_score_indexed(None, C.byref(p), 1, None, None, 1, idx, None, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_select_best_device(None, 1, idx, 1, None, None, None, None) == api.ICET_ERR_BAD_ARG
    ctx = icet_amd.Context.borrow(None)                              # a null handle: every call reaches the library and is refused there
    scan = np.zeros((100, 3), np.float32)
    calls = [lambda: ctx.score_indexed_device([0], [(0, 0, 0)], p, 0, 0),
             lambda: ctx.register_indexed_scored_device([0], [(0, 0, 0)], p, 0, 0),
             lambda: ctx.select_best_device([0], 1, 0, 0),
             lambda: ctx.solve_indexed_scored([scan], [scan], [0], 7),
             lambda: ctx.score_indexed([scan], [scan], [0], np.zeros((1, 6), np.float32)),
             lambda: ctx.solve_multistart(scan, scan, np.zeros((2, 6), np.float32), 7),
             # mismatched lengths: refused before the library is called
             lambda: ctx.score_indexed_device([0, 0], [(0, 0, 0)], p, 0, 0),
             lambda: ctx.register_indexed_scored_device([0], [(0, 0, 0)] * 2, p, 0, 0),
             lambda: ctx.solve_indexed_scored([scan], [scan, scan], [0], 7),
             lambda: ctx.score_indexed([scan], [scan, scan], [0, 0], np.zeros((1, 6), np.float32)),
             lambda: ctx.score_indexed([scan], [scan], [0, 0], np.zeros((1, 6), np.float32))]
    for f in calls:
        with pytest.raises(icet_amd.IcetError):
            f()


def test_host_selection_rule():
    """The NumPy statement of the rule that the device selection is tested against."""
    from icet_amd import api
    sc = dict(voxels=np.array([10, 4, 6, 0, 0, 8, 8]), chi2_per_voxel=np.array([5.0, 1.0, 7.0, np.inf, np.inf, 3.0, 3.0], np.float32))
    # group 0: r0 (10 vox), r1 (4 < 5: not eligible), r2 -> r0 wins on chi2; group 1: nothing; group 2: zero voxels only; group 3: tie -> lower index
    best = api.select_best(sc, [0, 0, 0, 2, 2, 3, 3], 4)
    assert best.tolist() == [0, -1, -1, 5]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).to(dev)


def _desc(t, n=None):
    return (t.data_ptr(), t.shape[1] if n is None else int(n), t.shape[1])


def _np(t):
    """(3, N) tensor -> N x 3 numpy."""
    return np.ascontiguousarray(t.detach().cpu().numpy().T)


def _score_rows(t):
    """A (k, 8) int32 device tensor holding icet_score records -> SCORE_DTYPE numpy array."""
    from icet_amd import api
    return np.frombuffer(t.detach().cpu().numpy().tobytes(), dtype=api.SCORE_DTYPE)


def _oracle_score(a, b, X, double_w=False):
    """The score at X from the CPU restatement's per-voxel trace of iteration 0 (runlen 1 from x0 = X, the device's arithmetic), with W = the restated
    float COD of the float matrix M R_noise M^T; double_w: W = the 50-digit pseudo-inverse of its upper triangle under the 3 eps rank rule (ICET_FLAG_DOUBLE_W)."""
    from oracle import pyoracle as po
    from oracle import mpref
    ref = po.solve(a, b, x0=np.asarray(X, np.float32), runlen=1, trace=True, mode=po.DEVICE_ARITH)
    tr = ref["trace"]
    used = np.nonzero(tr["used"][0])[0]
    chi2 = 0.0
    for v in used:
        M = (tr["Ldiag"][v][:, None] * tr["evecs1"][v]).astype(np.float32)                  # L U^T
        d1 = np.float32(tr["n1_raw"][v] - 1); d2 = np.float32(tr["n2_raw"][0][v] - 1)
        Rn = (tr["sigma1"][v] / d1 + tr["sigma2"][0][v] / d2).astype(np.float32)
        Rp = (M @ Rn @ M.T).astype(np.float32)
        if double_w:
            W = mpref.unpack3(mpref.pinv3_sym(mpref.pack_upper(Rp))[0])
        else:
            W, _ = po.pinv(Rp)
        dz = M.astype(np.float64) @ (tr["mu2"][0][v].astype(np.float64) - tr["mu1"][v].astype(np.float64))
        chi2 += float(dz @ W.astype(np.float64) @ dz)
    return dict(chi2=chi2, voxels=int(used.size), points_in=int(tr["n2_in"][0][used].sum()), points=int(b.shape[0]))


def _cases(frames, sample_pc):
    from icet_amd import lidar_sim as ls
    a, b = sample_pc
    yield "sample", a, b, [[0.644, 0.004, 0.017, 0.001, 0.0, 0.001], [0, 0, 0, 0, 0, 0], [0.2, 0, 0, 0, 0, 0]]
    a, b = frames
    yield "frame_804_805", a, b, [[0, 0, 0, 0, 0, 0], [0.05, 0.01, 0, 0, 0, 0.002], [0.6, -0.2, 0, 0, 0, 0.04]]
    for seed in (0, 1):
        s1, s2, xt = ls.make_pair(scene_seed=3000 + seed, noise_seed=3100 + seed, rings=32, steps=1024)
        bad = xt.copy(); bad[0] += 0.4; bad[5] += 0.05
        yield "synthetic%d" % seed, _np(s1), _np(s2), [xt, np.zeros(6, np.float32), bad]


@pytest.mark.gpu
def test_score_matches_the_cpu_restatement(gpu_ctx, frames, sample_pc):
    import icet_amd
    ctx = icet_amd.Context(0)
    for name, a, b, poses in _cases(frames, sample_pc):
        X = np.asarray(poses, np.float32)
        got = ctx.score_indexed([a], [b] * 3, [0, 0, 0], X)
        for k in range(3):
            ref = _oracle_score(a, b, X[k])
            assert got["voxels"][k] == ref["voxels"], (name, k, got["voxels"][k], ref["voxels"])
            assert got["points_in"][k] == ref["points_in"], (name, k, got["points_in"][k], ref["points_in"])
            assert got["points"][k] == ref["points"]
            rtol = 1e-4
            assert abs(float(got["chi2"][k]) - ref["chi2"]) <= rtol * abs(ref["chi2"]), (name, k, float(got["chi2"][k]), ref["chi2"])
            assert np.isclose(got["chi2_per_voxel"][k], got["chi2"][k] / got["voxels"][k], rtol=1e-6)
            assert np.isclose(got["overlap"][k], got["points_in"][k] / got["points"][k], rtol=1e-6)
    ctx.close()


@pytest.mark.gpu
def test_double_w_score_matches_a_50_digit_restatement(gpu_ctx, frames, sample_pc):
    """Under ICET_FLAG_DOUBLE_W (k_gn_score<false>): chi2, voxels and points_in against the trace with W = the 50-digit pseudo-inverse (3 eps rank rule)."""
    import icet_amd
    from icet_amd import api
    ctx = icet_amd.Context(0)
    for name, a, b, poses in _cases(frames, sample_pc):
        X = np.asarray(poses, np.float32)
        got = ctx.score_indexed([a], [b] * 3, [0, 0, 0], X, flags=api.FLAG_DOUBLE_W)
        for k in range(3):
            ref = _oracle_score(a, b, X[k], double_w=True)
            assert got["voxels"][k] == ref["voxels"], (name, k, got["voxels"][k], ref["voxels"])
            assert got["points_in"][k] == ref["points_in"], (name, k, got["points_in"][k], ref["points_in"])
            assert got["points"][k] == ref["points"]
            rtol = 1e-4
            assert abs(float(got["chi2"][k]) - ref["chi2"]) <= rtol * abs(ref["chi2"]), (name, k, float(got["chi2"][k]), ref["chi2"])
    ctx.close()


@pytest.mark.gpu
def test_sample_pair_score_at_the_converged_pose(gpu_ctx, sample_pc):
    import icet_amd
    a, b = sample_pc
    ctx = icet_amd.Context(0)
    got = ctx.score_indexed([a], [b], [0], np.array([[0.644, 0.004, 0.017, 0.001, 0.0, 0.001]], np.float32))
    ctx.close()
    assert got["voxels"][0] == 96 and got["points_in"][0] == 9359 and got["points"][0] == b.shape[0]
    assert 0.0 < got["chi2_per_voxel"][0] < 100.0


def _keyframes(dev, frames, sample_pc):
    from icet_amd import lidar_sim as ls
    p0, p1 = ls.make_batch_pair(0, device=dev), ls.make_batch_pair(1, device=dev)
    kf = [p0[0], p1[0], _dev(frames[0], dev), _dev(sample_pc[0], dev)]
    partner = [p0[1], p1[1], _dev(frames[1], dev), _dev(sample_pc[1], dev)]
    return kf, partner


def _registrations(partner, kf_index, seed):
    rng = np.random.default_rng(seed)
    d2 = []
    for r, k in enumerate(kf_index):
        t = partner[k]
        d2.append(_desc(t, t.shape[1] * 2 // 3 if r % 3 == 2 else None))
    x0 = np.zeros((len(kf_index), 6), np.float32)
    x0[:, 0] = rng.uniform(-0.05, 0.05, len(kf_index)); x0[:, 1] = rng.uniform(-0.03, 0.03, len(kf_index)); x0[:, 5] = rng.uniform(-0.005, 0.005, len(kf_index))
    return d2, x0


def _mapping(n_regs, n_kf, seed):
    rng = np.random.default_rng(seed)
    m = np.concatenate([np.arange(n_kf)[::-1], rng.integers(0, n_kf, max(0, n_regs - n_kf))])[:n_regs]
    return [int(v) for v in m]


def _run(ctx, kind, kf_index, d2, prm, dev, x=None):
    """kind: 'plain' (register_indexed_device), 'scored', 'score' (score_indexed_device at the poses x).  Returns (out, score rows)."""
    k = len(kf_index)
    out = torch.full((k, 48), float("nan"), dtype=torch.float32, device=dev)
    sc = torch.full((k, 8), -7, dtype=torch.int32, device=dev)
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev) if not torch.is_tensor(x) else x.contiguous()
    torch.cuda.synchronize()
    if kind == "plain":
        ctx.register_indexed_device(kf_index, d2, prm, out.data_ptr(), xd.data_ptr())
    elif kind == "scored":
        ctx.register_indexed_scored_device(kf_index, d2, prm, out.data_ptr(), sc.data_ptr(), xd.data_ptr())
    else:
        ctx.score_indexed_device(kf_index, d2, prm, xd.data_ptr(), sc.data_ptr())
    ctx.sync()
    return out, sc


@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["NONE", "DOUBLE_W", "REJECT_MOVING", "ROUNDTRIP_SCAN2"])
@pytest.mark.parametrize("n_regs", [5, 300])
def test_scoring_leaves_results_alone(gpu_ctx, frames, sample_pc, flag, n_regs):
    """d_out of the scored call carries the bits of the unscored call; its score carries the bits of score_indexed_device at the returned X.
    (5 registrations: eager, captured and replayed calls.)"""
    import icet_amd
    from icet_amd import api
    dev = torch.device("cuda", 0)
    kf, partner = _keyframes(dev, frames, sample_pc)
    f = 0 if flag == "NONE" else getattr(api, "FLAG_" + flag)
    prm = api.Params(9, 24, 75, 25, 0.1, 0.1, f)                     # 9 iterations: the moving-voxel gate (from iteration 4) is live at the score
    kf_index = _mapping(n_regs, 4, 41)
    d2, x0 = _registrations(partner, kf_index, 42)
    ctx = icet_amd.Context(0)
    ctx.keyframe_device([_desc(t) for t in kf], prm)
    ref, _ = _run(ctx, "plain", kf_index, d2, prm, dev, x0)
    assert bool(torch.isfinite(ref).all())
    first = None
    for _ in range(3):
        out, sc = _run(ctx, "scored", kf_index, d2, prm, dev, x0)
        assert torch.equal(out, ref)
        if first is None:
            first = sc.clone()
        assert torch.equal(sc, first)
        _, sc2 = _run(ctx, "score", kf_index, d2, prm, dev, out[:, :6])
        assert torch.equal(sc, sc2)
    s = _score_rows(first)
    assert (s["voxels"] > 0).all() and np.isfinite(s["chi2"]).all() and (s["reserved"] == 0).all()
    assert torch.equal(_run(ctx, "plain", kf_index, d2, prm, dev, x0)[0], ref)   # the workspace is as a solve leaves it
    ctx.close()


@pytest.mark.gpu
def test_scored_runlen_zero_scores_x0(gpu_ctx, frames, sample_pc):
    import icet_amd
    from icet_amd import api
    dev = torch.device("cuda", 0)
    kf, partner = _keyframes(dev, frames, sample_pc)
    prm0 = api.Params(0, 24, 75, 25, 0.1, 0.1, 0)
    kf_index = [3, 2, 2]
    d2, x0 = _registrations(partner, kf_index, 51)
    ctx = icet_amd.Context(0)
    ctx.keyframe_device([_desc(t) for t in kf], prm0)
    out, sc = _run(ctx, "scored", kf_index, d2, prm0, dev, x0)
    assert torch.equal(out[:, :6].cpu(), torch.from_numpy(x0)) and not bool(out[:, 6:].any())
    _, sc2 = _run(ctx, "score", kf_index, d2, prm0, dev, x0)
    assert torch.equal(sc, sc2)
    ctx.close()


@pytest.mark.gpu
def test_a_registrations_score_does_not_depend_on_the_call(gpu_ctx, frames, sample_pc):
    import icet_amd
    from icet_amd import api
    dev = torch.device("cuda", 0)
    kf, partner = _keyframes(dev, frames, sample_pc)
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    kf_index = _mapping(300, 4, 61)
    d2, x0 = _registrations(partner, kf_index, 62)
    ctx = icet_amd.Context(0)
    ctx.keyframe_device([_desc(t) for t in kf], prm)
    out, sc = _run(ctx, "scored", kf_index, d2, prm, dev, x0)
    _, sc_pose = _run(ctx, "score", kf_index, d2, prm, dev, out[:, :6])
    for r in (0, 1, 2, 3, 150, 299):
        _, one = _run(ctx, "scored", [kf_index[r]], [d2[r]], prm, dev, x0[r:r + 1])
        assert torch.equal(one[0], sc[r]), r
        _, one = _run(ctx, "score", [kf_index[r]], [d2[r]], prm, dev, out[r:r + 1, :6])
        assert torch.equal(one[0], sc_pose[r]), r
    ctx.close()


@pytest.mark.gpu
def test_workspace_and_keyframe_survive_score_calls_and_refusals(gpu_ctx, frames, sample_pc):
    import icet_amd
    from icet_amd import api
    dev = torch.device("cuda", 0)
    kf, partner = _keyframes(dev, frames, sample_pc)
    kf, partner = kf[:3], partner[:3]
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    kf_index = [2, 0, 1, 1]
    d2, x0 = _registrations(partner, kf_index, 71)
    ctx = icet_amd.Context(0)
    ctx.keyframe_device([_desc(t) for t in kf], prm)
    before, _ = _run(ctx, "plain", kf_index, d2, prm, dev, x0)
    _run(ctx, "scored", kf_index, d2, prm, dev, x0)
    bad_pose = x0.copy(); bad_pose[:, 0] += 3.0
    _run(ctx, "score", kf_index, d2, prm, dev, bad_pose)
    assert torch.equal(_run(ctx, "plain", kf_index, d2, prm, dev, x0)[0], before)
    sc = torch.zeros((2, 8), dtype=torch.int32, device=dev); out = torch.zeros((2, 48), dtype=torch.float32, device=dev)
    xd = torch.zeros((2, 6), dtype=torch.float32, device=dev)
    refusals = [(lambda: ctx.score_indexed_device([0, 3], d2[:2], prm, xd.data_ptr(), sc.data_ptr()), api.ICET_ERR_BAD_ARG),
                (lambda: ctx.register_indexed_scored_device([-1, 0], d2[:2], prm, out.data_ptr(), sc.data_ptr()), api.ICET_ERR_BAD_ARG),
                (lambda: ctx.score_indexed_device([0, 1], d2[:2], api.Params(7, 48, 150, 25, 0.1, 0.1, 0), xd.data_ptr(), sc.data_ptr()), api.ICET_ERR_BAD_ARG),
                (lambda: ctx.register_indexed_scored_device([0, 1], d2[:2], api.Params(7, 24, 75, 25, 0.1, 0.1, api.FLAG_TRUE_SORT), out.data_ptr(), sc.data_ptr()), api.ICET_ERR_BAD_ARG),
                (lambda: ctx.register_indexed_scored_device([0, 1], d2[:2], prm, out.data_ptr(), 0), api.ICET_ERR_BAD_ARG),
                (lambda: ctx.score_indexed_device([0, 1], d2[:2], prm, 0, sc.data_ptr()), api.ICET_ERR_BAD_ARG)]
    for call, status in refusals:
        with pytest.raises(icet_amd.IcetError) as e:
            call()
        assert e.value.status == status
    ctx.set_option("keep", 1)
    for call in (lambda: ctx.score_indexed_device([0, 1], d2[:2], prm, xd.data_ptr(), sc.data_ptr()),
                 lambda: ctx.register_indexed_scored_device([0, 1], d2[:2], prm, out.data_ptr(), sc.data_ptr())):
        with pytest.raises(icet_amd.IcetError) as e:
            call()
        assert e.value.status == api.ICET_ERR_UNSUPPORTED
    ctx.set_option("keep", 0)
    assert torch.equal(_run(ctx, "plain", kf_index, d2, prm, dev, x0)[0], before)      # still parked, workspace clean
    ctx.close()


@pytest.mark.gpu
def test_multistart_selects_the_answer(gpu_ctx, sample_pc):
    import icet_amd
    a, b = sample_pc
    starts = np.zeros((6, 6), np.float32); starts[:, 0] = [0.0, 0.2, 0.4, 0.6, 0.8, 1.0]
    ctx = icet_amd.Context(0)
    res = ctx.solve_multistart(a, b, starts, 12)
    ctx.close()
    best = res["best"]
    cpv = res["score"]["chi2_per_voxel"]
    assert best >= 2 and abs(res["X"][0] - 0.645) < 0.01, (best, res["X"], cpv)
    assert np.array_equal(res["X"], res["X_all"][best])
    # the CPU restatement's trace gives 78.8 and 72.9 per voxel for the stuck starts (final X[0] -0.002 and 0.063) against 55.3 at 0.644
    assert cpv[0] >= 1.3 * cpv[best] and cpv[1] >= 1.3 * cpv[best], cpv
    single = gpu_ctx.solve(a, b, 12, starts[best], 24, 75)                     # the chosen result is the solve from that start
    assert np.array_equal(res["X"], single["X"]) and np.array_equal(res["cov"], single["cov"])


@pytest.mark.gpu
def test_select_best_device_follows_the_rule(gpu_ctx):
    import icet_amd
    from icet_amd import api
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(81)
    n = 200
    sc = np.zeros(n, api.SCORE_DTYPE)
    sc["voxels"] = rng.integers(0, 120, n)
    sc["chi2_per_voxel"] = rng.choice(np.array([10.0, 20.0, 30.0, 55.5], np.float32), n)      # few values: many ties
    sc["chi2_per_voxel"][sc["voxels"] == 0] = np.inf
    sc["chi2_per_voxel"][7] = np.nan
    group = rng.integers(0, 12, n).astype(np.int32)                                          # groups in any order, 12 .. 14 empty
    group[group == 5] = 6                                                                    # group 5 empty too
    sc["voxels"][group == 9] = 0                                                             # every registration of group 9 at 0 voxels
    sc["chi2_per_voxel"][group == 9] = np.inf
    n_groups = 15
    out = torch.arange(n * 48, dtype=torch.float32, device=dev).reshape(n, 48)
    dsc = torch.from_numpy(np.frombuffer(sc.tobytes(), np.int32).reshape(n, 8).copy()).to(dev)
    best = torch.full((n_groups,), 99, dtype=torch.int32, device=dev)
    best_out = torch.full((n_groups, 48), float("nan"), dtype=torch.float32, device=dev)
    ctx = icet_amd.Context(0)
    torch.cuda.synchronize()
    ctx.select_best_device(group, n_groups, dsc.data_ptr(), best.data_ptr(), out.data_ptr(), best_out.data_ptr())
    ctx.sync()
    want = api.select_best(sc, group, n_groups)
    assert best.cpu().numpy().tolist() == want.tolist()
    assert want[9] == -1 and want[5] == -1 and want[13] == -1
    for g in range(n_groups):
        row = best_out[g].cpu()
        if want[g] < 0:
            assert not bool(row.any())
        else:
            assert torch.equal(row, out[want[g]].cpu())
    best2 = torch.full((n_groups,), 99, dtype=torch.int32, device=dev)                       # without the rows
    ctx.select_best_device(group, n_groups, dsc.data_ptr(), best2.data_ptr()); ctx.sync()
    assert torch.equal(best2, best)
    with pytest.raises(icet_amd.IcetError):
        ctx.select_best_device(group, 11, dsc.data_ptr(), best2.data_ptr())                  # group id out of range
    ctx.close()


@pytest.mark.gpu
def test_score_is_lowest_at_the_true_motion(gpu_ctx):
    import icet_amd
    from icet_amd import lidar_sim as ls
    ctx = icet_amd.Context(0)
    for seed in (0, 1):
        s1, s2, xt = ls.make_pair(scene_seed=4000 + seed, noise_seed=4100 + seed)
        X = np.stack([xt, xt + np.array([0.3, 0, 0, 0, 0, 0], np.float32), xt + np.array([0, 0, 0, 0, 0, 0.05], np.float32)])
        got = ctx.score_indexed([_np(s1)], [_np(s2)] * 3, [0, 0, 0], X)
        cpv = got["chi2_per_voxel"]
        assert cpv[0] < cpv[1] and cpv[0] < cpv[2], (seed, cpv, got["voxels"])
    ctx.close()
