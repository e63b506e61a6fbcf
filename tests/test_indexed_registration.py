"""Indexed registration (include/icet_hip.h: icet_register_indexed_device, icet_solve_indexed): many scan 2s against a few parked keyframes,
each keyframe built once.  Every result must carry the bits icet_solve_batch_device gives for the expanded pair (scan1[kf_index[r]], scan2[r],
x0[r]); the parked keyframe survives the call, growth of the registration side and refused calls."""
import ctypes as C

import numpy as np
import pytest
import torch


def test_indexed_entry_points_are_exported_and_refuse_a_null_context():
    from icet_amd import api
    lib = api.load_library()
    for name in ("icet_register_indexed_device", "icet_solve_indexed"):
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    p = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    idx = (C.c_int32 * 1)(0)
    assert lib.icet_register_indexed_device(None, C.byref(p), 1, idx, None, None, None) == api.ICET_ERR_BAD_ARG
    assert lib.icet_solve_indexed(None, C.byref(p), 1, None, None, 1, idx, None, None, None, None, None, None) == api.ICET_ERR_BAD_ARG


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def _dev(a, dev):
    """numpy N x 3 -> float32 (3, N) on the device (column-major N x 3, ld = N)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).to(dev)


def _desc(t, n=None):
    return (t.data_ptr(), t.shape[1] if n is None else int(n), t.shape[1])


def _keyframes(dev, frames, sample_pc):
    """Four keyframes of three sizes (two synthetic batch pairs, the real frame pair, the reference's sample pair) and each one's partner scan."""
    from icet_amd import lidar_sim as ls
    p0, p1 = ls.make_batch_pair(0, device=dev), ls.make_batch_pair(1, device=dev)
    kf = [p0[0], p1[0], _dev(frames[0], dev), _dev(sample_pc[0], dev)]
    partner = [p0[1], p1[1], _dev(frames[1], dev), _dev(sample_pc[1], dev)]
    return kf, partner


def _registrations(kf, partner, kf_index, seed):
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


def _expanded(kf, kf_index, d2, x0, prm, dev):
    """icet_solve_batch_device on the expanded pairs, in a context of its own."""
    import icet_amd
    ref = icet_amd.Context(0)
    out = torch.zeros((len(kf_index), 48), dtype=torch.float32, device=dev)
    xd = torch.from_numpy(x0).to(dev)
    torch.cuda.synchronize()
    ref.solve_batch_device([_desc(kf[k]) for k in kf_index], d2, prm, out.data_ptr(), xd.data_ptr())
    ref.sync(); ref.close()
    return out


def _indexed(ctx, kf_index, d2, x0, prm, dev):
    out = torch.full((len(kf_index), 48), float("nan"), dtype=torch.float32, device=dev)
    xd = torch.from_numpy(x0).to(dev)
    torch.cuda.synchronize()
    ctx.register_indexed_device(kf_index, d2, prm, out.data_ptr(), xd.data_ptr())
    ctx.sync()
    return out


def _mapping(n_regs, n_kf, seed):
    """Every keyframe used, repeats, out of order."""
    rng = np.random.default_rng(seed)
    m = np.concatenate([np.arange(n_kf)[::-1], rng.integers(0, n_kf, max(0, n_regs - n_kf))])[:n_regs]
    return [int(v) for v in m]


@pytest.mark.gpu
@pytest.mark.parametrize("n_regs", [5, 300])
def test_indexed_registrations_carry_the_bits_of_the_expanded_batch(gpu_ctx, frames, sample_pc, n_regs):
    """n_regs = 5: small batch (graph replay applies, and the replay must read the new keyframe index); 300: the throughput path."""
    import icet_amd
    from icet_amd import api
    dev = torch.device("cuda", 0)
    kf, partner = _keyframes(dev, frames, sample_pc)
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    kf_index = _mapping(n_regs, 4, 11)
    d2, x0 = _registrations(kf, partner, kf_index, 12)
    ref = _expanded(kf, kf_index, d2, x0, prm, dev)
    assert bool(torch.isfinite(ref).all())
    ctx = icet_amd.Context(0)
    ctx.keyframe_device([_desc(t) for t in kf], prm)
    for _ in range(3):                                               # eager, captured + replayed, replayed (small batch)
        assert torch.equal(_indexed(ctx, kf_index, d2, x0, prm, dev), ref)
    if n_regs <= 8:
        # same sizes, other keyframes: the launch key is the same, so a replay must take the new index from the staging
        other = [kf_index[(r + 1) % n_regs] for r in range(n_regs)]
        d2o = [d2[(r + 1) % n_regs] for r in range(n_regs)]
        x0o = np.roll(x0, -1, axis=0).copy()
        assert torch.equal(_indexed(ctx, other, d2o, x0o, prm, dev), ref[[(r + 1) % n_regs for r in range(n_regs)]])
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flag,n_regs", [("TRUE_SORT", 6), ("REJECT_MOVING", 6), ("DOUBLE_W", 6), ("ROUNDTRIP_SCAN2", 6), ("ROUNDTRIP_SCAN2", 70)])
def test_indexed_registrations_with_flags(gpu_ctx, frames, sample_pc, flag, n_regs):
    import icet_amd
    from icet_amd import api
    dev = torch.device("cuda", 0)
    kf, partner = _keyframes(dev, frames, sample_pc)
    kf, partner = kf[1:], partner[1:]                                # three keyframes
    f = getattr(api, "FLAG_" + flag)
    prm = api.Params(9, 24, 75, 25, 0.1, 0.1, f)
    kf_index = _mapping(n_regs, 3, 21)
    d2, x0 = _registrations(kf, partner, kf_index, 22)
    ref = _expanded(kf, kf_index, d2, x0, prm, dev)
    assert bool(torch.isfinite(ref).all())
    ctx = icet_amd.Context(0)
    ctx.keyframe_device([_desc(t) for t in kf], prm)
    assert torch.equal(_indexed(ctx, kf_index, d2, x0, prm, dev), ref)
    assert torch.equal(_indexed(ctx, kf_index, d2, x0, prm, dev), ref)
    ctx.close()


@pytest.mark.gpu
def test_parked_keyframe_survives_indexed_calls_and_refusals(gpu_ctx, frames, sample_pc):
    import icet_amd
    from icet_amd import api
    dev = torch.device("cuda", 0)
    kf, partner = _keyframes(dev, frames, sample_pc)
    kf, partner = kf[:3], partner[:3]
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    d1 = [_desc(t) for t in kf]; d2 = [_desc(t) for t in partner]
    xd = torch.zeros((3, 6), dtype=torch.float32, device=dev); xd[:, 0] = torch.tensor([0.0, 0.02, -0.01], device=dev)
    ctx = icet_amd.Context(0)
    ctx.keyframe_device(d1, prm)

    def register():
        out = torch.zeros((3, 48), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.register_device(d2, prm, out.data_ptr(), xd.data_ptr()); ctx.sync()
        return out

    before = register()
    assert bool(torch.isfinite(before).all())
    # two indexed calls with different mappings; the second one is larger than anything so far: the registration side grows, the keyframe stays
    for kf_index, seed in (([2, 0, 1, 1], 31), (_mapping(40, 3, 32), 33)):
        d2i, x0 = _registrations(kf, partner, kf_index, seed)
        assert torch.equal(_indexed(ctx, kf_index, d2i, x0, prm, dev), _expanded(kf, kf_index, d2i, x0, prm, dev))
    assert torch.equal(register(), before)
    out = torch.zeros((2, 48), dtype=torch.float32, device=dev)
    with pytest.raises(icet_amd.IcetError) as e:                     # index out of range
        ctx.register_indexed_device([0, 3], d2[:2], prm, out.data_ptr())
    assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError) as e:
        ctx.register_indexed_device([-1, 0], d2[:2], prm, out.data_ptr())
    assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError) as e:                     # other grid than the parked keyframe's
        ctx.register_indexed_device([0, 1], d2[:2], api.Params(7, 48, 150, 25, 0.1, 0.1, 0), out.data_ptr())
    assert e.value.status == api.ICET_ERR_BAD_ARG
    with pytest.raises(icet_amd.IcetError) as e:                     # keyframe-shaping flag differs
        ctx.register_indexed_device([0, 1], d2[:2], api.Params(7, 24, 75, 25, 0.1, 0.1, api.FLAG_TRUE_SORT), out.data_ptr())
    assert e.value.status == api.ICET_ERR_BAD_ARG
    ctx.set_option("keep", 1)
    with pytest.raises(icet_amd.IcetError) as e:                     # the indexed loop has no keep list
        ctx.register_indexed_device([0, 1], d2[:2], prm, out.data_ptr())
    assert e.value.status == api.ICET_ERR_UNSUPPORTED
    ctx.set_option("keep", 0)
    assert torch.equal(register(), before)
    ctx.register_indexed_device([], [], prm, out.data_ptr())        # n_regs == 0: nothing
    x0 = torch.tensor([[0.1, 0, 0, 0, 0, 0.01], [0, 0.2, 0, 0, 0, 0]], dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.register_indexed_device([1, 1], d2[:2], api.Params(0, 24, 75, 25, 0.1, 0.1, 0), out.data_ptr(), x0.data_ptr()); ctx.sync()
    assert torch.equal(out[:, :6], x0) and not bool(out[:, 6:].any())  # runlen == 0: X = X0
    assert torch.equal(register(), before)
    ctx.solve_batch_device(d1[:1], d2[:1], prm, out.data_ptr()); ctx.sync()
    with pytest.raises(icet_amd.IcetError) as e:                     # a whole solve un-parks the keyframe
        ctx.register_indexed_device([0, 0], d2[:2], prm, out.data_ptr())
    assert e.value.status == api.ICET_ERR_BAD_ARG
    ctx.close()


@pytest.mark.gpu
def test_multi_start_on_the_sample_pair(gpu_ctx, sample_pc):
    """One keyframe, five starts (the reference's sample pair only converges from a start near the answer): each start carries the bits of the
    single-pair solve from that X0, and the 0.6 m start reaches 0.645 m (test_nonzero_x0_and_longer_run)."""
    import icet_amd
    a, b = sample_pc
    starts = [0.0, 0.2, 0.4, 0.6, 0.8]
    X0 = np.zeros((5, 6), np.float32); X0[:, 0] = starts
    ctx = icet_amd.Context(0)
    res = ctx.solve_indexed([a], [b] * 5, [0] * 5, 12, X0=X0)
    ctx.close()
    for r in range(5):
        single = gpu_ctx.solve(a, b, 12, X0[r], 24, 75)
        assert np.array_equal(res["X"][r], single["X"]), (r, res["X"][r], single["X"])
        assert np.array_equal(res["pred_stds"][r], single["pred_stds"])
        assert np.array_equal(res["cov"][r], single["cov"])
    assert abs(res["X"][3][0] - 0.645) < 0.01
