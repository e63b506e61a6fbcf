"""Growth of the context's and the keyframe store's buffers (icet_amd/csrc/icet_buffers.h: owned groups, one free path).  One context is taken through a sequence
of calls that grows every group of the device-resident path -- pair tables, registration side, scan-1 arrays, what depends on both, the scan-2 overflow list,
thresholds and LUT, counts and tile tables -- each followed by a call that grows nothing; every result must carry the bits a FRESH context gives for the same call.
One store grows by reserve() and must then hold, and give, the bytes of a store created at the final capacity.  Small scans: a few seconds in all.  (A refused
allocation is not provoked here: tests/test_buffer_group_host.py covers that path on the host.)"""
import numpy as np
import pytest
import torch

DEV = torch.device("cuda", 0)
COARSE, FINE = (12, 40), (30, 90)          # bins_phi x bins_theta: 480 and 2700 voxels around the default's 1800, far below the limit of 10000
N_MIN = 8                                  # rows that make a voxel: small scans on a fine grid still fit a few hundred voxels


def _desc(t):
    return (t.data_ptr(), t.shape[1], t.shape[1])


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def scans():
    """Three pairs of 16 x 256 = 4096 rays and three of 16 x 512 = 8192 rays (the simulator drops the rays that hit nothing: ~3700 and ~7400 rows, odd sizes), on
    the device."""
    from icet_amd import lidar_sim as ls
    small = [ls.make_pair(scene_seed=1000 + k, noise_seed=2000 + k, rings=16, steps=256, device=DEV)[:2] for k in range(3)]
    large = [ls.make_pair(scene_seed=1000 + k, noise_seed=3000 + k, rings=16, steps=512, device=DEV)[:2] for k in range(3)]
    assert all(3000 < a.shape[1] <= 4096 and 3000 < b.shape[1] <= 4096 for a, b in small) and all(6000 < a.shape[1] <= 8192 and 6000 < b.shape[1] <= 8192 for a, b in large)
    torch.cuda.synchronize()
    return small, large


def _solve(ctx, pairs, prm):
    """icet_solve_batch_device of the pairs from small deterministic starts: (n, 48) floats."""
    n = len(pairs)
    x0 = torch.zeros((n, 6), dtype=torch.float32, device=DEV); x0[:, 0] = 0.01 * torch.arange(n, device=DEV)
    out = torch.full((n, 48), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.solve_batch_device([_desc(a) for a, _ in pairs], [_desc(b) for _, b in pairs], prm, out.data_ptr(), x0.data_ptr())
    ctx.sync()
    return out


def _indexed(ctx, pairs, prm):
    """icet_keyframe_device of the pairs' first scans, then n + 2 indexed registrations (more registrations than keyframes, out of order, with repeats)."""
    n = len(pairs)
    kf_of = [(n - 1 - r) % n for r in range(n + 2)]
    x0 = torch.zeros((n + 2, 6), dtype=torch.float32, device=DEV); x0[:, 1] = 0.005 * torch.arange(n + 2, device=DEV)
    out = torch.full((n + 2, 48), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.keyframe_device([_desc(a) for a, _ in pairs], prm)
    ctx.register_indexed_device(kf_of, [_desc(pairs[k][1]) for k in kf_of], prm, out.data_ptr(), x0.data_ptr())
    ctx.sync()
    return out


@pytest.mark.gpu
def test_one_context_through_every_growth_gives_the_bits_of_fresh_contexts(scans):
    import icet_amd
    from icet_amd import api
    small, large = scans
    prm = lambda grid: api.Params(5, grid[0], grid[1], N_MIN, 0.1, 0.1, 0)
    steps = (("1 pair", small[:1], COARSE),                     # everything is allocated
             ("3 pairs: the pair tables grow", small, COARSE),
             ("the finer grid: V grows", small, FINE),
             ("the larger scans: n1 and n2 grow", large, FINE),
             ("1 pair on the coarse grid: nothing grows", small[:1], COARSE))
    fresh = {}

    def reference(call, pairs, grid, key):
        if key not in fresh:                                     # computed once per distinct call, on a context that has seen nothing else
            ref = icet_amd.Context(0)
            fresh[key] = call(ref, pairs, prm(grid)).clone()
            ref.close()
        return fresh[key]

    ctx = icet_amd.Context(0)
    try:
        for name, pairs, grid in steps:
            for call in (_solve, _indexed):
                want = reference(call, pairs, grid, (call.__name__, len(pairs), pairs[0][0].shape[1], grid))
                assert torch.isfinite(want).all() and float(want[:, :6].abs().max()) > 1e-3, (name, call.__name__)      # (a solve that did something)
                for again in (False, True):                      # the call that grows, then the same call growing nothing (captured as a graph, then replayed)
                    got = call(ctx, pairs, prm(grid))
                    assert torch.equal(_bits(got), _bits(want)), (name, call.__name__, "repeat" if again else "first")
                got = call(ctx, pairs, prm(grid))
                assert torch.equal(_bits(got), _bits(want)), (name, call.__name__, "third")
    finally:
        ctx.close()


def _store_scans(scans):
    small, _ = scans
    kf = [small[0][0], small[1][0], small[2][0], small[0][1], small[1][1]]      # the keyframes of slots 0, 1, 2 and, later, 9 and 12
    reg = [small[1][1], small[1][0]]                                            # registered against slot 1 (old) and slot 12 (new)
    return kf, reg


def _fill(store, kf, features, reserve):
    if features:
        store.enable_appearance(); store.enable_coarse()
    store.put_device([0, 1, 2], [_desc(t) for t in kf[:3]])
    store._ctx.sync()
    before = _carried(store, features)
    if reserve:
        store.reserve(16)
    store.put_device([9, 12], [_desc(t) for t in kf[3:]])
    store._ctx.sync()
    return before


def _carried(store, features):
    """The bytes of slots 0, 1, 2: the four keyframe tables and, with the features on, descriptor, weights and grid."""
    rows = []
    for s in (0, 1, 2):
        row = [np.int64(store.debug_fetch(s, "n_slots")), store.debug_fetch(s, "hot").copy(), store.debug_fetch(s, "fit").copy(), store.debug_fetch(s, "slot_of_voxel").copy()]
        if features:
            row += [store.debug_fetch(s, "descriptor").copy(), store.debug_fetch(s, "weights").copy().view(np.uint32), store.debug_fetch(s, "grid").copy()]
        rows.append(row)
    return rows


def _same(a, b):
    return all(len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("features", [False, True], ids=["tables", "appearance+coarse"])
def test_a_reserved_store_is_a_store_created_at_that_capacity(scans, features):
    import icet_amd
    from icet_amd import api
    kf, reg = _store_scans(scans)
    prm = api.Params(5, 24, 75, N_MIN, 0.1, 0.1, 0)
    x0 = torch.zeros((2, 6), dtype=torch.float32, device=DEV); x0[1, 0] = 0.02
    results = []
    for reserve in (True, False):
        ctx = icet_amd.Context(0)
        store = api.KeyframeStore(ctx, 4 if reserve else 16, n=N_MIN)
        try:
            before = _fill(store, kf, features, reserve)
            after = _carried(store, features)
            assert _same(before, after)                          # the carried slots, byte for byte
            if features:                                         # ... and they are the descriptors and grids of the scans that were put
                D, w = store.describe([t.T.cpu().numpy() for t in kf[:3]])
                G = store.coarse_grid([t.T.cpu().numpy() for t in kf[:3]])
                for s in range(3):
                    assert np.array_equal(after[s][4], D[s]) and np.array_equal(after[s][5], w[s].view(np.uint32)) and np.array_equal(after[s][6], G[s])
            out = torch.full((2, 48), float("nan"), dtype=torch.float32, device=DEV)
            torch.cuda.synchronize()
            store.register_device([1, 12], [_desc(t) for t in reg], prm, out.data_ptr(), x0.data_ptr())
            ctx.sync()
            assert torch.isfinite(out).all() and float(out[:, :6].abs().max()) > 1e-3
            results.append((after, _bits(out).cpu()))
        finally:
            store.close(); ctx.close()
    assert _same(results[0][0], results[1][0])
    assert torch.equal(results[0][1], results[1][1])
