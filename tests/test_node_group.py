"""Node groups (include/icet_nodes.h, icet_node_group_*): many lidar streams advanced in one call.  The contract: every stream behaves exactly like its own
icet_node with the same parameters fed the same frames in the same order -- the same BITS in every result field and in the map, previous scan, aligned cloud
and snail trail.  The GPU tests check that against S independent api.Node objects; the CPU tests check the ABI, the Python and the C++ surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch   # before libicet_hip.so is loaded: both must share one HIP runtime (torch ships its own libamdhip64)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_SYMBOLS = ("icet_node_group_create", "icet_node_group_destroy", "icet_node_group_last_error", "icet_node_group_push_device", "icet_node_group_map",
                 "icet_node_group_prev_scan", "icet_node_group_aligned", "icet_node_group_snail_trail")


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_group_symbols_exported_and_refuse_bad_handles():
    import icet_amd
    from icet_amd import api
    L = icet_amd.load_library()
    for name in GROUP_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS and getattr(L, name) is not None
    p = api.node_params(**api.ODOMETRY_NODE)
    h = C.c_void_p()
    # no context, no params, no out pointer, n_streams <= 0: refused before any device is touched
    assert L.icet_node_group_create(None, C.byref(p), 4, C.byref(h)) == api.ICET_ERR_BAD_ARG and not h.value
    assert L.icet_node_group_create(None, None, 4, C.byref(h)) == api.ICET_ERR_BAD_ARG
    assert L.icet_node_group_create(None, C.byref(p), 0, C.byref(h)) == api.ICET_ERR_BAD_ARG
    assert L.icet_node_group_create(None, C.byref(p), -3, C.byref(h)) == api.ICET_ERR_BAD_ARG
    assert L.icet_node_group_create(None, C.byref(p), 4, None) == api.ICET_ERR_BAD_ARG
    assert L.icet_node_group_destroy(None) == api.ICET_ERR_BAD_ARG
    assert L.icet_node_group_last_error(None) == b""
    ids = (C.c_int32 * 1)(0); fr = (api.DevScan * 1)(); res = (api.NodeResult * 1)()
    assert L.icet_node_group_push_device(None, 1, ids, fr, res) == api.ICET_ERR_BAD_ARG
    rows = C.c_int64()
    for name in ("icet_node_group_map", "icet_node_group_prev_scan", "icet_node_group_aligned", "icet_node_group_snail_trail"):
        assert getattr(L, name)(None, 0, None, 0, C.byref(rows)) == api.ICET_ERR_BAD_ARG


def test_python_node_group_surface():
    from icet_amd import api
    assert hasattr(api, "NodeGroup")
    for m in ("push_device", "map", "prev_scan", "aligned", "snail_trail", "close"):
        assert callable(getattr(api.NodeGroup, m)), m


def test_cpp_node_group_compiles(tmp_path):
    src = tmp_path / "g.cpp"
    src.write_text('#include "icet_nodes.hpp"\n'
                   'int main() {\n'
                   '  icet_amd::NodeGroup g(icet_node_params{{7, 24, 75, 25, 0.1f, 0.1f, ICET_FLAG_NONE}, 2.0f, 1, 0.f, 0.f, 0, 0, 0}, 4);\n'
                   '  std::vector<int32_t> ids{2, 0}; std::vector<icet_dev_scan> frames(2, icet_dev_scan{nullptr, 0, 0}); std::vector<icet_node_result> res;\n'
                   '  const bool ok = g.pushDevice(ids, frames, res);\n'
                   '  int64_t rows = 0; std::vector<float> m = g.mapPC(0, &rows); std::vector<float> s = g.prevScan(1, &rows);\n'
                   '  return ok && g.streams() == 4 && m.empty() && s.empty() ? 0 : 1;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)])


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------

MOTION = (0.25, 0.02, 0.005, 0.001, -0.001, 0.006)


def _drive(s, n_frames, rings=32, steps=1024):
    """Stream s's synthetic drive: a scene and noise of its own, frames on the device as (3, N) float32 tensors."""
    from icet_amd import lidar_sim as ls
    return [t.to("cuda:0").contiguous() for t in ls.make_sequence(n_frames, scene_seed=3000 + 11 * s, noise_seed=5000 + 11 * s, motion=MOTION, rings=rings, steps=steps)]


def _frame(s, t):
    n = int(t.shape[1])
    return (s, t.data_ptr() if n else 0, n, n)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_result(rg, rn, where):
    for k in ("solved", "diverged", "n_kept", "map_rows"):
        assert rg[k] == rn[k], (where, k, rg[k], rn[k])
    for k in ("X", "pred_stds", "pose", "quat"):
        assert np.array_equal(_u32(rg[k]), _u32(rn[k])), (where, k, rg[k], rn[k])


class _Twin:
    """A group of S streams next to S independent nodes with the same parameters; every call goes to both and is compared bit for bit."""

    def __init__(self, ctx, S, **kw):
        from icet_amd import api
        self.kw = kw
        self.g = api.NodeGroup(ctx, S, **kw)
        self.nodes = [api.Node(ctx, **kw) for _ in range(S)]
        self.calls = 0

    def push(self, frames, check=("prev_scan",)):
        torch.cuda.synchronize()
        rg = self.g.push_device(frames)
        assert len(rg) == len(frames)
        for (s, p, n, ld), r in zip(frames, rg):
            rn = self.nodes[s].push_device(p, n, ld)
            _same_result(r, rn, (self.calls, s))
            for what in check:
                a, b = getattr(self.g, what)(s), getattr(self.nodes[s], what)()
                assert a.shape == b.shape and np.array_equal(_u32(a), _u32(b)), (self.calls, s, what)
        self.calls += 1
        return rg

    def close(self):
        self.g.close()
        for nd in self.nodes:
            nd.close()


@pytest.mark.gpu
def test_gpu_group_odometry_all_streams(gpu_ctx):
    """Five streams on distinct drives, 32- and 64-ring frames mixed (row counts differ), six calls that each carry every stream."""
    from icet_amd import api
    S = 5
    drives = [_drive(s, 6, rings=64 if s % 2 else 32) for s in range(S)]
    tw = _Twin(gpu_ctx, S, **api.ODOMETRY_NODE)
    for k in range(6):
        rg = tw.push([_frame(s, drives[s][k]) for s in range(S)])
        assert all(r["solved"] == (k > 0) for r in rg)
    tw.close()


@pytest.mark.gpu
def test_gpu_group_subsets_order_late_empty_and_growing(gpu_ctx):
    """Seeded random subsets in random id order; streams that start late; an empty frame; a frame larger than any before it (its buffers grow)."""
    from icet_amd import api
    S, calls = 6, 9
    drives = [_drive(s, calls, rings=32, steps=768) for s in range(S)]
    drives[1][4] = torch.zeros((3, 0), dtype=torch.float32, device="cuda:0")                       # an empty frame
    drives[2][3] = _drive(2, 1, rings=64, steps=2048)[0]                                             # larger than anything stream 2 (or any stream) saw before
    rs = np.random.RandomState(11)
    tw = _Twin(gpu_ctx, S, **api.ODOMETRY_NODE)
    pos = [0] * S
    for c in range(calls):
        live = [s for s in range(S) if c >= 3 or s < 4]                                              # streams 4 and 5 start at the fourth call
        pick = [int(s) for s in rs.permutation(live)[:rs.randint(1, len(live) + 1)]]
        for s in (1, 2):                                                                             # streams 1 and 2 every call, anywhere in the order: the empty
            if s not in pick:                                                                        # frame comes at the fifth call, the large one at the fourth
                pick.insert(int(rs.randint(0, len(pick) + 1)), s)
        frames = []
        for s in pick:
            frames.append(_frame(s, drives[s][pos[s]])); pos[s] += 1
        tw.push(frames)
    assert pos[1] > 4 and pos[2] > 3
    tw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("S", [3, 12])
def test_gpu_group_both_solve_paths(gpu_ctx, S):
    """S = 3: the loop of <= 8 pairs (captured graph path); S = 12: the throughput path.  Both bitwise."""
    from icet_amd import api
    drives = [_drive(s, 4, rings=32, steps=512) for s in range(S)]
    tw = _Twin(gpu_ctx, S, **api.ODOMETRY_NODE)
    for k in range(4):
        tw.push([_frame(s, drives[s][k]) for s in range(S)])
    tw.close()


@pytest.mark.gpu
def test_gpu_group_map_maker(gpu_ctx):
    """map_capacity 5000, map_downsample 2000: every ring wraps on the third frame.  Then the guard tripped on every frame (thresholds 1e-6)."""
    from icet_amd import api
    S = 4
    drives = [_drive(s, 5, rings=32, steps=1024) for s in range(S)]
    kw = dict(api.MAP_MAKER_NODE); kw.update(map_capacity=5000, map_downsample=2000, runlen=7)
    tw = _Twin(gpu_ctx, S, **kw)
    for k in range(5):
        order = list(range(S)) if k % 2 == 0 else list(reversed(range(S)))
        tw.push([_frame(s, drives[s][k]) for s in order], check=("prev_scan", "map"))
    tw.close()
    kw.update(trans_thresh=1e-6, rot_thresh=1e-6, map_capacity=4500)
    tw = _Twin(gpu_ctx, S, **kw)
    for k in range(4):
        rg = tw.push([_frame(s, drives[s][k]) for s in range(S)], check=("map",))
        assert all(r["diverged"] for r in rg) or k == 0
    tw.close()


@pytest.mark.gpu
def test_gpu_group_scan_registration_preset(gpu_ctx):
    """flags = 7 (no range filter, aligned cloud, snail trail) with NaN rows in the frames: aligned cloud and snail trail per stream, bitwise."""
    from icet_amd import api
    S = 3
    drives = [_drive(s, 4, rings=32, steps=768) for s in range(S)]
    for s in range(S):
        for k, t in enumerate(drives[s]):
            t[:, (7 + 13 * s + k)::997] = float("nan")
    tw = _Twin(gpu_ctx, S, **api.SCAN_REGISTRATION_NODE)
    for k in range(4):
        tw.push([_frame(s, drives[s][k]) for s in range(S)], check=("prev_scan", "aligned", "snail_trail"))
    tw.close()


@pytest.mark.gpu
def test_gpu_group_double_w_and_runlen0(gpu_ctx):
    """ICET_NODE_DOUBLE_W, and the scheduling flags (accepted, ignored: same bits)."""
    from icet_amd import api
    S = 2
    drives = [_drive(s, 3, rings=32, steps=512) for s in range(S)]
    for flags in (api.NODE_DOUBLE_W, api.NODE_NO_PIPELINE | api.NODE_SERIAL_ENQUEUE | api.NODE_TIME_PHASES):
        kw = dict(api.ODOMETRY_NODE); kw["flags"] = flags
        tw = _Twin(gpu_ctx, S, **kw)
        for k in range(3):
            tw.push([_frame(s, drives[s][k]) for s in range(S)])
        tw.close()


@pytest.mark.gpu
def test_gpu_group_refused_calls_leave_streams_alone(gpu_ctx):
    import icet_amd
    from icet_amd import api
    L = icet_amd.load_library()
    S = 3
    drives = [_drive(s, 3, rings=32, steps=512) for s in range(S)]
    h = C.c_void_p()
    p = api.node_params(**api.ODOMETRY_NODE)
    assert L.icet_node_group_create(gpu_ctx._h, C.byref(p), 0, C.byref(h)) == api.ICET_ERR_BAD_ARG
    tw = _Twin(gpu_ctx, S, **api.ODOMETRY_NODE)
    tw.push([_frame(s, drives[s][0]) for s in range(S)])
    torch.cuda.synchronize()

    def raw(ids, frames, n=None):
        k = len(frames) if n is None else n
        I = (C.c_int32 * max(len(ids), 1))(*ids)
        A = (api.DevScan * max(len(frames), 1))(*[api.DevScan(int(fp), int(fn), int(fl)) for (fp, fn, fl) in frames])
        R = (api.NodeResult * max(len(frames), 1))()
        return L.icet_node_group_push_device(tw.g._h, k, I, A, R)

    ok = [(drives[s][1].data_ptr(), drives[s][1].shape[1], drives[s][1].shape[1]) for s in range(S)]
    assert raw([0, 0], ok[:2]) == api.ICET_ERR_BAD_ARG                                               # duplicate id
    assert raw([0, S], ok[:2]) == api.ICET_ERR_BAD_ARG                                               # out of range
    assert raw([-1], ok[:1]) == api.ICET_ERR_BAD_ARG
    assert raw([0], ok[:1], n=-1) == api.ICET_ERR_BAD_ARG                                            # n < 0
    assert raw([0, 1], [ok[0], (0, 100, 100)]) == api.ICET_ERR_BAD_ARG                              # NULL scan with rows
    assert raw([0, 1], [ok[0], (ok[1][0], ok[1][1], ok[1][1] - 1)]) == api.ICET_ERR_BAD_ARG         # ld < n
    assert raw([0, 1], [ok[0], (ok[1][0], -1, 5)]) == api.ICET_ERR_BAD_ARG                           # n < 0 in a frame
    assert L.icet_node_group_push_device(tw.g._h, 2, None, None, None) == api.ICET_ERR_BAD_ARG      # NULL arrays with n > 0
    rows = C.c_int64()
    assert L.icet_node_group_prev_scan(tw.g._h, S, None, 0, C.byref(rows)) == api.ICET_ERR_BAD_ARG
    assert L.icet_node_group_map(tw.g._h, -1, None, 0, C.byref(rows)) == api.ICET_ERR_BAD_ARG
    out = np.zeros(3 * 8, np.float32)
    assert L.icet_node_group_prev_scan(tw.g._h, 0, out.ctypes.data_as(C.c_void_p), 8, C.byref(rows)) == api.ICET_ERR_BAD_ARG   # ld < rows
    assert L.icet_node_group_push_device(tw.g._h, 0, None, None, None) == api.ICET_OK                # nothing to do
    # every refused call left every stream as it was: the next valid calls still match the reference nodes bit for bit
    tw.push([_frame(s, drives[s][1]) for s in range(S)])
    tw.push([_frame(s, drives[s][2]) for s in reversed(range(S))])
    tw.close()


@pytest.mark.gpu
def test_gpu_group_one_stream_matches_cpu_node(gpu_ctx):
    """One stream of a group against the CPU node twin, with the tolerances of test_gpu_odometry_node_matches_oracle."""
    from oracle import pyoracle as po
    from icet_amd import api, lidar_sim as ls
    seq = [s.T.contiguous().numpy() for s in ls.make_sequence(4, motion=MOTION, rings=64, steps=2048)]
    g = api.NodeGroup(gpu_ctx, 2, **api.ODOMETRY_NODE)
    o = po.Node(**api.ODOMETRY_NODE)
    for k, s in enumerate(seq):
        t = torch.from_numpy(np.ascontiguousarray(s.T)).to("cuda:0")
        torch.cuda.synchronize()
        rg = g.push_device([(1, t.data_ptr(), len(s), len(s))])[0]
        ro = o.push(s)
        assert rg["solved"] == ro["solved"] and rg["n_kept"] == ro["n_kept"] and rg["diverged"] == ro["diverged"]
        if k:
            assert np.abs(rg["X"][:3] - ro["X"][:3]).max() <= 3e-4 * k and np.abs(rg["X"][3:] - ro["X"][3:]).max() <= 1e-4 * k, (k, rg["X"], ro["X"])
            assert np.allclose(rg["pred_stds"], ro["pred_stds"], rtol=2e-2, atol=1e-7)
            assert np.abs(rg["pose"] - ro["pose"]).max() <= 1e-3
            assert min(np.abs(rg["quat"] - ro["quat"]).max(), np.abs(rg["quat"] + ro["quat"]).max()) <= 1e-3
    assert g.prev_scan(0).shape == (0, 3)                                                            # the other stream was never named
    g.close(); o.close()


@pytest.mark.gpu
def test_gpu_done_word_waits_for_every_pair(gpu_ctx):
    """icet_sync behind a small batch (<= 8 pairs, replayed graph) watches the pinned word the solve's last kernel raises: it must be raised by the LAST pair to
    finish, not the first.  Pairs of very unequal size (a few hundred rows next to ~600 k) into pinned host memory, read at once after icet_sync; every pair must
    equal its single solve.  (A race guard: without the fix it can fail, not deterministically.)"""
    import icet_amd
    from icet_amd import api, lidar_sim as ls
    big = [t.to("cuda:0").contiguous() for t in ls.make_sequence(2, motion=MOTION, rings=128, steps=4800)]
    small = [t[:, ::2000].contiguous() for t in _drive(0, 2, rings=32, steps=1024)]
    prm = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    desc = lambda t: (t.data_ptr(), t.shape[1], t.shape[1])
    solo = {}
    ref = icet_amd.Context(0)
    d1 = torch.zeros(48, dtype=torch.float32, device="cuda:0")
    for i, pr in enumerate((big, small)):                                                            # each pair alone: 0 the big one, 1 the small one
        torch.cuda.synchronize()
        ref.solve_batch_device([desc(pr[0])], [desc(pr[1])], prm, d1.data_ptr())
        ref.sync()
        solo[i] = d1.cpu().numpy().copy()
    ref.close()
    for n in (2, 3, 5, 8):
        kinds = [(k % 2) for k in range(n)]                                                          # alternate big and small pairs
        s1 = [desc(big[0] if k == 0 else small[0]) for k in kinds]
        s2 = [desc(big[1] if k == 0 else small[1]) for k in kinds]
        out = torch.zeros(n * 48, dtype=torch.float32).pin_memory()
        for rep in range(4):                                                                         # the first call runs eagerly, the second is captured, then replays
            out.fill_(0.0)
            torch.cuda.synchronize()
            gpu_ctx.solve_batch_device(s1, s2, prm, out.data_ptr())
            gpu_ctx.sync()
            got = out.numpy().reshape(n, 48).copy()
            for k in range(n):
                assert np.array_equal(_u32(got[k]), _u32(solo[kinds[k]])), (n, rep, k)
