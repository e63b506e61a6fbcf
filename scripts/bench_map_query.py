#!/usr/bin/env python3
"""The voxel map's query on one GPU, variants alternating in one process (GPU box):

    python scripts/bench_map_query.py [--scans 256] [--table-log2 24] [--cell 0.1] [--reps 7] [--range 30] [--out FILE.json]

The map: the --scans synthetic 64-channel scans of scripts/bench_map.py (lidar_sim, scene 2000) along a drive, each at its own pose, about 634 k cells.
  (1) index       icet_voxel_map_index of a stale index (a one-row add and its remove in front of every window make it stale and leave the map as it was).
  (2) query       one icet_voxel_map_query_device call of Q = 1 and Q = 32 poses at max_range --range, option "map_query_prune" 1 against 0, and the count-only
                  form; the poses are those of scans spread evenly over the drive.
  (3) put         KeyframeStore.put_from_map of 32 slots (query + put, the row counts on the device).
  (4) yardstick   what the tree offered before for ONE sub-map: clear + add of the neighbouring scans at poses relative to the middle one into a second map +
                  extract_device -- with 16 neighbours and with every scan (the sub-map of (2) holds cells of every scan in range).
  (5) accuracy    8 scans 0.4 m apart (rings 64, steps 1024): each registered against the sub-map around its own true pose (of a map of all 8 at their true
                  poses) from a start a few centimetres off, beside the same scan registered against its raw predecessor through the store's scan-to-scan
                  path from a start equally far off.  Pose errors in metres and radians.  No bound: none has been measured.
A window is ONE call (or the calls named) between two HIP events on the context's stream, behind 2 warm-up rounds; the figure is the median of --reps windows.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--table-log2", type=int, default=24)
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--range", type=float, default=30.0)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import icet_amd
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_query: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    scene = lidar_sim.make_scene(2000)

    def pose_of(t, yaw):
        T = np.eye(4); T[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]; T[:3, 3] = t
        return T

    scans, poses = [], []
    for k in range(a.scans):
        t = np.array([-20.0 + 0.15 * k, -1.0 + 0.01 * k, 0.0])
        T = pose_of(t, 0.01 * k)
        scans.append(lidar_sim.make_scan(scene, (t, T[:3, :3]), 50 + k, rings=a.rings, steps=a.steps, device=dev).contiguous())
        poses.append(T.astype(np.float32))
    poses = np.stack(poses)
    torch.cuda.synchronize()
    descs = [(s.data_ptr(), s.shape[1], s.shape[1]) for s in scans]

    ctx = api.Context(0)
    stream = torch.cuda.ExternalStream(api.load_library().icet_stream(ctx._h), device=dev)
    m = api.VoxelMap(ctx, cell=a.cell, table_log2=a.table_log2)
    m.add_device(descs, poses)
    cells = m.index()["cells_out"]

    def timed(fn, before=None):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(fns, before=None):
        for _ in range(2):
            for fn in fns.values():
                timed(fn, before)
        t = {k: [] for k in fns}
        for _ in range(a.reps):                                      # alternating
            for k, fn in fns.items():
                t[k].append(timed(fn, before))
        return {k: float(np.median(v)) for k, v in t.items()}, {k: [float(min(v)), float(max(v))] for k, v in t.items()}

    result = dict(scans=a.scans, cells=cells, cell=a.cell, table_log2=a.table_log2, reps=a.reps, max_range=a.range)

    # (1) the index
    one = torch.tensor([[1.0], [2.0], [3.0]], dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    one_desc = [(one.data_ptr(), 1, 1)]

    def stale():
        m.add_device(one_desc, poses[:1]); m.remove_device(one_desc, poses[:1])
    med, spread = measure({"index": m.index}, before=stale)
    result["index"] = dict(ms=med["index"], range_ms=spread["index"])
    print("(1) index of %d cells: %.3f ms" % (cells, med["index"]), flush=True)

    # (2) the query
    def buffers(T):
        q = T.shape[0]
        w = torch.zeros((3, q), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        m.query_device(T, [(None, 0, 0)] * q, w[0].data_ptr(), max_range=a.range, d_total_ptr=w[1].data_ptr())
        ctx.sync()
        tot = [int(v) for v in w[1].cpu().numpy()]
        x = [torch.zeros((3, max(t, 1)), dtype=torch.float32, device=dev) for t in tot]
        torch.cuda.synchronize()
        return w, x, [(b.data_ptr(), max(t, 1), t) for b, t in zip(x, tot)], tot

    fns, keep = {}, []
    for q in (1, 32):
        T = poses[np.linspace(0, a.scans - 1, q + 2).astype(int)[1:-1]]
        w, x, outs, tot = buffers(T)
        keep.append((w, x))
        result["query_%d_rows" % q] = tot
        for prune in (1, 0):
            def fn(T=T, outs=outs, w=w, prune=prune):
                ctx.set_option("map_query_prune", prune)
                m.query_device(T, outs, w[0].data_ptr(), max_range=a.range, d_total_ptr=w[1].data_ptr(), d_status_ptr=w[2].data_ptr())
            fns["q%d_prune%d" % (q, prune)] = fn

        def count_only(T=T, w=w, q=q):
            ctx.set_option("map_query_prune", 1)
            m.query_device(T, [(None, 0, 0)] * q, w[0].data_ptr(), max_range=a.range, d_total_ptr=w[1].data_ptr())
        fns["q%d_count_only" % q] = count_only
    med, spread = measure(fns)
    ctx.set_option("map_query_prune", 1)
    result["query"] = {k: dict(ms=med[k], range_ms=spread[k]) for k in fns}
    print("(2) query at %.0f m: " % a.range + "   ".join("%s %.3f ms" % (k, med[k]) for k in fns), flush=True)
    print("    rows: Q = 1 %s   Q = 32 %d .. %d" % (result["query_1_rows"], min(result["query_32_rows"]), max(result["query_32_rows"])), flush=True)

    # (3) sub-maps into a store
    store = icet_amd.KeyframeStore(ctx, 32)
    T32 = poses[np.linspace(0, a.scans - 1, 34).astype(int)[1:-1]]
    cap = max(result["query_32_rows"]) + 1024
    med, spread = measure({"put_from_map": lambda: store.put_from_map(list(range(32)), m, T32, a.range, cap_rows=cap)})
    result["put_from_map_32"] = dict(ms=med["put_from_map"], range_ms=spread["put_from_map"], cap_rows=cap)
    print("(3) put_from_map of 32 slots: %.3f ms" % med["put_from_map"], flush=True)
    store.close()

    # (4) the yardstick: one sub-map the old way
    second = api.VoxelMap(ctx, cell=a.cell, max_range=0.0, table_log2=a.table_log2)
    mid = a.scans // 2
    inv_mid = np.linalg.inv(poses[mid].astype(np.float64))
    rel = np.stack([(inv_mid @ poses[k].astype(np.float64)).astype(np.float32) for k in range(a.scans)])
    out = torch.zeros((3, cells + 65536), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def old_way(lo, hi):
        def fn():
            second.clear(); second.add_device(descs[lo:hi], rel[lo:hi]); second.extract_device(out.data_ptr(), out.shape[1], out.shape[1])
        return fn
    med, spread = measure({"yard_16": old_way(max(mid - 8, 0), min(mid + 8, a.scans)), "yard_all": old_way(0, a.scans)})
    result["yardstick"] = {k: dict(ms=med[k], range_ms=spread[k]) for k in med}
    print("(4) clear + add + extract into a second map: 16 neighbours %.3f ms   all %d scans %.3f ms" % (med["yard_16"], a.scans, med["yard_all"]), flush=True)
    second.close(); m.close()

    # (5) localisation accuracy
    sgn = 1.0 if api.pose_step_from_X([0, 0, 0, 0, 0, 0.1])[1, 0] > 0 else -1.0      # the sign of X's yaw in a pose step

    def start_of(T_rel, off):
        """An X whose pose step is T_rel (yaw-only), moved by off."""
        R = T_rel[:3, :3].astype(np.float64)
        X = np.zeros(6); X[:3] = R.T @ T_rel[:3, 3]; X[5] = sgn * np.arctan2(R[1, 0], R[0, 0])
        return (X + off).astype(np.float32)

    def pose_error(X, T_rel):
        E = api.pose_step_from_X(X).astype(np.float64)
        dR = E[:3, :3].T @ T_rel[:3, :3]
        return float(np.linalg.norm(E[:3, 3] - T_rel[:3, 3])), float(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))

    ds, dp = [], []
    for k in range(8):
        t = np.array([-5.0 + 0.4 * k, -1.0, 0.0])
        T = pose_of(t, 0.02 * k)
        ds.append(lidar_sim.make_scan(scene, (t, T[:3, :3]), 70 + k, rings=64, steps=1024, device=dev).contiguous()); dp.append(T.astype(np.float32))
    dp = np.stack(dp)
    torch.cuda.synchronize()
    dd = [(s.data_ptr(), s.shape[1], s.shape[1]) for s in ds]
    dm = api.VoxelMap(ctx, cell=a.cell, table_log2=22)
    dm.add_device(dd, dp)
    store = icet_amd.KeyframeStore(ctx, 16)
    store.put_from_map(list(range(8)), dm, dp, a.range)
    store.put_device(list(range(8, 16)), dd)
    off = np.array([0.03, -0.02, 0.01, 0.0, 0.0, 0.003])
    P = api.Params(7, 24, 75, 25, 0.1, 0.1, 0)
    acc = []
    for k in range(1, 8):
        T_prev = np.linalg.inv(dp[k - 1].astype(np.float64)) @ dp[k].astype(np.float64)
        x0 = torch.from_numpy(np.stack([start_of(np.eye(4), off), start_of(T_prev, off)])).to(dev)
        res = torch.zeros((2, 48), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        store.register_device([k, 8 + k - 1], [dd[k], dd[k]], P, res.data_ptr(), x0.data_ptr())
        ctx.sync()
        X = res.cpu().numpy()[:, :6]
        e_map, e_raw = pose_error(X[0], np.eye(4)), pose_error(X[1], T_prev)
        s_map, s_raw = pose_error(x0.cpu().numpy()[0], np.eye(4)), pose_error(x0.cpu().numpy()[1], T_prev)
        acc.append(dict(scan=k, submap_m=e_map[0], submap_rad=e_map[1], raw_m=e_raw[0], raw_rad=e_raw[1], start_m=s_map[0], start_rad=s_map[1], raw_start_m=s_raw[0]))
        print("(5) scan %d: against its sub-map %.4f m %.5f rad   against raw scan %d %.4f m %.5f rad   (starts %.4f m / %.4f m off)"
              % (k, e_map[0], e_map[1], k - 1, e_raw[0], e_raw[1], s_map[0], s_raw[0]), flush=True)
    result["accuracy"] = acc
    store.close(); dm.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
