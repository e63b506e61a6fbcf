#!/usr/bin/env python3
"""The voxel map's shape on one GPU, on bench_map.py's workload, the forms alternating in one process (GPU box):

    python scripts/bench_map_shape.py [--scans 256] [--table-log2 24] [--cell 0.1] [--reps 7] [--out FILE.json]

The workload: --scans synthetic 64-channel scans (lidar_sim, scene 2000, about 116 k rows each) along a drive, every one at its own pose.
  (1) add      one icet_voxel_map_add_device call of all scans into a cleared map: a plain map against a shaped one, option "map_lds" 1 and 0 -- four forms.
               A shaped flush issues 13 atomics per distinct (block, cell) pair where the plain one issues 4; the pairs are counted here with torch.
  (2) extract  icet_voxel_map_extract_device against icet_voxel_map_extract_shape_device (all four shape columns) of the shaped map.
A window is ONE call between two HIP events on the context's stream, behind 2 warm-up rounds; the figure is the median of --reps windows.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS_PER_BLOCK = 2048                                                 # kRowsPerBlock of icet_map.hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--table-log2", type=int, default=24)
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_shape: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    scene = lidar_sim.make_scene(2000)
    scans, poses = [], []
    for k in range(a.scans):
        t = np.array([-20.0 + 0.15 * k, -1.0 + 0.01 * k, 0.0]); yaw = 0.01 * k
        T = np.eye(4); T[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]; T[:3, 3] = t
        scans.append(lidar_sim.make_scan(scene, (t, T[:3, :3]), 50 + k, rings=a.rings, steps=a.steps, device=dev).contiguous())
        poses.append(T.astype(np.float32))
    poses = np.stack(poses)
    torch.cuda.synchronize()
    descs = [(s.data_ptr(), s.shape[1], s.shape[1]) for s in scans]
    rows = int(sum(s.shape[1] for s in scans))

    pairs = 0                                                         # the distinct (block, cell) pairs of the call, as bench_map.py counts them
    for s, T in zip(scans, poses):
        p = s.to(torch.float64)
        Td = torch.from_numpy(T.astype(np.float64)).to(dev)
        keep = (p * p).sum(0) > 0
        c = torch.floor((Td[:3, :3] @ p + Td[:3, 3:4]) / float(np.float32(a.cell))).to(torch.int64) + (1 << 20)
        key = (c[0] << 42) | (c[1] << 21) | c[2]
        block = torch.arange(s.shape[1], device=dev) // ROWS_PER_BLOCK
        pairs += int(torch.unique(torch.stack([block[keep], key[keep]]), dim=1).shape[1])

    ctx = api.Context(0)
    stream = torch.cuda.ExternalStream(api.load_library().icet_stream(ctx._h), device=dev)
    maps = dict(plain=api.VoxelMap(ctx, cell=a.cell, table_log2=a.table_log2), shaped=api.VoxelMap(ctx, cell=a.cell, table_log2=a.table_log2, shape=True))

    def timed(fn, before=None):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(fns):
        for _ in range(2):
            for fn, before in fns.values():
                timed(fn, before)
        t = {k: [] for k in fns}
        for _ in range(a.reps):                                      # alternating
            for k, (fn, before) in fns.items():
                t[k].append(timed(fn, before))
        return {k: float(np.median(v)) for k, v in t.items()}, {k: [float(min(v)), float(max(v))] for k, v in t.items()}

    result = dict(scans=a.scans, rows=rows, cell=a.cell, table_log2=a.table_log2, reps=a.reps, block_cell_pairs=pairs)

    def add(name, lds):
        def fn():
            ctx.set_option("map_lds", lds)
            maps[name].add_device(descs, poses)
        return fn, maps[name].clear
    med, spread = measure({"%s_lds%d" % (n, l): add(n, l) for l in (1, 0) for n in ("plain", "shaped")})
    ctx.set_option("map_lds", 1)
    st = maps["shaped"].stats()
    assert st == maps["plain"].stats()
    result["add"] = dict(ms=med, range_ms=spread, shaped_over_plain_lds1=med["shaped_lds1"] / med["plain_lds1"], shaped_over_plain_lds0=med["shaped_lds0"] / med["plain_lds0"],
                         stats=st)
    print("(1) add of %d scans, %d rows, %d cells, %d (block, cell) pairs" % (a.scans, rows, st["cells_occupied"], pairs))
    for l in (1, 0):
        print("    map_lds %d: plain %.3f ms   shaped %.3f ms   ratio %.2f" % (l, med["plain_lds%d" % l], med["shaped_lds%d" % l], med["shaped_lds%d" % l] / med["plain_lds%d" % l]),
              flush=True)

    n = st["cells_out"]
    xyz = torch.zeros((3, n), dtype=torch.float32, device=dev); cnt = torch.zeros(n, dtype=torch.int64, device=dev); key = torch.zeros(n, dtype=torch.int64, device=dev)
    fl = torch.zeros((12, n), dtype=torch.float32, device=dev); mom = torch.zeros((9, n), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    m = maps["shaped"]
    med, spread = measure({"extract": (lambda: m.extract_device(xyz.data_ptr(), n, n, 1, cnt.data_ptr(), key.data_ptr()), None),
                           "extract_shape": (lambda: m.extract_shape_device(xyz.data_ptr(), n, n, 1, cnt.data_ptr(), key.data_ptr(), fl[0:6].data_ptr(), fl[6:9].data_ptr(),
                                                                            fl[9:12].data_ptr(), mom.data_ptr()), None)})
    result["extract"] = dict(cells=n, ms=med, range_ms=spread)
    print("(2) %d cells: extract %.3f ms   extract_shape %.3f ms" % (n, med["extract"], med["extract_shape"]), flush=True)
    for v in maps.values():
        v.close()
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
