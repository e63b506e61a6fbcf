#!/usr/bin/env python3
"""The voxel map kept on one GPU, variants alternating in one process (GPU box):

    python scripts/bench_map_snapshot.py [--scans 256] [--table-log2 24] [--cell 0.1] [--reps 7] [--shape 1] [--dir DIR] [--out FILE.json]

The workload is bench_map.py's: --scans synthetic 64-channel scans (lidar_sim, scene 2000, about 116 k rows each) along a drive, fused into one map.
  save     VoxelMap.save of that map to a file in --dir (a temporary directory by default)
  load     VoxelMap.load of the file into a cleared map of the same size
  merge    VoxelMap.merge of the map into a cleared map of the same size
  grown    VoxelMap.grown(table_log2 + 1): a new, larger map and the merge into it
against two yardsticks:
  copies   for save and load: the table's raw arrays (40 or 112 bytes per ENTRY of the table, claimed or not) device -> pinned -> device with plain copies
  rebuild  for load and merge: clear + add of all the scans, which is what a process without the file would have to do (and nobody keeps the scans)
A window is one call, timed on the host from its start to the drained stream (save and load end on the host: the file), behind 2 warm-up rounds; the figure is
the median of --reps alternating windows, with their spread.  It reports only: no test depends on a time.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--table-log2", type=int, default=24)
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--shape", type=int, default=1)
    ap.add_argument("--dir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_snapshot: no GPU (this measures the MI355X path only)")
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

    ctx = api.Context(0)
    shaped = bool(a.shape)
    new = lambda log2=a.table_log2: api.VoxelMap(ctx, cell=a.cell, table_log2=log2, shape=shaped)
    src, dst = new(), new()
    src.add_device(descs, poses)
    st = src.stats()
    tmp = tempfile.TemporaryDirectory(dir=a.dir or None)
    path = os.path.join(tmp.name, "map.vxm")
    src.save(path)
    info = api.VoxelMap.snapshot_info(path)

    # the yardstick of plain copies: as many bytes as the table's arrays hold, device -> pinned -> device
    table_bytes = (1 << a.table_log2) * 8 * (14 if shaped else 5)
    d_raw = torch.zeros(table_bytes // 8, dtype=torch.int64, device=dev); h_raw = torch.zeros(table_bytes // 8, dtype=torch.int64).pin_memory()
    torch.cuda.synchronize()

    def copies_out():
        h_raw.copy_(d_raw, non_blocking=True); torch.cuda.synchronize()

    def copies_in():
        d_raw.copy_(h_raw, non_blocking=True); torch.cuda.synchronize()

    def rebuild():
        dst.clear(); dst.add_device(descs, poses); ctx.sync()

    def load():
        dst.clear(); dst.load(path); ctx.sync()

    def merge():
        dst.clear(); dst.merge(src); ctx.sync()

    def grown():
        g = src.grown(a.table_log2 + 1); ctx.sync(); g.close()

    fns = dict(save=lambda: src.save(path), load=load, merge=merge, grown=grown, copies_out=copies_out, copies_in=copies_in, rebuild=rebuild)

    def timed(fn):
        ctx.sync()
        t0 = time.perf_counter(); fn()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        for fn in fns.values():
            timed(fn)
    t = {k: [] for k in fns}
    for _ in range(a.reps):                                          # alternating
        for k, fn in fns.items():
            t[k].append(timed(fn))
    assert dst.stats() == st                                          # (the last window rebuilt it)
    result = dict(scans=a.scans, rows=rows, cell=a.cell, table_log2=a.table_log2, shaped=shaped, reps=a.reps, entries=int(info["entries"]),
                  file_bytes=int(info["file_bytes"]), table_bytes=table_bytes, cells_occupied=st["cells_occupied"],
                  ms={k: float(np.median(v)) for k, v in t.items()}, range_ms={k: [float(min(v)), float(max(v))] for k, v in t.items()})
    for k in fns:
        print("%-11s %9.3f ms  (%.3f - %.3f)" % (k, result["ms"][k], *result["range_ms"][k]), flush=True)
    for m in (src, dst):
        m.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()
    tmp.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
