#!/usr/bin/env python3
"""The voxel map on one GPU, variants alternating in one process (GPU box):

    python scripts/bench_map.py [--scans 256] [--table-log2 24] [--cell 0.1] [--reps 7] [--out FILE.json]

The workload: --scans synthetic 64-channel scans (lidar_sim, scene 2000, about 116 k rows each) along a drive, every one at its own pose.
  (1) add      one icet_voxel_map_add_device call of all scans into a cleared map, option "map_lds" 1 against 0: ms per call and rows / s.  With it the floor
               the design names: 12 bytes read per row + one 32-byte group of atomics per distinct (block, cell), at the 8 TB/s of the HBM's specification,
               and the measured fraction of it.  The distinct (block, cell) pairs are counted here with torch, in the kernel's blocks of 2048 rows.
  (2) extract  icet_voxel_map_extract_device of the resulting map (count pass, select, sort, centroids) into a caller's buffer.
  (3) re-pose  remove + add of 32 scans (a closure moved their poses) against clear + add of all scans.
A window is ONE call (or pair of calls) between two HIP events on the context's stream, behind 2 warm-up rounds; the figure is the median of --reps windows.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS_PER_BLOCK = 2048                                                 # kRowsPerBlock of icet_map.hip
HBM_PEAK = 8.0e12


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
        raise SystemExit("bench_map: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    scene = lidar_sim.make_scene(2000)
    scans, poses = [], []
    for k in range(a.scans):
        t = np.array([-20.0 + 0.15 * k, -1.0 + 0.01 * k, 0.0]); yaw = 0.01 * k
        T = np.eye(4); T[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]; T[:3, 3] = t
        scans.append(lidar_sim.make_scan(scene, (t, T[:3, :3]), 50 + k, rings=a.rings, steps=a.steps, device=dev).contiguous())
        poses.append(T.astype(np.float32))
    poses = np.stack(poses)
    moved = poses.copy(); moved[-32:, 0, 3] += 0.05                   # what a closure does to the last 32 poses
    torch.cuda.synchronize()
    descs = [(s.data_ptr(), s.shape[1], s.shape[1]) for s in scans]
    rows = int(sum(s.shape[1] for s in scans))

    # the distinct (block, cell) pairs of the call, for the floor (float64 on the device: within a rounding of the rule, which is all a count needs)
    pairs = 0
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
    m = api.VoxelMap(ctx, cell=a.cell, table_log2=a.table_log2)

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

    result = dict(scans=a.scans, rows=rows, cell=a.cell, table_log2=a.table_log2, reps=a.reps, block_cell_pairs=pairs)

    # (1) the add, both forms
    def add(lds):
        def fn():
            ctx.set_option("map_lds", lds)
            m.add_device(descs, poses)
        return fn
    med, spread = measure({"lds1": add(1), "lds0": add(0)}, before=m.clear)
    floor_ms = (12.0 * rows + 32.0 * pairs) / HBM_PEAK * 1e3
    st = m.stats()
    result["add"] = dict(lds1_ms=med["lds1"], lds0_ms=med["lds0"], lds1_range_ms=spread["lds1"], lds0_range_ms=spread["lds0"],
                         lds1_rows_per_s=rows / med["lds1"] * 1e3, lds0_rows_per_s=rows / med["lds0"] * 1e3, floor_ms=floor_ms,
                         lds1_fraction_of_floor=floor_ms / med["lds1"], lds0_fraction_of_floor=floor_ms / med["lds0"], stats=st)
    print("(1) add of %d scans, %d rows, %d cells, %d (block, cell) pairs: map_lds 1 %.3f ms (%.2f G rows/s)   map_lds 0 %.3f ms (%.2f G rows/s)   floor %.3f ms"
          % (a.scans, rows, st["cells_occupied"], pairs, med["lds1"], rows / med["lds1"] * 1e-6, med["lds0"], rows / med["lds0"] * 1e-6, floor_ms), flush=True)
    faster = 1 if med["lds1"] <= med["lds0"] else 0
    ctx.set_option("map_lds", faster)

    # (2) the extract, at that cell count
    n = st["cells_out"]
    xyz = torch.zeros((3, n), dtype=torch.float32, device=dev); cnt = torch.zeros(n, dtype=torch.int64, device=dev); key = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    med, spread = measure({"extract": lambda: m.extract_device(xyz.data_ptr(), n, n, 1, cnt.data_ptr(), key.data_ptr())})
    result["extract"] = dict(cells=n, ms=med["extract"], range_ms=spread["extract"])
    print("(2) extract of %d cells: %.3f ms" % (n, med["extract"]), flush=True)

    # (3) a closure moved 32 poses: remove + add of those scans against a rebuild
    state = dict(at=poses)

    def repose():
        new = moved if state["at"] is poses else poses
        m.remove_device(descs[-32:], state["at"][-32:]); m.add_device(descs[-32:], new[-32:])
        state["at"] = new

    def rebuild():
        m.clear(); m.add_device(descs, state["at"])

    med, spread = measure({"repose": repose, "rebuild": rebuild})
    result["repose_32"] = dict(map_lds=faster, remove_add_ms=med["repose"], clear_add_all_ms=med["rebuild"], remove_add_range_ms=spread["repose"], clear_add_all_range_ms=spread["rebuild"])
    print("(3) remove + add of 32 scans %.3f ms   clear + add of all %d %.3f ms   (map_lds %d)" % (med["repose"], a.scans, med["rebuild"], faster), flush=True)
    m.close()
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
