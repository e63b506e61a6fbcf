#!/usr/bin/env python3
"""The voxel map's visibility evidence on one GPU, variants alternating in one process (GPU box):

    python scripts/bench_map_evidence.py [--scans 256] [--table-log2 24] [--cell 0.1] [--reps 7] [--range 40] [--out FILE.json]

The map: the --scans synthetic 64-channel scans of scripts/bench_map.py (lidar_sim, scene 2000) along a drive, each at its own pose, about 634 k cells.
  (1) evidence    one icet_voxel_map_evidence_device call of all scans at image_log2 7, 8 and 9 (W 128, 256, 512), option "map_evidence_prune" 1 against 0.
                  The same call on an EMPTY map of the same cell size runs the fills, k_map_image and k_map_image_near alone: the "images" part; the "test" part
                  (k_map_evidence and the decision) is the pruned call minus that.  Beside the test: its traffic floor, index bytes in (8 count + 12 centroid: the keys are
                  read twice per block only) plus 8 B per cell out, per batch, and the fraction of 6.3 TB/s that floor would need.
  (2) query       a world query of every cell with and without ICET_VOXEL_MAP_QUERY_STATIC, behind the evidence of (1) at image_log2 8.
A window is ONE call between two HIP events on the context's stream, behind 2 warm-up rounds; the figure is the median of --reps windows.  Prints one JSON line.
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
    ap.add_argument("--range", type=float, default=40.0)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_evidence: no GPU (this measures the MI355X path only)")
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
    rows = sum(s.shape[1] for s in scans)

    ctx = api.Context(0)
    stream = torch.cuda.ExternalStream(api.load_library().icet_stream(ctx._h), device=dev)
    m = api.VoxelMap(ctx, cell=a.cell, table_log2=a.table_log2)
    m.add_device(descs, poses)
    cells = m.index()["cells_out"]
    empty = api.VoxelMap(ctx, cell=a.cell, table_log2=10)
    empty.index()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(fns):
        for _ in range(2):
            for fn in fns.values():
                timed(fn)
        t = {k: [] for k in fns}
        for _ in range(a.reps):                                      # alternating
            for k, fn in fns.items():
                t[k].append(timed(fn))
        return {k: float(np.median(v)) for k, v in t.items()}, {k: [float(min(v)), float(max(v))] for k, v in t.items()}

    result = dict(scans=a.scans, rows=rows, cells=cells, cell=a.cell, table_log2=a.table_log2, reps=a.reps, max_range=a.range)
    # (1) the evidence
    fns = {}
    for log2 in (7, 8, 9):
        kw = dict(max_range=a.range, image_log2=log2, stats=False)
        for prune in (1, 0):
            def fn(kw=kw, prune=prune):
                ctx.set_option("map_evidence_prune", prune)
                m.evidence_device(descs, poses, **kw)
            fns["w%d_prune%d" % (1 << log2, prune)] = fn
        fns["w%d_images" % (1 << log2)] = lambda kw=kw: empty.evidence_device(descs, poses, **kw)
    med, spread = measure(fns)
    ctx.set_option("map_evidence_prune", 1)
    result["evidence"] = {k: dict(ms=med[k], range_ms=spread[k]) for k in fns}
    for log2 in (7, 8, 9):
        w = 1 << log2
        batch = max(1, min(256, (64 << 20) // (8 * w * w)))
        batches = (a.scans + batch - 1) // batch
        floor_bytes = batches * cells * (20 + 8)
        test_ms = med["w%d_prune1" % w] - med["w%d_images" % w]
        st = m.evidence_device(descs, poses, max_range=a.range, image_log2=log2)
        result["w%d" % w] = dict(batches=batches, test_ms=test_ms, floor_bytes=floor_bytes, floor_ms_at_6p3_TBps=floor_bytes / 6.3e9, stats=st)
        print("(1) W %d: evidence %.3f ms pruned, %.3f ms not pruned; images %.3f ms, test %.3f ms; %d batches, floor %.1f MB = %.4f ms at 6.3 TB/s; transient %d of %d cells"
              % (w, med["w%d_prune1" % w], med["w%d_prune0" % w], med["w%d_images" % w], test_ms, batches, floor_bytes / 1e6, floor_bytes / 6.3e9, st["cells_transient"], cells), flush=True)

    # (2) a world query of everything, with and without STATIC
    m.evidence_device(descs, poses, max_range=a.range, image_log2=8)
    T = np.eye(4, dtype=np.float32)[None].copy(); T[0, :3, 3] = (1e4, 0, 0)      # no centroid lies there: every cell is kept
    w = torch.zeros((3, 1), dtype=torch.int32, device=dev)
    x = torch.zeros((3, cells), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    outs = [(x.data_ptr(), cells, cells)]
    med, spread = measure({"all": lambda: m.query_device(T, outs, w[0].data_ptr(), world=True, d_total_ptr=w[1].data_ptr()),
                           "static": lambda: m.query_device(T, outs, w[0].data_ptr(), world=True, d_total_ptr=w[1].data_ptr(), static=True)})
    ctx.sync()
    result["query"] = {k: dict(ms=med[k], range_ms=spread[k]) for k in med}
    result["query_static_rows"] = int(w[0, 0])
    print("(2) world query of %d cells: %.3f ms; with STATIC %.3f ms (%d rows)" % (cells, med["all"], med["static"], int(w[0, 0])), flush=True)
    m.close(); empty.close()
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
