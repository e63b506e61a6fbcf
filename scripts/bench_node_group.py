#!/usr/bin/env python3
"""Node groups against nodes pushed in turn (GPU box):

    python scripts/bench_node_group.py [--streams 1,4,8,16,32,64] [--presets odometry,mapmaker] [--frames 6] [--calls 30] [--out FILE.json]

Workload: S synthetic 64-channel drives (lidar_sim.make_sequence, rings 64 x 2048 steps, a scene of its own per stream), --frames frames each, resident
in HBM.  For every preset and S:
  group   one icet_node_group of S streams; a call carries one frame of every stream (icet_node_group_push_device);
  nodes   S icet_nodes with the same parameters, pushed in turn from this thread (icet_node_push_device), one frame each per round.
Both get a warm-up of --frames rounds, then --calls timed rounds (host clock; every call returns with its results on the host).  Reported: aggregate
frames/s (S x rounds / wall), the median wall time of one round (= the group's per-call latency), and the ratio group / nodes.  The first timed round's
results of both are compared bit for bit.  Prints one JSON line per (preset, S) and a table.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,4,8,16,32,64")
    ap.add_argument("--presets", default="odometry,mapmaker")
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--no-nodes", action="store_true", help="time the groups only")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_node_group: no GPU (this measures the MI355X path only)")
    Ss = [int(x) for x in a.streams.split(",")]
    motion = (0.25, 0.02, 0.005, 0.001, -0.001, 0.006)
    drives = []
    for s in range(max(Ss)):
        drives.append([t.to("cuda:0").contiguous() for t in lidar_sim.make_sequence(a.frames, scene_seed=3000 + 11 * s, noise_seed=5000 + 11 * s, motion=motion,
                                                                                     rings=a.rings, steps=a.steps)])
    torch.cuda.synchronize()
    presets = dict(odometry=api.ODOMETRY_NODE, mapmaker=api.MAP_MAKER_NODE)
    ctx = api.Context(0)
    lines = []

    def frame(s, k):
        t = drives[s][k % a.frames]
        return (s, t.data_ptr(), t.shape[1], t.shape[1])

    for pname in a.presets.split(","):
        kw = presets[pname]
        for S in Ss:
            rec = dict(preset=pname, streams=S, calls=a.calls, rows_per_frame=int(np.mean([drives[s][0].shape[1] for s in range(S)])))
            g = api.NodeGroup(ctx, S, **kw)
            for k in range(a.frames):
                g.push_device([frame(s, k) for s in range(S)])
            first_g = g.push_device([frame(s, a.frames) for s in range(S)])
            lat = []
            t0 = time.perf_counter()
            for c in range(a.calls):
                t1 = time.perf_counter()
                g.push_device([frame(s, a.frames + 1 + c) for s in range(S)])
                lat.append(time.perf_counter() - t1)
            wall = time.perf_counter() - t0
            rec.update(group_frames_per_s=S * a.calls / wall, group_call_ms=1e3 * float(np.median(lat)))
            g.close()
            if not a.no_nodes:
                nodes = [api.Node(ctx, **kw) for _ in range(S)]
                for k in range(a.frames):
                    for s in range(S):
                        nodes[s].push_device(*frame(s, k)[1:])
                first_n = [nodes[s].push_device(*frame(s, a.frames)[1:]) for s in range(S)]
                lat = []
                t0 = time.perf_counter()
                for c in range(a.calls):
                    t1 = time.perf_counter()
                    for s in range(S):
                        nodes[s].push_device(*frame(s, a.frames + 1 + c)[1:])
                    lat.append(time.perf_counter() - t1)
                wall = time.perf_counter() - t0
                rec.update(nodes_frames_per_s=S * a.calls / wall, nodes_round_ms=1e3 * float(np.median(lat)))
                rec["speedup"] = rec["group_frames_per_s"] / rec["nodes_frames_per_s"]
                rec["same_bits"] = all(np.array_equal(x["X"].view(np.uint32), y["X"].view(np.uint32)) and np.array_equal(x["pose"].view(np.uint32), y["pose"].view(np.uint32))
                                       for x, y in zip(first_g, first_n))
                for nd in nodes:
                    nd.close()
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    ctx.close()
    print("\n| preset | S | group frames/s | group ms/call | nodes frames/s | nodes ms/round | group / nodes |")
    print("|---|---|---|---|---|---|---|")
    for r in lines:
        print("| %s | %d | %.0f | %.3f | %s | %s | %s |" % (r["preset"], r["streams"], r["group_frames_per_s"], r["group_call_ms"],
                                                           "%.0f" % r["nodes_frames_per_s"] if "nodes_frames_per_s" in r else "-",
                                                           "%.3f" % r["nodes_round_ms"] if "nodes_round_ms" in r else "-",
                                                           "%.2fx" % r["speedup"] if "speedup" in r else "-"))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
