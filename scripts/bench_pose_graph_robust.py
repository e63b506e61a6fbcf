#!/usr/bin/env python3
"""The pose-graph optimiser under a robust kernel (icet_pose_graph_optimize_robust, DESIGN.md section 20 "Robust kernels") beside the plain run (GPU box):

    python scripts/bench_pose_graph_robust.py [--nodes 64,256,1024] [--closures 4,32] [--reps 5] [--kernel cauchy] [--solver direct] [--out FILE.json]

Graph (N, C): the graph of scripts/bench_pose_graph.py -- tests/pose_graph_model.py make_loop(N, pairs, seed=7) with C noisy closures between random nodes at
least two apart, the first of them (0, N - 1) -- optimised from its drifted chain with the defaults.  No closure is false here: the row shows what the robust
machinery costs on the graph the plain run is measured on.  Per graph: the wall time of one Context.optimize_pose_graph call without and with the kernel (host
arrays in and out, allocation and copies included; the median of --reps calls after one warm-up), the statuses, Gauss-Newton iterations and band solves of both,
the least weight and the count of downweighted edges, and how far the two results are apart.  The robust run takes more iterations (its convergence is linear),
so the time per iteration stands beside the time per call.  Reported only: no test depends on a time.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="64,256,1024")
    ap.add_argument("--closures", default="4,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel", default="cauchy", choices=["huber", "cauchy", "geman_mcclure"])
    ap.add_argument("--solver", default="direct", choices=["cg", "direct", "auto"])
    ap.add_argument("--gn-iters", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import pose_graph_model as pgm
    from icet_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_graph_robust: no GPU (this measures the MI355X path only)")
    ctx = api.Context(0)
    rows = []
    for n in [int(v) for v in a.nodes.split(",")]:
        for c in [int(v) for v in a.closures.split(",")]:
            rs = np.random.RandomState(1000 * c + n)
            pairs = [(0, n - 1)]
            while len(pairs) < c:
                i, j = (int(v) for v in rs.randint(0, n, 2))
                if abs(i - j) >= 2:
                    pairs.append((i, j))
            g = pgm.make_loop(n, pairs, seed=7)
            row = dict(n=n, closures=c, q=6 * len(api.pose_graph_ends(n, g["closures"])))
            res = {}
            for name, kw in (("plain", {}), ("robust", dict(robust=a.kernel))):
                call = lambda: ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], solver=a.solver, gn_iters=a.gn_iters, **kw)
                call()
                t = []
                for _ in range(max(a.reps, 1)):
                    t0 = time.perf_counter(); r = call(); t.append(time.perf_counter() - t0)
                res[name] = r
                ms = float(np.median(t)) * 1e3
                row.update({name + "_ms": ms, name + "_status": r["status"], name + "_gn_iterations": r["gn_iterations"], name + "_band_solves": r["pcg_iterations"],
                            name + "_ms_per_iteration": ms / max(r["gn_iterations"], 1)})
            dt, dr = pgm.pose_error(res["robust"]["poses64"], res["plain"]["poses64"])
            row.update(solver=res["robust"]["solver"], min_weight=float(res["robust"]["edge_weight"].min()), downweighted=res["robust"]["downweighted"], diff_m=dt, diff_rad=dr)
            print("# " + json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
    ctx.close()
    line = json.dumps(dict(bench="pose_graph_robust", kernel=a.kernel, device=torch.cuda.get_device_name(0), rows=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
