#!/usr/bin/env python3
"""The pose-graph optimiser (icet_pose_graph_optimize) at a range of sizes, against the NumPy model where that finishes (GPU box):

    python scripts/bench_pose_graph.py [--nodes 64,256,1024,4096] [--closures 4,32,128] [--reps 3] [--model-max 1024] [--solver cg|direct|auto] [--out FILE.json]

Graph (N, C): tests/pose_graph_model.py make_loop(N, pairs, seed=7) -- a 30 m loop with noisy odometry and C noisy closures between random nodes at least two
apart, the first of them (0, N - 1) -- optimised from its drifted chain with the defaults (gn_iters 10, dx_tol 1e-7).  Per graph: the wall time of one
Context.optimize_pose_graph call (host arrays in, host arrays out, allocation and copies included; the median of --reps calls after one warm-up, a single call
where one takes more than two seconds), its status, Gauss-Newton iterations and band solves, and the wall time of pose_graph_model.optimise for N <= --model-max
with the largest difference of the two results.  The split of a call into linearise, assemble, factor and CG is per kernel and comes from the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_pose_graph.py --nodes 1024 --closures 32 --reps 1 --model-max 0

(k_pg_linearise | k_pg_assemble + k_pg_offband | k_pg_factor | k_pg_precond + k_pg_hp + k_pg_step; k_pg_chi, k_pg_retract, k_pg_stats are the accept step).
--solver: the linear solve (option "pg_solver"): cg (the default), direct (the kernels k_pg_z, k_pg_wm, k_pg_chol, k_pg_sl, k_pg_ks, k_pg_band,
k_pg_cap_solve, k_pg_zw, k_pg_resid; a graph with more than 128 end nodes is refused and its row says so) or auto.  A row carries the solver that ran and
q = 6 x the graph's end nodes.
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
    ap.add_argument("--nodes", default="64,256,1024,4096")
    ap.add_argument("--closures", default="4,32,128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model-max", type=int, default=1024, help="largest N the NumPy model is timed at (0: never)")
    ap.add_argument("--solver", default="cg", choices=["cg", "direct", "auto"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import pose_graph_model as pgm
    from icet_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_graph: no GPU (this measures the MI355X path only)")
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
            call = lambda: ctx.optimize_pose_graph(g["poses"], g["odo_X"], g["odo_info"], g["closures"], solver=a.solver)
            q = 6 * len(api.pose_graph_ends(n, g["closures"]))
            try:
                call()
            except api.IcetError as e:
                if e.status != api.ICET_ERR_UNSUPPORTED:
                    raise
                rows.append(dict(n=n, closures=c, q=q, refused=str(e)))
                print("# " + json.dumps(rows[-1]), file=sys.stderr, flush=True)
                continue
            t = []
            for _ in range(max(a.reps, 1)):
                t0 = time.perf_counter(); r = call(); t.append(time.perf_counter() - t0)
                if t[-1] > 2.0:
                    break
            row = dict(n=n, closures=c, q=q, solver=r["solver"], ms=float(np.median(t)) * 1e3, calls=len(t), status=r["status"], gn_iterations=r["gn_iterations"], band_solves=r["pcg_iterations"],
                       chi2_initial=r["chi2_initial"], chi2_final=r["chi2_final"])
            if n <= a.model_max:
                t0 = time.perf_counter(); m = pgm.optimise(g["poses"], g["odo_X"], g["odo_info"], g["closures"]); row["model_ms"] = (time.perf_counter() - t0) * 1e3
                dt, dr = pgm.pose_error(r["poses64"], m["poses64"])
                row.update(model_status=m["status"], model_gn_iterations=m["gn_iterations"], model_chi2_final=m["chi2_final"], diff_m=dt, diff_rad=dr)
            print("# " + json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
    ctx.close()
    line = json.dumps(dict(bench="pose_graph", device=torch.cuda.get_device_name(0), rows=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
