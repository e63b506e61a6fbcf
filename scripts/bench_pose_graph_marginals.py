#!/usr/bin/env python3
"""The pose graph's marginal covariances (icet_pose_graph_marginals) at a range of sizes (GPU box):

    python scripts/bench_pose_graph_marginals.py [--nodes 64,256,1024,4096] [--closures 4,32,d64] [--reps 3] [--inv-max 1024] [--out FILE.json]

Graph (N, C): scripts/bench_pose_graph.py's -- make_loop(N, pairs, seed=7) with C closures between random nodes, the first of them (0, N - 1); "d64" is 64
DISJOINT closures (1 + k, N / 2 + 1 + k): 128 end nodes, q = 768, the limit (N >= 256).  Per graph, wall times of whole calls (host arrays in and out,
allocation and copies included; the median of --reps calls after one warm-up, a single call where one takes more than two seconds):
    ms            one Context.pose_graph_marginals call at the graph's drifted chain
    direct_ms     one iteration of the direct optimiser on the same graph (optimize_pose_graph, gn_iters = 1, solver "direct")
    inv_ms        numpy.linalg.inv of the dense H (from the hook's D, B, A) for N <= --inv-max, and the scaled difference of the two results
The per-kernel split comes from the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_pose_graph_marginals.py --nodes 1024 --closures d64 --reps 1 --inv-max 0

(k_pg_selinv_prep | k_pg_selinv | k_pg_marg_lt | k_pg_marg, behind the linearisation, k_pg_factor and the direct solve's k_pg_z, k_pg_wm, k_pg_chol, k_pg_sl, k_pg_ks).
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
    ap.add_argument("--closures", default="4,32,d64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inv-max", type=int, default=1024, help="largest N the dense inverse is timed at (0: never)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import pose_graph_model as pgm
    from icet_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_graph_marginals: no GPU (this measures the MI355X path only)")
    ctx = api.Context(0)

    def timed(call):
        call()
        t = []
        for _ in range(max(a.reps, 1)):
            t0 = time.perf_counter(); r = call(); t.append(time.perf_counter() - t0)
            if t[-1] > 2.0:
                break
        return float(np.median(t)) * 1e3, len(t), r
    rows = []
    for n in [int(v) for v in a.nodes.split(",")]:
        for cs in a.closures.split(","):
            if cs.startswith("d"):
                c = int(cs[1:])
                if n // 2 < c + 1:
                    continue
                pairs = [(1 + k, n // 2 + 1 + k) for k in range(c)]
            else:
                c = int(cs)
                rs = np.random.RandomState(1000 * c + n)
                pairs = [(0, n - 1)]
                while len(pairs) < c:
                    i, j = (int(v) for v in rs.randint(0, n, 2))
                    if abs(i - j) >= 2:
                        pairs.append((i, j))
            g = pgm.make_loop(n, pairs, seed=7)
            args = (g["poses"], g["odo_X"], g["odo_info"], g["closures"])
            q = 6 * len(api.pose_graph_ends(n, g["closures"]))
            if q > 6 * api.PG_DIRECT_MAX_ENDS:
                rows.append(dict(n=n, closures=cs, q=q, refused="more than 128 end nodes"))
                continue
            ms, calls, r = timed(lambda: ctx.pose_graph_marginals(*args))
            dms, _, w = timed(lambda: ctx.optimize_pose_graph(*args, gn_iters=1, solver="direct"))
            sd = api.pose_stds(r["cov"])
            row = dict(n=n, closures=cs, q=q, ms=ms, calls=calls, status=r["status"], direct_ms=dms, direct_band_solves=w["pcg_iterations"],
                       std_t_last=float(sd[-1, :3].max()), std_r_last=float(sd[-1, 3:].max()))
            if n <= a.inv_max:
                h = ctx.debug_pose_graph_marginals(*args)
                fx = pgm.fixed_mask(n)
                H = pgm.dense_from_band(h["D"], h["B"], h["A"], pgm.edge_list(n, g["closures"]), fx)
                t0 = time.perf_counter(); S = np.linalg.inv(H); row["inv_ms"] = (time.perf_counter() - t0) * 1e3
                R = np.stack([S[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(n - 1)])
                d = np.sqrt(np.einsum("kaa->ka", R))
                row["scaled_diff"] = float((np.abs(h["cov"][1:] - R) / (d[:, :, None] * d[:, None, :])).max())
            print("# " + json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
    ctx.close()
    line = json.dumps(dict(bench="pose_graph_marginals", device=torch.cuda.get_device_name(0), rows=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
