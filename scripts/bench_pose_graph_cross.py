#!/usr/bin/env python3
"""The pose graph's covariance columns and gate (icet_pose_graph_covariance_columns, icet_pose_graph_gate) on the rows of
scripts/bench_pose_graph_marginals.py (GPU box):

    python scripts/bench_pose_graph_cross.py [--nodes 64,256,1024,4096] [--closures 4,32,d64] [--reps 5] [--parent-lib PATH/libicet_hip.so] [--out FILE.json]

Per graph, wall times of whole calls through the C ABI (host arrays in and out, allocation and copies included), the median of --reps rounds after one warm-up
round; within a round the calls ALTERNATE, so that a drift of the machine moves them together:
    marg_ms              icet_pose_graph_marginals of this build
    marg_parent_ms       the same call of the build at --parent-lib (a library built from the parent commit), when given
    marg_again_ms        a second marginals call of this build in the same round: how far two runs of one build lie from each other
    cols1_ms, cols8_ms, cols32_ms      icet_pose_graph_covariance_columns with T = 1, 8, 32 targets spread over the chain
    gate32_ms            icet_pose_graph_gate with 32 candidates (i, N - 1 - i) on 32 distinct live nodes
Prints one JSON line.
"""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import pose_graph_model as pgm
    import icet_amd
    from icet_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_graph_cross: no GPU (this measures the MI355X path only)")
    ctx = api.Context(0)
    lib = icet_amd.load_library()
    parent = parent_h = None
    if a.parent_lib:
        # the parent build's library beside this one: its own context, the marginals call through the same argument list
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.icet_create.argtypes = lib.icet_create.argtypes
        parent.icet_destroy.argtypes = lib.icet_destroy.argtypes
        parent.icet_pose_graph_marginals.argtypes = lib.icet_pose_graph_marginals.argtypes
        parent_h = C.c_void_p()
        assert parent.icet_create(C.byref(parent_h), 0, None) == api.ICET_OK

    def clock(call):
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3
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
            q = 6 * len(api.pose_graph_ends(n, g["closures"]))
            if q > 6 * api.PG_DIRECT_MAX_ENDS:
                rows.append(dict(n=n, closures=cs, q=q, refused="more than 128 end nodes"))
                continue
            pg = ctx._pose_graph_host(g["poses"], g["odo_X"], g["odo_info"], g["closures"], None)
            cov = np.zeros((n, 36)); res = api.PoseGraphMarginalsResult(); gres = api.PoseGraphGateResult()
            T64 = g["poses"].astype(np.float64)
            calls = {"marg_ms": lambda: lib.icet_pose_graph_marginals(*pg.args, cov.ctypes.data, C.byref(res))}
            if parent is not None:
                pargs = (parent_h,) + tuple(pg.args[1:])
                calls["marg_parent_ms"] = lambda: parent.icet_pose_graph_marginals(*pargs, cov.ctypes.data, C.byref(res))
            calls["marg_again_ms"] = calls["marg_ms"]
            for T in (1, 8, 32):
                if T >= n:
                    continue
                t = np.ascontiguousarray(np.linspace(1, n - 1, T).astype(np.int32))
                assert len(set(t.tolist())) == T
                cols = np.zeros((T, n, 36))
                calls["cols%d_ms" % T] = (lambda t=t, cols=cols, T=T: lib.icet_pose_graph_covariance_columns(*pg.args, T, t.ctypes.data, cols.ctypes.data, cov.ctypes.data, C.byref(res)))
            if n >= 66:
                gi = np.arange(1, 33, dtype=np.int32); gj = np.ascontiguousarray(n - 1 - gi, np.int32)
                cX = np.ascontiguousarray([pgm.xof(T64[i], T64[j]) for i, j in zip(gi, gj)], np.float32)
                cC = np.tile((np.diag([0.005] * 3 + [0.0005] * 3) ** 2).astype(np.float32).reshape(1, 36), (32, 1))
                d2 = np.zeros(32); S = np.zeros((32, 36)); st = np.zeros(32, np.int32)
                calls["gate32_ms"] = lambda: lib.icet_pose_graph_gate(*pg.args, 32, gi.ctypes.data, gj.ctypes.data, cX.ctypes.data, cC.ctypes.data, 0.0, d2.ctypes.data,
                                                                      S.ctypes.data, st.ctypes.data, C.byref(gres))
            for k, f in calls.items():          # the warm-up round; every call must succeed
                assert f() == api.ICET_OK, k
            t = {k: [] for k in calls}
            for _ in range(max(a.reps, 1)):
                for k, f in calls.items():
                    t[k].append(clock(f))
            row = dict(n=n, closures=cs, q=q, status=int(res.status), **{k: float(np.median(v)) for k, v in t.items()})
            if "gate32_ms" in calls:
                row["gate_rejected"] = int(gres.rejected)
            print("# " + json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
    if parent is not None:
        parent.icet_destroy(parent_h)
    ctx.close()
    line = json.dumps(dict(bench="pose_graph_cross", device=torch.cuda.get_device_name(0), parent=bool(a.parent_lib), rows=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
