#!/usr/bin/env python3
"""The registration against a shaped voxel map on one GPU, variants alternating in one process (GPU box):

    python scripts/bench_map_register.py [--scans 64] [--table-log2 22] [--cell 0.5] [--reps 7] [--max-iters 20] [--neighbours 1,7,27] [--out FILE.json]

The workload is bench_map.py's: --scans synthetic 64-channel scans (lidar_sim, scene 2000, about 116 k rows each) along a drive, fused at their poses into a shaped
map.  Live scans are taken at poses between the fused ones and started 0.15 m and 0.02 rad off.
  (1) register   one icet_voxel_map_register_device call of 1 / 16 / 64 live scans, max_iters as given: ms per call, ms per pass (the call enqueues 1 + max_iters
                 passes whatever the queries do), rows / s over the passes the queries actually ran, and how they ended.
  (2) score      the same scans with max_iters = 0: one row pass and one step -- the row pass's own rate.
                 --neighbours 1,7,27 runs (1) and (2) under each neighbourhood (the cells a row is scored against the best of), all of them alternating in the
                 same windows; the keys of a neighbourhood other than 1 end in _n7 / _n27.  (3) and (4) are centre-only.
  (3) gauss      the score of one scan with sigma_min changing from call to call, so that every call rebuilds the Gaussians, then the same call with them current
                 (two runs of windows, one after the other: alternating the two would make every call stale).
  (4) detour     the same localisations the way they were done before: VoxelMap.query + KeyframeStore.put_from_map (a keyframe per start pose) and
                 icet_keyframe_store_close_device of the live scans against those slots.
A window is ONE call (or pair of calls) between two HIP events on the context's stream, behind 2 warm-up rounds; the figure is the median of --reps windows, with
the smallest and the largest beside it.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--table-log2", type=int, default=22)
    ap.add_argument("--cell", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-iters", type=int, default=20)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--runlen", type=int, default=7)
    ap.add_argument("--neighbours", default="1", help="comma-separated: 1, 7, 27")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    nbs = [int(v) for v in a.neighbours.split(",")]
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_register: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    scene = lidar_sim.make_scene(2000)

    def pose(k, dx=0.0, dy=0.0, dyaw=0.0):
        t = np.array([-20.0 + 0.15 * k + dx, -1.0 + 0.01 * k + dy, 0.0]); yaw = 0.01 * k + dyaw
        T = np.eye(4); T[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]; T[:3, 3] = t
        return T

    def scan(T, seed):
        return lidar_sim.make_scan(scene, (T[:3, 3], T[:3, :3]), seed, rings=a.rings, steps=a.steps, device=dev).contiguous()

    fused = [pose(k) for k in range(a.scans)]
    scans = [scan(T, 50 + k) for k, T in enumerate(fused)]
    n_live = 64
    true = [pose((k + 0.5) * (a.scans - 1) / n_live) for k in range(n_live)]
    live = [scan(T, 5000 + k) for k, T in enumerate(true)]
    starts = np.stack([pose((k + 0.5) * (a.scans - 1) / n_live, 0.15 * (-1) ** k, 0.1, 0.02 * (-1) ** (k // 2)) for k in range(n_live)]).astype(np.float32)
    torch.cuda.synchronize()
    descs = [(s.data_ptr(), s.shape[1], s.shape[1]) for s in scans]
    ldesc = [(s.data_ptr(), s.shape[1], s.shape[1]) for s in live]

    ctx = api.Context(0)
    stream = torch.cuda.ExternalStream(api.load_library().icet_stream(ctx._h), device=dev)
    m = api.VoxelMap(ctx, cell=a.cell, table_log2=a.table_log2, shape=True)
    m.add_device(descs, np.stack(fused).astype(np.float32))
    ctx.sync()
    st = m.stats(5)
    recs = torch.zeros(n_live * api.MAP_REGISTRATION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

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

    def records(q):
        ctx.sync()
        return recs.cpu().numpy().view(api.MAP_REGISTRATION_DTYPE)[:q].copy()

    result = dict(fused_scans=a.scans, cell=a.cell, table_log2=a.table_log2, reps=a.reps, max_iters=a.max_iters, cells_occupied=st["cells_occupied"], cells_usable=st["cells_out"])
    par = api.map_register_params(max_iters=a.max_iters)
    par0 = api.map_register_params(max_iters=0)
    sizes = (1, 16, 64)
    result["neighbours"] = nbs

    # (1) and (2): the loop and the score, 1 / 16 / 64 scans, under every neighbourhood asked for, alternating
    pars = {nb: (api.map_register_params(max_iters=a.max_iters, neighbours=nb), api.map_register_params(max_iters=0, neighbours=nb)) for nb in nbs}
    tag = lambda nb: "" if nb == 1 else "_n%d" % nb
    fns = {}
    for q in sizes:
        for nb in nbs:
            fns["register_%d%s" % (q, tag(nb))] = (lambda q=q, nb=nb: m.register_device(ldesc[:q], starts[:q], recs.data_ptr(), pars[nb][0]))
            fns["score_%d%s" % (q, tag(nb))] = (lambda q=q, nb=nb: m.register_device(ldesc[:q], starts[:q], recs.data_ptr(), pars[nb][1]))
    med, spread = measure(fns)
    for q in sizes:
        rows = int(sum(s.shape[1] for s in live[:q]))
        for nb in nbs:
            kr, ks = "register_%d%s" % (q, tag(nb)), "score_%d%s" % (q, tag(nb))
            m.register_device(ldesc[:q], starts[:q], recs.data_ptr(), pars[nb][0])
            r = records(q)
            passes = int((r["iterations"] + 1).sum())
            ran = float(sum(live[k].shape[1] * (int(r["iterations"][k]) + 1) for k in range(q)))
            err = [float(np.linalg.norm(r["pose"][k].reshape(4, 4)[:3, 3] - true[k][:3, 3])) for k in range(q)]
            result[kr] = dict(ms=med[kr], range_ms=spread[kr], ms_per_pass=med[kr] / (a.max_iters + 1), rows=rows, query_passes=passes, accepted=int(r["accepted"].sum()),
                              max_query_passes=int(r["iterations"].max()) + 1, rows_per_s=ran / med[kr] * 1e3, status_counts=np.bincount(r["status"], minlength=5).tolist(),
                              rows_matched=int(r["rows_matched"].sum()), median_error_m=float(np.median(err)), max_error_m=float(max(err)))
            result[ks] = dict(ms=med[ks], range_ms=spread[ks], rows=rows, rows_per_s=rows / med[ks] * 1e3)
            print("(1) register %2d scans, %2d cells, %8d rows: %.3f ms [%.3f, %.3f]  %.3f ms / pass  %.2f G rows/s over %d query passes (%d accepted, longest %d)  status %s  "
                  "error median %.4f m max %.4f m" % (q, nb, rows, med[kr], *spread[kr], med[kr] / (a.max_iters + 1), ran / med[kr] * 1e-6, passes, result[kr]["accepted"],
                                                      result[kr]["max_query_passes"], result[kr]["status_counts"], np.median(err), max(err)), flush=True)
            print("(2) score    %2d scans, %2d cells: %.3f ms [%.3f, %.3f]  %.2f G rows/s" % (q, nb, med[ks], *spread[ks], rows / med[ks] * 1e-6), flush=True)

    # (3) the Gaussians: every call stale against every call current
    flip = dict(k=0)
    pa, pb = api.map_register_params(max_iters=0, sigma_min=0.02), api.map_register_params(max_iters=0, sigma_min=0.021)

    def stale():
        flip["k"] ^= 1
        m.register_device(ldesc[:1], starts[:1], recs.data_ptr(), pb if flip["k"] else pa)

    med, spread = measure({"stale": stale})                           # (not alternating with the next: a call with another sigma_min between them would make both stale)
    m.register_device(ldesc[:1], starts[:1], recs.data_ptr(), par0)
    med2, spread2 = measure({"current": lambda: m.register_device(ldesc[:1], starts[:1], recs.data_ptr(), par0)})
    med.update(med2); spread.update(spread2)
    result["gauss"] = dict(entries=1 << a.table_log2, stale_ms=med["stale"], stale_range_ms=spread["stale"], current_ms=med["current"], current_range_ms=spread["current"],
                           build_ms=med["stale"] - med["current"])
    print("(3) Gaussians over %d entries: a stale score %.3f ms, a current one %.3f ms: the build %.3f ms" % (1 << a.table_log2, med["stale"], med["current"], med["stale"] - med["current"]),
          flush=True)

    # (4) the detour: a keyframe per start pose out of the map, then the closure call of the live scans against those slots
    try:
        store = api.KeyframeStore(ctx, 64)
        crec = torch.zeros((n_live, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        query = api.ClosureQuery(0.05, 1, 0, 1, float("inf"), 0, 0)
        fns = {}
        for q in sizes:
            def detour(q=q):
                store.put_from_map(list(range(q)), m, starts[:q], max_range=120.0, stamps=list(range(q)))
                store.close_device(ldesc[:q], starts[:q], [1000 + k for k in range(q)], store._params(a.runlen, 0), query, crec.data_ptr())
            fns["detour_%d" % q] = detour
            fns["direct_%d" % q] = (lambda q=q: m.register_device(ldesc[:q], starts[:q], recs.data_ptr(), par))
        med, spread = measure(fns)
        for q in sizes:
            result["detour_%d" % q] = dict(ms=med["detour_%d" % q], range_ms=spread["detour_%d" % q], direct_ms=med["direct_%d" % q], direct_range_ms=spread["direct_%d" % q])
            print("(4) %2d localisations: query + put_from_map + close %.3f ms [%.3f, %.3f]   register against the map %.3f ms [%.3f, %.3f]"
                  % (q, med["detour_%d" % q], *spread["detour_%d" % q], med["direct_%d" % q], *spread["direct_%d" % q]), flush=True)
        ctx.sync()
        c = crec.cpu().numpy().view(api.CLOSURE_DTYPE).reshape(-1)
        result["detour_found"] = int((c["slot"][:64] >= 0).sum())
        store.close()
    except Exception as e:                                            # (the figures above stand without the comparison)
        result["detour_error"] = repr(e)
        print("(4) the detour did not run: %r" % (e,), flush=True)
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
