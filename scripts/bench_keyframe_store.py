#!/usr/bin/env python3
"""The keyframe store against the context's own keyframe path, in one process, alternating (GPU box):

    python scripts/bench_keyframe_store.py [--pairs 256] [--runlen 7] [--reps 7] [--inner 10] [--out FILE.json]

Workload: the pairs of bench.py's default batch (lidar_sim.make_batch_pair(k), k < --pairs).  Four comparisons:
  (a) put      icet_keyframe_store_put_device of the --pairs scan 1s into slots 0 .. pairs-1   vs   icet_keyframe_device of the same scans;
  (b) regs16   --pairs registrations, scan 2 of pair r against store slot r mod 16               vs   icet_register_indexed_device against the same
               16 keyframes parked in a context;
  (c) regs_far --pairs registrations against --pairs distinct slots of a 4096-slot store (~0.96 GB at 75 x 24, filled by putting the scan 1s 16 times;
               registration r reads slot 256 (r mod 16) + r, spread over the whole store: the L2-cold case), reported alone;
  (d) query    one loop-closure query -- scan 2 of pair 0 against 16 slots x 4 starts, scored, best selected on the device   vs   the same query
               rebuilding its 16 keyframes first (icet_keyframe_device + icet_register_indexed_scored_device + icet_select_best_device).
A window is --inner calls ended by a device synchronise, timed on the host clock; the figure is the median over --reps windows.
Results are checked bit for bit: (b) and (d) against the context path, (c) against icet_solve_batch_device of the same pairs.  Prints one JSON line.
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
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--runlen", type=int, default=7)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--big", type=int, default=4096, help="slots of the store of workload (c)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_keyframe_store: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    s1, s2 = [], []
    for k in range(a.pairs):
        x, y, _ = lidar_sim.make_batch_pair(k, device=dev)
        s1.append(x.contiguous()); s2.append(y.contiguous())
    torch.cuda.synchronize()
    desc = lambda t: (t.data_ptr(), t.shape[1], t.shape[1])
    prm = api.Params(a.runlen, 24, 75, 25, 0.1, 0.1, 0)
    d1 = [desc(t) for t in s1]; d2 = [desc(t) for t in s2]
    ctx_s, ctx_c = api.Context(0), api.Context(0)
    store = api.KeyframeStore(ctx_s, max(a.pairs, 16))

    def window(fn, sync):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            fn()
        sync()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.inner

    def measure(fns):
        for _ in range(3):                                          # warm-up of every call (and of the workspace sizes)
            for fn, _s in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.reps):                                      # alternating
            for k, (fn, sync) in fns.items():
                t[k].append(window(fn, sync))
        return {k: float(np.median(v)) * 1e3 for k, v in t.items()}, {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}

    result = dict(pairs=a.pairs, runlen=a.runlen, reps=a.reps, inner=a.inner)
    # (a) put vs keyframe build
    slots_a = list(range(a.pairs))
    med, spread = measure({"put": (lambda: store.put_device(slots_a, d1), ctx_s.sync), "keyframe": (lambda: ctx_c.keyframe_device(d1, prm), ctx_c.sync)})
    result["a"] = dict(put_ms=med["put"], keyframe_ms=med["keyframe"], overhead=med["put"] / med["keyframe"] - 1.0, spread=spread)
    print("(a) put %d scans %.3f ms   keyframe build %.3f ms   overhead %+.1f %%" % (a.pairs, med["put"], med["keyframe"], 100 * result["a"]["overhead"]), flush=True)
    # (b) registrations against 16 slots vs 16 parked keyframes
    kf_index = [r % 16 for r in range(a.pairs)]
    store.put_device(list(range(16)), d1[:16]); ctx_c.keyframe_device(d1[:16], prm)
    out_s = torch.zeros((a.pairs, 48), dtype=torch.float32, device=dev); out_c = torch.zeros_like(out_s)
    med, spread = measure({"store": (lambda: store.register_device(kf_index, d2, prm, out_s.data_ptr()), ctx_s.sync),
                           "parked": (lambda: ctx_c.register_indexed_device(kf_index, d2, prm, out_c.data_ptr()), ctx_c.sync)})
    same_b = bool(torch.equal(out_s, out_c)) and bool(torch.isfinite(out_s).all())
    result["b"] = dict(store_ms=med["store"], parked_ms=med["parked"], ratio=med["store"] / med["parked"], same_bits=same_b, spread=spread)
    print("(b) %d regs x 16 slots: store %.3f ms   parked %.3f ms   ratio %.3f   same bits: %s" % (a.pairs, med["store"], med["parked"], result["b"]["ratio"], same_b), flush=True)
    # (d) one loop-closure query: 16 slots x 4 starts, scored, best selected -- from the store, or rebuilding the 16 keyframes
    q_idx = [k for k in range(16) for _ in range(4)]
    x0 = np.zeros((64, 6), np.float32); x0[:, 0] = [0.0, 0.1, -0.1, 0.2] * 16
    xd = torch.from_numpy(x0).to(dev)
    qd2 = [d2[0]] * 64
    q_out = {k: torch.zeros((64, 48), dtype=torch.float32, device=dev) for k in ("s", "c")}
    q_sc = {k: torch.zeros((64, 8), dtype=torch.int32, device=dev) for k in ("s", "c")}
    q_best = {k: torch.zeros((1,), dtype=torch.int32, device=dev) for k in ("s", "c")}
    grp = np.zeros(64, np.int32)

    def query_store():
        store.register_scored_device(q_idx, qd2, prm, q_out["s"].data_ptr(), q_sc["s"].data_ptr(), xd.data_ptr())
        ctx_s.select_best_device(grp, 1, q_sc["s"].data_ptr(), q_best["s"].data_ptr())

    def query_rebuild():
        ctx_c.keyframe_device(d1[:16], prm)
        ctx_c.register_indexed_scored_device(q_idx, qd2, prm, q_out["c"].data_ptr(), q_sc["c"].data_ptr(), xd.data_ptr())
        ctx_c.select_best_device(grp, 1, q_sc["c"].data_ptr(), q_best["c"].data_ptr())

    med, spread = measure({"store": (query_store, ctx_s.sync), "rebuild": (query_rebuild, ctx_c.sync)})
    same_d = all(bool(torch.equal(d["s"], d["c"])) for d in (q_out, q_sc, q_best))
    result["d"] = dict(store_ms=med["store"], rebuild_ms=med["rebuild"], saved_ms=med["rebuild"] - med["store"], same_bits=same_d, spread=spread)
    print("(d) query 16 slots x 4 starts: store %.3f ms   rebuilding %.3f ms   same bits: %s" % (med["store"], med["rebuild"], same_d), flush=True)
    # (c) the L2-cold case: a 4096-slot store
    store.close()
    big = api.KeyframeStore(ctx_s, a.big)
    for j in range(a.big // a.pairs):
        big.put_device([a.pairs * j + k for k in range(a.pairs)], d1)
    far = [(a.pairs * (r % 16) + r) % a.big for r in range(a.pairs)]
    out_f = torch.zeros((a.pairs, 48), dtype=torch.float32, device=dev)
    med, spread = measure({"far": (lambda: big.register_device(far, d2, prm, out_f.data_ptr()), ctx_s.sync)})
    ctx_c.solve_batch_device(d1, d2, prm, out_c.data_ptr()); ctx_c.sync()
    same_c = bool(torch.equal(out_f, out_c))
    result["c"] = dict(store_slots=a.big, store_gb=a.big * (1800 * 128 + 2 * 1800 + 4) / 1e9, regs_ms=med["far"], same_bits=same_c, spread=spread)
    print("(c) %d regs x %d distinct slots of a %d-slot store: %.3f ms   same bits: %s" % (a.pairs, a.pairs, a.big, med["far"], same_c), flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    big.close(); ctx_s.close(); ctx_c.close()
    return 0 if (same_b and same_c and same_d) else 1


if __name__ == "__main__":
    sys.exit(main())
