#!/usr/bin/env python3
"""Coarse alignment of the keyframe store on one GPU, variants alternating in one process (GPU box):

    python scripts/bench_coarse.py [--slots 256] [--k 16] [--runlen 7] [--reps 7] [--inner 10] [--out FILE.json]

  (1) put      icet_keyframe_store_put_device of the 256 scan 1s of bench.py's pairs into a store with coarse alignment enabled against one without.
  (2) align    icet_keyframe_store_coarse_align_device alone (the queries' grids, the hypotheses, the correlation, the resolve), back to back, for Q = 1 and 8,
               K = --k, 6 hypotheses (Y = 1 with the half turn), window 12; the kernel split comes from a rocprofv3 --kernel-trace --stats run of this script.
  (3) query    Q = 1, K = --k: icet_keyframe_store_close_coarse_device (candidates by appearance) + icet_sync + the copy of the record at S = 1 and at S = 9
               (the lattice), against icet_keyframe_store_close_appearance_device at S = 9 on the same store.
A window is --inner calls ended by a device synchronise, timed on the host clock; the figure is the median over --reps windows.  Prints one JSON line.
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
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--runlen", type=int, default=7)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_coarse: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    pairs = 256
    s1, s2 = [], []
    for k in range(pairs):
        x, y, _ = lidar_sim.make_batch_pair(k, device=dev)
        s1.append(x.contiguous()); s2.append(y.contiguous())
    torch.cuda.synchronize()
    desc = lambda t: (t.data_ptr(), t.shape[1], t.shape[1])
    prm = api.Params(a.runlen, 24, 75, 25, 0.1, 0.1, 0)
    d1 = [desc(t) for t in s1]; d2 = [desc(t) for t in s2]
    ctx = api.Context(0)
    K = a.k

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            fn()
        ctx.sync()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.inner

    def measure(fns):
        for _ in range(3):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.reps):                                      # alternating
            for k, fn in fns.items():
                t[k].append(window(fn))
        return {k: float(np.median(v)) * 1e3 for k, v in t.items()}

    result = dict(slots=a.slots, k=K, runlen=a.runlen, reps=a.reps, inner=a.inner)
    # (1) the put, with and without grids
    plain = api.KeyframeStore(ctx, pairs)
    store = api.KeyframeStore(ctx, max(a.slots, pairs))
    store.enable_coarse()
    first = list(range(pairs))
    med = measure({"on": lambda: store.put_device(first, d1), "off": lambda: plain.put_device(first, d1), "off2": lambda: plain.put_device(first, d1)})
    result["put_256"] = dict(coarse_ms=med["on"], plain_ms=med["off"], plain_again_ms=med["off2"], extra_ms=med["on"] - min(med["off"], med["off2"]))
    print("(1) put of 256 scans: coarse on %.3f ms   off %.3f / %.3f ms" % (med["on"], med["off"], med["off2"]), flush=True)
    plain.close()
    store.enable_appearance()                                        # (the descriptors come with the next put)
    store.put_device(first, d1)
    ctx.sync()

    # (2) the search alone: candidates 0 .. K - 1 of every query, the scan's own partner among them
    se = api.KeyframeStore.coarse_search(12, 1, np.pi / 120, True)
    out = {}
    for Q in (1, 8):
        cand = torch.tensor([[(q + k) % pairs for k in range(K)] for q in range(Q)], dtype=torch.int32, device=dev)
        base = torch.zeros((Q, K, 6), dtype=torch.float32, device=dev)
        x0 = torch.zeros((Q, K, 6), dtype=torch.float32, device=dev)
        m = torch.zeros((Q, K, 32), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        out["q%d_ms" % Q] = measure({"s": lambda: store.coarse_align_device(d2[:Q], K, cand.data_ptr(), base.data_ptr(), se, x0.data_ptr(), m.data_ptr())})["s"]
        mm = np.frombuffer(m.cpu().numpy().tobytes(), api.COARSE_MATCH_DTYPE).reshape(Q, K)
        out["q%d_partner_found" % Q] = bool((mm["found"][:, 0] == 1).all() and (mm["score"][:, 0] >= mm["score"][:, 1:].max(1)).all())
    result["align_k%d_h6" % K] = out
    print("(2) coarse_align_device, K = %d, 6 hypotheses, window 12: %s" % (K, out), flush=True)

    # (3) the whole query: one coarse start, the lattice around it, and the lattice on the appearance yaw alone
    rec = torch.zeros((1, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    one = np.zeros((1, 6), np.float32)
    last = {}

    def coarse(S, starts, name):
        def fn():
            store.close_coarse_device(d2[:1], None, None, prm, api.ClosureQuery(float("inf"), K, 0, S, float("inf"), 0, 0), se, rec.data_ptr(), starts)
            ctx.sync()
            last[name] = np.frombuffer(rec.cpu().numpy().tobytes(), api.CLOSURE_DTYPE)
        return fn

    def by_appearance():
        store.close_appearance_device(d2[:1], None, prm, api.ClosureQuery(float("inf"), K, 0, 9, float("inf"), 0, 0), rec.data_ptr(), api.LATTICE_STARTS)
        ctx.sync()
        last["app"] = np.frombuffer(rec.cpu().numpy().tobytes(), api.CLOSURE_DTYPE)

    med = measure({"coarse_s1": coarse(1, one, "c1"), "app_s9": by_appearance, "coarse_s9": coarse(9, api.LATTICE_STARTS, "c9"), "app_s9_again": by_appearance})
    result["query_q1"] = dict(coarse_s1_ms=med["coarse_s1"], coarse_s9_ms=med["coarse_s9"], appearance_s9_ms=med["app_s9"], appearance_s9_again_ms=med["app_s9_again"],
                              winners=[int(last[n]["slot"][0]) for n in ("c1", "c9", "app")], coarse_score=int(last["c1"]["reserved1"][0][0]))
    print("(3) Q = 1, K = %d: coarse S = 1 %.3f ms   coarse S = 9 %.3f ms   by appearance S = 9 %.3f / %.3f ms" % (K, med["coarse_s1"], med["coarse_s9"], med["app_s9"],
                                                                                                          med["app_s9_again"]), flush=True)
    store.close()
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
