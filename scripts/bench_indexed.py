#!/usr/bin/env python3
"""Indexed registration against the expanded batch, in one process, alternating (GPU box):

    python scripts/bench_indexed.py [--pairs 256] [--runlen 7] [--reps 7] [--inner 10] [--out FILE.json]

Workload: the pairs of bench.py's default batch (lidar_sim.make_batch_pair(k), k < --pairs).  Two mappings:
  (a) every scan 2 against ONE keyframe (scan 1 of pair 0);
  (b) scan 2 of pair r against keyframe r mod 16 (scan 1 of pairs 0..15).
For each, three things are timed, in turn, after a warm-up of every call:
  expanded   icet_solve_batch_device on the expanded pairs (scan1[kf_index[r]], scan2[r]) -- a keyframe build per pair;
  indexed    icet_register_indexed_device against the keyframes parked beforehand -- the registrations alone;
  keyframe   icet_keyframe_device of the distinct keyframes -- what the indexed path pays once per keyframe.
A window is --inner calls ended by a device synchronise, timed on the host clock; the figure is the median over --reps windows.
The indexed results are checked bit for bit against the expanded batch's.  Prints one JSON line.
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
    ap.add_argument("--kf", type=int, default=16, help="keyframes of mapping (b)")
    ap.add_argument("--runlen", type=int, default=7)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_indexed: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    s1, s2 = [], []
    for k in range(a.pairs):
        x, y, _ = lidar_sim.make_batch_pair(k, device=dev)
        s1.append(x.contiguous()); s2.append(y.contiguous())
    torch.cuda.synchronize()
    desc = lambda t: (t.data_ptr(), t.shape[1], t.shape[1])
    prm = api.Params(a.runlen, 24, 75, 25, 0.1, 0.1, 0)
    d2 = [desc(t) for t in s2]
    ctx_e, ctx_i = api.Context(0), api.Context(0)
    result = dict(pairs=a.pairs, runlen=a.runlen, reps=a.reps, inner=a.inner)
    for tag, n_kf in (("a", 1), ("b", a.kf)):
        kf_index = [r % n_kf for r in range(a.pairs)]
        dk = [desc(s1[k]) for k in range(n_kf)]
        d1x = [dk[k] for k in kf_index]
        out_e = torch.zeros((a.pairs, 48), dtype=torch.float32, device=dev)
        out_i = torch.zeros_like(out_e)

        def expanded():
            ctx_e.solve_batch_device(d1x, d2, prm, out_e.data_ptr())

        def indexed():
            ctx_i.register_indexed_device(kf_index, d2, prm, out_i.data_ptr())

        def keyframe():
            ctx_i.keyframe_device(dk, prm)

        def window(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.inner):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.inner

        keyframe()
        for _ in range(3):                                          # warm-up of every call (and of the workspace sizes)
            expanded(); indexed(); keyframe()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_e, out_i)) and bool(torch.isfinite(out_e).all())
        t = {"expanded": [], "indexed": [], "keyframe": []}
        for _ in range(a.reps):                                      # alternating: expanded, indexed, keyframe
            t["expanded"].append(window(expanded))
            t["indexed"].append(window(indexed))
            t["keyframe"].append(window(keyframe))
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}
        r = dict(n_kf=n_kf, same_bits=same,
                 expanded_ms=med["expanded"] * 1e3, indexed_ms=med["indexed"] * 1e3, keyframe_ms=med["keyframe"] * 1e3,
                 expanded_regs_per_s=a.pairs / med["expanded"], indexed_regs_per_s=a.pairs / med["indexed"],
                 indexed_with_keyframe_regs_per_s=a.pairs / (med["indexed"] + med["keyframe"]),
                 speedup=med["expanded"] / med["indexed"], speedup_with_keyframe=med["expanded"] / (med["indexed"] + med["keyframe"]),
                 spread=spread)
        result[tag] = r
        print("(%s) %3d keyframe(s): expanded %.3f ms  indexed %.3f ms (+ keyframe build %.3f ms)  -> %.2fx (%.2fx with the build)  same bits: %s"
              % (tag, n_kf, r["expanded_ms"], r["indexed_ms"], r["keyframe_ms"], r["speedup"], r["speedup_with_keyframe"], same), flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx_e.close(); ctx_i.close()
    ok = result["a"]["same_bits"] and result["b"]["same_bits"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
