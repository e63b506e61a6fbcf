#!/usr/bin/env python3
"""Loop closure by appearance on one GPU, variants alternating in one process (GPU box):

    python scripts/bench_appearance.py [--slots 4096] [--k 16] [--runlen 7] [--reps 7] [--inner 10] [--big 262144] [--out FILE.json]

  (1) put      icet_keyframe_store_put_device of the 256 scan 1s of bench.py's pairs into a store with appearance enabled against one without.
  (2) search   icet_keyframe_store_candidates_appearance_device alone (the queries' descriptors, the match, the selection), back to back, for Q = 1 and 8 at
               --slots slots (75 x 24 store) and at --big slots (7 x 3 store); the kernel split comes from a rocprofv3 --kernel-trace --stats run of this script.
  (3) query    Q = 1, K = --k, S = 9 (the lattice): icet_keyframe_store_close_appearance_device + icet_sync + the copy of the record, against
               icet_keyframe_store_close_device with the same counts (poses on a 3 m grid, a radius that admits K slots).
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
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--runlen", type=int, default=7)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--big", type=int, default=262144, help="slots of the 7 x 3 store of workload (2); 0 skips it")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_appearance: no GPU (this measures the MI355X path only)")
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
    K, S = a.k, 9

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

    result = dict(slots=a.slots, k=K, starts=S, runlen=a.runlen, reps=a.reps, inner=a.inner)
    # (1) the put, with and without descriptors
    plain = api.KeyframeStore(ctx, pairs)
    store = api.KeyframeStore(ctx, a.slots)
    store.enable_appearance()
    first = list(range(pairs))
    med = measure({"on": lambda: store.put_device(first, d1), "off": lambda: plain.put_device(first, d1), "off2": lambda: plain.put_device(first, d1)})
    result["put_256"] = dict(appearance_ms=med["on"], plain_ms=med["off"], plain_again_ms=med["off2"], extra_ms=med["on"] - min(med["off"], med["off2"]))
    print("(1) put of 256 scans: appearance on %.3f ms   off %.3f / %.3f ms" % (med["on"], med["off"], med["off2"]), flush=True)
    plain.close()

    def fill(st, n_slots, side):
        for lo in range(0, n_slots, pairs):
            st.put_device(list(range(lo, lo + pairs)), d1)
        j = np.arange(n_slots)
        T = np.tile(np.eye(4, dtype=np.float32), (n_slots, 1, 1))
        T[:, 0, 3] = 3.0 * (j % side); T[:, 1, 3] = 3.0 * (j // side)
        st.set_pose(j, T, j.astype(np.int64))
        ctx.sync()
        return T

    side = int(np.ceil(np.sqrt(a.slots)))
    T_host = fill(store, a.slots, side)

    # (2) the search alone
    def search_time(st):
        cand = torch.zeros((8, K), dtype=torch.int32, device=dev)
        out = {}
        for Q in (1, 8):
            q = api.ClosureQuery(float("inf"), K, 0, 1, float("inf"), 0, 0)
            out["q%d_ms" % Q] = measure({"s": lambda: st.candidates_appearance_device(d2[:Q], None, q, cand.data_ptr())})["s"]
        return out
    result["search_%d" % a.slots] = search_time(store)
    print("(2) search over %d slots: %s" % (a.slots, result["search_%d" % a.slots]), flush=True)

    # (3) the whole query against the pose query with the same counts
    home = (side // 2) * side // pairs * pairs
    Tq = T_host[home:home + 1].copy()
    sq = np.full(1, 10 ** 6, np.int64)
    radius = 3.0 * np.sqrt(K / np.pi) * 1.15
    rec = torch.zeros((1, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    last = {}

    def by_appearance():
        store.close_appearance_device(d2[:1], None, prm, api.ClosureQuery(float("inf"), K, 0, S, float("inf"), 0, 0), rec.data_ptr(), api.LATTICE_STARTS)
        ctx.sync()
        last["app"] = np.frombuffer(rec.cpu().numpy().tobytes(), api.CLOSURE_DTYPE)

    def by_pose():
        store.close_device(d2[:1], Tq, sq, prm, api.ClosureQuery(float(radius), K, 0, S, float("inf"), 0, 0), rec.data_ptr(), api.LATTICE_STARTS)
        ctx.sync()
        last["pose"] = np.frombuffer(rec.cpu().numpy().tobytes(), api.CLOSURE_DTYPE)

    med = measure({"app": by_appearance, "pose": by_pose, "pose2": by_pose})
    result["query_q1"] = dict(appearance_ms=med["app"], pose_ms=med["pose"], pose_again_ms=med["pose2"], n_candidates=[int(last["app"]["n_candidates"][0]), int(last["pose"]["n_candidates"][0])],
                              winner_holds_the_scans_partner=bool(int(last["app"]["slot"][0]) % pairs == 0))
    print("(3) Q = 1, K = %d, S = %d: by appearance %.3f ms   by pose %.3f / %.3f ms" % (K, S, med["app"], med["pose"], med["pose2"]), flush=True)
    store.close()
    if a.big > 0:
        big = api.KeyframeStore(ctx, a.big, num_bins_phi=3, num_bins_theta=7)
        big.enable_appearance()
        for lo in range(0, a.big, pairs):
            big.put_device(list(range(lo, lo + pairs)), d1)
        ctx.sync()
        result["search_%d" % a.big] = search_time(big)
        print("(2) search over %d slots (7 x 3 store): %s" % (a.big, result["search_%d" % a.big]), flush=True)
        big.close()
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
