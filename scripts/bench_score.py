#!/usr/bin/env python3
"""What the registration score costs (GPU box):

    python scripts/bench_score.py [--pairs 256] [--runlen 7] [--poses 1024] [--reps 7] [--inner 10] [--out FILE.json]

(a) Scored against unscored indexed registration: the pairs of bench.py's default batch (lidar_sim.make_batch_pair(k), k < --pairs), scan 2 of pair r
    against parked keyframe r (scan 1 of pair r), from X0 = 0.  icet_register_indexed_device and icet_register_indexed_scored_device are timed in
    turn; the difference is the score's added time (one point pass at the final X plus k_gn_score).  The scored call's results are checked bit for
    bit against the unscored call's.
(b) Pose hypotheses: --poses poses of ONE 64-channel scan (scan 2 of pair 0) around its solved X against ONE keyframe (scan 1 of pair 0), scored in
    one icet_score_indexed_device call; then the best of the poses by icet_select_best_device (one group).
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
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--runlen", type=int, default=7)
    ap.add_argument("--poses", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_score: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    s1, s2 = [], []
    for k in range(a.pairs):
        x, y, _ = lidar_sim.make_batch_pair(k, device=dev)
        s1.append(x.contiguous()); s2.append(y.contiguous())
    torch.cuda.synchronize()
    desc = lambda t: (t.data_ptr(), t.shape[1], t.shape[1])
    prm = api.Params(a.runlen, 24, 75, 25, 0.1, 0.1, 0)
    ctx = api.Context(0)

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.inner

    # (a) scored vs unscored registration of the batch
    ctx.keyframe_device([desc(t) for t in s1], prm)
    kf_index = list(range(a.pairs)); d2 = [desc(t) for t in s2]
    out_u = torch.zeros((a.pairs, 48), dtype=torch.float32, device=dev); out_s = torch.zeros_like(out_u)
    sc = torch.zeros((a.pairs, 8), dtype=torch.int32, device=dev)
    plain = lambda: ctx.register_indexed_device(kf_index, d2, prm, out_u.data_ptr())
    scored = lambda: ctx.register_indexed_scored_device(kf_index, d2, prm, out_s.data_ptr(), sc.data_ptr())
    for _ in range(3):
        plain(); scored()
    torch.cuda.synchronize()
    same = bool(torch.equal(out_u, out_s)) and bool(torch.isfinite(out_u).all())
    t = {"plain": [], "scored": []}
    for _ in range(a.reps):
        t["plain"].append(window(plain)); t["scored"].append(window(scored))
    med = {k: float(np.median(v)) for k, v in t.items()}
    ra = dict(pairs=a.pairs, runlen=a.runlen, same_bits=same, plain_ms=med["plain"] * 1e3, scored_ms=med["scored"] * 1e3,
              added_ms=(med["scored"] - med["plain"]) * 1e3, added_frac=(med["scored"] - med["plain"]) / med["plain"],
              spread={k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()})
    print("(a) %d pairs, runlen %d: unscored %.3f ms  scored %.3f ms  -> +%.3f ms (%.1f %%)  same bits: %s"
          % (a.pairs, a.runlen, ra["plain_ms"], ra["scored_ms"], ra["added_ms"], 100 * ra["added_frac"], same), flush=True)

    # (b) many poses of one scan against one keyframe
    ctx.keyframe_device([desc(s1[0])], prm)
    one = torch.zeros((1, 48), dtype=torch.float32, device=dev)
    ctx.register_indexed_device([0], [desc(s2[0])], prm, one.data_ptr()); ctx.sync()
    rng = np.random.default_rng(5)
    X = np.repeat(one[:, :6].cpu().numpy(), a.poses, axis=0)
    X[1:, :3] += rng.normal(0, 0.2, (a.poses - 1, 3)).astype(np.float32); X[1:, 3:] += rng.normal(0, 0.02, (a.poses - 1, 3)).astype(np.float32)
    Xd = torch.from_numpy(X).to(dev)
    scp = torch.zeros((a.poses, 8), dtype=torch.int32, device=dev)
    best = torch.zeros(1, dtype=torch.int32, device=dev)
    kf0 = [0] * a.poses; d2p = [desc(s2[0])] * a.poses; group = np.zeros(a.poses, np.int32)
    score = lambda: ctx.score_indexed_device(kf0, d2p, prm, Xd.data_ptr(), scp.data_ptr())
    select = lambda: ctx.select_best_device(group, 1, scp.data_ptr(), best.data_ptr())
    for _ in range(3):
        score(); select()
    torch.cuda.synchronize()
    tb = {"score": [], "select": []}
    for _ in range(a.reps):
        tb["score"].append(window(score)); tb["select"].append(window(select))
    medb = {k: float(np.median(v)) for k, v in tb.items()}
    rb = dict(poses=a.poses, n2=int(s2[0].shape[1]), score_ms=medb["score"] * 1e3, poses_per_s=a.poses / medb["score"], select_ms=medb["select"] * 1e3,
              best=int(best.item()), spread={k: float((max(v) - min(v)) / np.median(v)) for k, v in tb.items()})
    print("(b) %d poses of one %d-row scan: %.3f ms per call (%.0f poses/s); best-of-group selection %.3f ms; chosen pose %d"
          % (a.poses, rb["n2"], rb["score_ms"], rb["poses_per_s"], rb["select_ms"], rb["best"]), flush=True)
    line = json.dumps(dict(a=ra, b=rb, reps=a.reps, inner=a.inner))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
