#!/usr/bin/env python3
"""The loop-closure query of the keyframe store against the path it replaces, in one process, alternating (GPU box):

    python scripts/bench_loop_closure.py [--slots 4096] [--k 16] [--starts 4] [--runlen 7] [--reps 7] [--inner 10] [--big 262144] [--out FILE.json]

The store holds --slots keyframes at 75 x 24 (the scan 1s of bench.py's 256 pairs, put repeatedly) with poses on a 3 m grid; query q is scan 2 of pair q
at the pose of a slot that holds its scan 1, moved by the pair's motion.
  (1) query    Q = 1 and Q = 8, K = --k, S = --starts:
               (a) icet_keyframe_store_close_device + icet_sync + the copy of the Q records
               (b) the manual path on the older entries: NumPy search over host poses, host start poses, upload, icet_keyframe_store_register_scored_device,
                   icet_select_best_device, icet_sync, the copy of the winner's row and score.  Measured twice (b, b2): their difference is the A/A spread.
  (2) search   the search passes alone (icet_keyframe_store_candidates_device without start poses), back to back, at --slots and on a 7 x 3 store of --big
               slots; bytes per second over 16 B x capacity.
  (3) padding  Q = 1, K = --k with --k eligible slots, with 2 eligible slots, and a K = 2 query.
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
    ap.add_argument("--starts", type=int, default=4)
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
        raise SystemExit("bench_loop_closure: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    pairs = 256
    s1, s2, motion = [], [], []
    for k in range(pairs):
        x, y, m = lidar_sim.make_batch_pair(k, device=dev)
        s1.append(x.contiguous()); s2.append(y.contiguous()); motion.append(m)
    torch.cuda.synchronize()
    desc = lambda t: (t.data_ptr(), t.shape[1], t.shape[1])
    prm = api.Params(a.runlen, 24, 75, 25, 0.1, 0.1, 0)
    d1 = [desc(t) for t in s1]; d2 = [desc(t) for t in s2]
    ctx = api.Context(0)
    K, S = a.k, a.starts

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

    def fill(store, n_slots, side):
        """Scan 1 of pair j % 256 into slot j; poses on a `side` x `side` grid of 3 m, yaw by slot."""
        for first in range(0, n_slots, pairs):
            store.put_device(list(range(first, first + pairs)), d1)
        j = np.arange(n_slots)
        T = np.tile(np.eye(4, dtype=np.float32), (n_slots, 1, 1))
        yaw = 0.001 * (j % 1000)
        T[:, 0, 0] = np.cos(yaw); T[:, 0, 1] = -np.sin(yaw); T[:, 1, 0] = np.sin(yaw); T[:, 1, 1] = np.cos(yaw)
        T[:, 0, 3] = 3.0 * (j % side); T[:, 1, 3] = 3.0 * (j // side)
        store.set_pose(j, T, j.astype(np.int64))
        ctx.sync()
        return T

    result = dict(slots=a.slots, k=K, starts=S, runlen=a.runlen, reps=a.reps, inner=a.inner)
    store = api.KeyframeStore(ctx, a.slots)
    side = int(np.ceil(np.sqrt(a.slots)))
    T_host = fill(store, a.slots, side)
    t_host = np.ascontiguousarray(T_host[:, :3, 3]); R_host = T_host[:, :3, :3].astype(np.float64)
    offsets = np.zeros((S, 6), np.float32); offsets[:, 0] = [0.0, 0.1, -0.1, 0.2, -0.2, 0.3, -0.3, 0.4][:S] if S <= 8 else 0.0
    # query q: scan 2 of pair q at the pose of slot home[q] (which holds scan 1 of pair q) moved by the pair's motion; a radius that admits about K slots
    home = [(side // 2) * side // pairs * pairs + pairs * (q % 2) + q for q in range(8)]
    Tq = np.stack([(T_host[h].astype(np.float64) @ api.pose_step_from_X(motion[q]).astype(np.float64)).astype(np.float32) for q, h in enumerate(home)])
    sq = np.full(8, 10 ** 6, np.int64)
    radius = 3.0 * np.sqrt(K / np.pi) * 1.15

    def euler_of(R):
        return np.array([np.arctan2(-R[2, 1], R[2, 2]), np.arcsin(np.clip(R[2, 0], -1, 1)), np.arctan2(-R[1, 0], R[0, 0])])

    def manual(Q, bufs):
        """INTEGRATION 'Loop closure against a keyframe store', step 3, by hand."""
        idx, x0 = [], np.zeros((Q * K * S, 6), np.float32)
        r2 = np.float32(radius) * np.float32(radius)
        n_live = 0
        for q in range(Q):
            d = Tq[q, :3, 3] - t_host
            dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            el = np.nonzero(dd <= r2)[0]
            cand = el[np.lexsort((el, dd[el]))][:K]
            Rq = Tq[q, :3, :3].astype(np.float64)
            for j in cand:
                base = np.concatenate([Rq.T @ (Tq[q, :3, 3].astype(np.float64) - t_host[j]), euler_of(Rq.T @ R_host[j])]).astype(np.float32)
                for s in range(S):
                    x0[n_live] = base + offsets[s]; idx.append(int(j)); n_live += 1
            bufs["group"][len(idx) - len(cand) * S:len(idx)] = q
        xd = torch.from_numpy(x0[:n_live]).to(dev)
        descs = [d2[int(g)] for g in bufs["group"][:n_live]]
        store.register_scored_device(idx, descs, prm, bufs["out"].data_ptr(), bufs["sc"].data_ptr(), xd.data_ptr())
        ctx.select_best_device(bufs["group"][:n_live], Q, bufs["sc"].data_ptr(), bufs["best"].data_ptr())
        ctx.sync()
        best = bufs["best"][:Q].cpu().numpy()
        rows = [(bufs["out"][int(b)].cpu(), bufs["sc"][int(b)].cpu()) for b in best if b >= 0]
        return [idx[int(b)] if b >= 0 else -1 for b in best], rows

    for Q in (1, 8):
        rec = torch.zeros((Q, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        query = api.ClosureQuery(float(radius), K, 0, S, float("inf"), 0, 0)
        bufs = dict(out=torch.zeros((Q * K * S, 48), dtype=torch.float32, device=dev), sc=torch.zeros((Q * K * S, 8), dtype=torch.int32, device=dev),
                    best=torch.zeros((Q,), dtype=torch.int32, device=dev), group=np.zeros(Q * K * S, np.int32))
        last = {}

        def one_call():
            store.close_device(d2[:Q], Tq[:Q], sq[:Q], prm, query, rec.data_ptr(), offsets)
            ctx.sync()
            last["rec"] = np.frombuffer(rec.cpu().numpy().tobytes(), api.CLOSURE_DTYPE)

        def by_hand():
            last["manual"] = manual(Q, bufs)

        med = measure({"a": one_call, "b": by_hand, "b2": by_hand})
        same = [int(s) for s in last["rec"]["slot"]] == last["manual"][0]
        aa = abs(med["b"] - med["b2"])
        result["query_q%d" % Q] = dict(close_ms=med["a"], manual_ms=med["b"], manual_again_ms=med["b2"], aa_spread_ms=aa, same_winners=same,
                                       n_candidates=[int(v) for v in last["rec"]["n_candidates"]], winners=[int(s) for s in last["rec"]["slot"]], homes=home[:Q],
                                       not_slower=bool(med["a"] <= min(med["b"], med["b2"]) + aa))
        print("(1) Q = %d: close_device %.3f ms   manual %.3f / %.3f ms   same winners: %s   winners %s (homes %s)" %
              (Q, med["a"], med["b"], med["b2"], same, result["query_q%d" % Q]["winners"], home[:Q]), flush=True)

    # (3) padding: 16 eligible, 2 eligible under K = 16, and K = 2
    rec1 = torch.zeros((1, api.CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    dq = np.sort(np.sqrt(((Tq[0, :3, 3] - t_host).astype(np.float64) ** 2).sum(1)))
    small = 0.5 * (dq[1] + dq[2])                                    # the two nearest slots and no third
    qk = lambda r, k: api.ClosureQuery(float(r), k, 0, S, float("inf"), 0, 0)
    calls = {"k16_full": lambda: store.close_device(d2[:1], Tq[:1], sq[:1], prm, qk(radius, K), rec1.data_ptr(), offsets),
             "k16_two": lambda: store.close_device(d2[:1], Tq[:1], sq[:1], prm, qk(small, K), rec1.data_ptr(), offsets),
             "k2": lambda: store.close_device(d2[:1], Tq[:1], sq[:1], prm, qk(small, 2), rec1.data_ptr(), offsets)}
    med = measure(calls)
    calls["k16_two"](); ctx.sync()
    n_two = int(np.frombuffer(rec1.cpu().numpy().tobytes(), api.CLOSURE_DTYPE)["n_candidates"][0])
    result["padding"] = dict(k_full_ms=med["k16_full"], k_two_eligible_ms=med["k16_two"], k2_ms=med["k2"], eligible_in_small_radius=n_two)
    print("(3) K = %d, all eligible %.3f ms   %d eligible %.3f ms   K = 2 %.3f ms" % (K, med["k16_full"], n_two, med["k16_two"], med["k2"]), flush=True)

    # (2) the search alone
    def search_time(st, n_slots, T):
        cand = torch.zeros((8, K), dtype=torch.int32, device=dev)
        out = {}
        for Q in (1, 8):
            q = api.ClosureQuery(float(radius), K, 0, 1, float("inf"), 0, 0)
            m = measure({"s": lambda: st.candidates_device(T[:Q], sq[:Q], q, cand.data_ptr())})["s"]
            out["q%d_ms" % Q] = m
            out["q%d_gbps" % Q] = 16.0 * n_slots / (m * 1e-3) / 1e9
            out["q%d_share_of_8tbps" % Q] = out["q%d_gbps" % Q] / 8000.0
        return out
    result["search_%d" % a.slots] = search_time(store, a.slots, Tq)
    print("(2) search over %d slots: %s" % (a.slots, result["search_%d" % a.slots]), flush=True)
    store.close()
    if a.big > 0:
        big = api.KeyframeStore(ctx, a.big, num_bins_phi=3, num_bins_theta=7)
        fill(big, a.big, int(np.ceil(np.sqrt(a.big))))
        result["search_%d" % a.big] = search_time(big, a.big, Tq)
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
