#!/usr/bin/env python3
"""Saving and loading a keyframe store (icet_keyframe_store_save / _load) against a plain copy of its raw tables, in one process,
alternating (GPU box):

    python scripts/bench_snapshot.py [--slots 256,4096] [--reps 7] [--dir DIR] [--out FILE.json] [--once]

Workload: a 75 x 24 store whose slots hold the scan 1s of bench.py's default batch (lidar_sim.make_batch_pair(k), k < 256; a larger store repeats them), once
plain and once with appearance and coarse alignment enabled.  Per store: save (all slots, to a file in --dir), load (into a second store of the same shape),
and the yardstick -- the bytes of the store's four raw tables copied device -> pinned host -> device with plain copies.  A window is one call ended by a
device synchronise, on the host clock; the figure is the median over --reps windows, the three variants alternating.  Also: file bytes against raw table bytes,
and that the loaded store holds the saved one's bits (debug_fetch of a few slots).  --once: one save and one load of the first store with both features enabled and nothing else, for a
kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/bench_snapshot.py --once).  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="256,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dir", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_snapshot: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    s1 = [lidar_sim.make_batch_pair(k, device=dev)[0].contiguous() for k in range(256)]
    torch.cuda.synchronize()
    d1 = [(t.data_ptr(), t.shape[1], t.shape[1]) for t in s1]
    tmp = a.dir or tempfile.mkdtemp(prefix="icet_snapshot_")
    os.makedirs(tmp, exist_ok=True)
    V = 24 * 75
    results = []
    for n_slots in [int(v) for v in a.slots.split(",")]:
        for features in ((True,) if a.once else (False, True)):
            ctx = api.Context(0)
            src, dst = api.KeyframeStore(ctx, n_slots), api.KeyframeStore(ctx, n_slots)
            for st in (src, dst):
                if features:
                    st.enable_coarse(); st.enable_appearance()
            for first in range(0, n_slots, 256):
                cnt = min(256, n_slots - first)
                src.put_device(list(range(first, first + cnt)), d1[:cnt])
            ctx.sync()
            path = os.path.join(tmp, "bench_%d_%d.kfs" % (n_slots, features))
            if a.once:
                src.save(path); dst.load(path); os.remove(path)
                src.close(); dst.close(); ctx.close()
                print(json.dumps(dict(once=True, slots=n_slots, features=features)))
                return 0
            raw = n_slots * (V * 128 + 2 * V + 4)                    # SlotHot + SlotFit rows, slot_of_voxel rows, n_slots
            if features:
                raw += n_slots * ((120 * 5 + 120 + 1) * 4 + 256 * 256 // 8 + 4)
            d_raw = torch.empty(raw, dtype=torch.uint8, device=dev); h_raw = torch.empty(raw, dtype=torch.uint8).pin_memory()

            def copy_out():
                h_raw.copy_(d_raw, non_blocking=True); torch.cuda.synchronize()

            def copy_in():
                d_raw.copy_(h_raw, non_blocking=True); torch.cuda.synchronize()

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            fns = dict(save=lambda: src.save(path), load=lambda: dst.load(path), copy_out=copy_out, copy_in=copy_in)
            for fn in fns.values():                                    # warm-up
                fn()
            t = {k: [] for k in fns}
            for _ in range(a.reps):                                    # alternating
                for k, fn in fns.items():
                    t[k].append(timed(fn))
            med = {k: float(np.median(v)) for k, v in t.items()}
            file_bytes = os.path.getsize(path)
            probe = sorted({0, n_slots // 2, n_slots - 1})
            same = all(np.array_equal(src.debug_fetch(s, w), dst.debug_fetch(s, w)) for s in probe
                       for w in ("hot", "fit", "slot_of_voxel") + (("descriptor", "weights", "grid") if features else ()))
            r = dict(slots=n_slots, features=features, raw_bytes=raw, file_bytes=file_bytes, file_over_raw=file_bytes / raw, save_ms=med["save"], load_ms=med["load"],
                     copy_out_ms=med["copy_out"], copy_in_ms=med["copy_in"], save_over_copy=med["save"] / med["copy_out"], load_over_copy=med["load"] / med["copy_in"],
                     spread={k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}, same_bits=bool(same))
            results.append(r)
            print("%5d slots%s: file %.1f MB = %.2f x raw %.1f MB   save %.2f ms (copy out %.2f)   load %.2f ms (copy in %.2f)   same bits: %s"
                  % (n_slots, " + features" if features else "", file_bytes / 1e6, r["file_over_raw"], raw / 1e6, med["save"], med["copy_out"], med["load"], med["copy_in"], same), flush=True)
            os.remove(path)
            del d_raw, h_raw
            src.close(); dst.close(); ctx.close()
    line = json.dumps(dict(reps=a.reps, results=results))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["same_bits"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
