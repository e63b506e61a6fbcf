#!/usr/bin/env python3
"""The deskewer on one GPU, variants alternating in one process (GPU box):

    python scripts/bench_deskew.py [--scans 256] [--rings 64] [--steps 2048] [--reps 7] [--out FILE.json]

The workload: --scans organised sweeps of rings x steps rows (lidar_sim.make_sweep, scene 2000, drop=False: the misses stay as exact-zero rows, as a driver
delivers them), each in buffers of its own, each with its own twist, deskewed to the sweep end in ONE icet_deskew_device call.
  array     ICET_DESKEW_TIME_ARRAY: 28 bytes per row (12 read, 4 of time, 12 written)
  column    ICET_DESKEW_TIME_COLUMN_FAST: 24 bytes per row
  zeros     the array call on buffers of exact zeros: every row takes the early exit of the rule, so this is the kernel's memory traffic without its arithmetic
  copy      torch's device-to-device copy of the same 12 + 12 bytes per row: what streaming reaches on this machine
  torch     the same rule written with torch float64 ops, one scan after the other: what a user has today
A window is ONE call between two HIP events on the context's stream (torch's stream for the last two), behind 2 warm-up rounds; the figure is the median of
--reps windows.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STREAM_CEILING = 6.3e12                                               # bytes / s a streaming kernel reaches on an MI355X (8 TB/s is the HBM's specification)


def torch_deskew(p, s, xi, ref, fa, fb, fc):
    """The rule of icet_deskew.h with torch float64 ops on (3, N) float32 rows and (N,) float32 sweep fractions: (3, N) float32.  (Zero and non-finite rows are
    put back by a where, as the rule copies them.)"""
    import torch
    q = p.to(torch.float64)
    d = s.to(torch.float64) - ref
    th = d[None, :] * xi[3:, None]; sg = d[None, :] * xi[:3, None]
    u = (th[0] * th[0] + th[1] * th[1]) + th[2] * th[2]

    def horner(c):
        r = torch.full_like(u, c[9])
        for k in range(8, -1, -1):
            r = r * u + c[k]
        return r

    def cross(a, b):
        return torch.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    A, B, C = horner(fa), horner(fb), horner(fc)
    c1 = cross(th, q); c2 = cross(th, c1); r1 = cross(th, sg); r2 = cross(th, r1)
    o = ((q + A * c1) + B * c2) + ((sg + B * r1) + C * r2)
    keep = (torch.isfinite(p).all(0) & (p != 0).any(0) & (u <= 1.0))[None, :]
    return torch.where(keep, o.to(torch.float32), p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=8, help="sweeps that are ray-cast; the others are copies of them in buffers of their own")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-baselines", action="store_true", help="the three deskew calls only (under a profiler)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import deskew_model as dm
    from icet_amd import api, lidar_sim
    if not torch.cuda.is_available():
        raise SystemExit("bench_deskew: no GPU (this measures the MI355X path only)")
    dev = torch.device("cuda", 0)
    n = a.rings * a.steps
    rs = np.random.RandomState(1)
    twists = np.stack([dm.TWIST * rs.uniform(0.5, 1.5, 6) for _ in range(a.scans)])
    base = []
    for k in range(min(a.distinct, a.scans)):
        sweeps, _ = lidar_sim.make_sweep_sequence(1, twists[k], 2000, 2001 + k, a.rings, a.steps, device=dev, drop=False)
        base.append(sweeps[0])
    src = [base[k % len(base)][0].clone() for k in range(a.scans)]          # (3, n) float32 each
    tim = [base[k % len(base)][1].clone() for k in range(a.scans)]
    dst = [torch.zeros_like(s) for s in src]
    zsrc = [torch.zeros_like(s) for s in src]
    cnt = torch.zeros((a.scans, 8), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    rows = n * a.scans

    ctx = api.Context(0)
    stream = torch.cuda.ExternalStream(api.load_library().icet_stream(ctx._h), device=dev)
    dk = api.Deskewer(ctx)

    def recs(srcs, mode):
        r = [api.deskew_scan(s.data_ptr(), n, n, d.data_ptr(), n, t.data_ptr() if mode == api.DESKEW_TIME_ARRAY else 0, mode, a.steps if mode else 0, 0.0,
                                1.0 if mode == api.DESKEW_TIME_ARRAY else float(a.steps), 1.0, x) for s, d, t, x in zip(srcs, dst, tim, twists)]
        return (api.DeskewScan * len(r))(*r)                        # built once: a window holds the call, not the making of its records

    r_array, r_column, r_zeros = recs(src, api.DESKEW_TIME_ARRAY), recs(src, api.DESKEW_TIME_COLUMN_FAST), recs(zsrc, api.DESKEW_TIME_ARRAY)

    def timed(fn, st):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(fns, st, reps):
        for _ in range(2):
            for fn in fns.values():
                timed(fn, st)
        t = {k: [] for k in fns}
        for _ in range(reps):                                        # alternating
            for k, fn in fns.items():
                t[k].append(timed(fn, st))
        return {k: float(np.median(v)) for k, v in t.items()}, {k: [float(min(v)), float(max(v))] for k, v in t.items()}

    med, spread = measure({"array": lambda: dk.deskew_device(r_array, None, cnt.data_ptr()), "column": lambda: dk.deskew_device(r_column, None, cnt.data_ptr()),
                           "zeros": lambda: dk.deskew_device(r_zeros, None, cnt.data_ptr())}, stream, a.reps)
    dk.deskew_device(r_array, None, cnt.data_ptr()); ctx.sync()
    counts = {k: int(v) for k, v in zip(dm.CLASS_NAMES, cnt.cpu().numpy()[:, :5].sum(0))}
    # the array call against the model, on one scan (a bench that computes something else measures nothing)
    want, _ = dm.deskew(src[0].cpu().numpy().T, twists[0], tim[0].cpu().numpy(), ref=1.0)
    assert np.array_equal(dst[0].cpu().numpy().T.view(np.uint32), want.view(np.uint32)), "the device rows differ from the model"

    if a.no_baselines:
        print("deskew of %d sweeps x %d rows: array %.3f ms   column %.3f ms   all-zero rows %.3f ms" % (a.scans, n, med["array"], med["column"], med["zeros"]))
        return 0
    # the yardsticks on torch's own stream
    big_src = torch.cat(src, 1); big_dst = torch.zeros_like(big_src)
    cur = torch.cuda.current_stream(dev)
    fa, fb, fc = dm.FA, dm.FB, dm.FC
    xis = [torch.from_numpy(x).to(dev) for x in twists]

    def torch_all():
        for s, t, x, d in zip(src, tim, xis, dst):
            d.copy_(torch_deskew(s, t, x, 1.0, fa, fb, fc))

    torch.cuda.synchronize()
    med2, spread2 = measure({"copy": lambda: big_dst.copy_(big_src), "torch": torch_all}, cur, min(a.reps, 3))
    torch_equal = bool(np.array_equal(dst[0].cpu().numpy().T.view(np.uint32), want.view(np.uint32)))
    med.update(med2); spread.update(spread2)

    def line(ms, bytes_per_row):
        return dict(ms=ms, rows_per_s=rows / ms * 1e3, gb_per_s=rows * bytes_per_row / ms * 1e-6, fraction_of_streaming_ceiling=rows * bytes_per_row / ms * 1e3 / STREAM_CEILING)

    result = dict(scans=a.scans, rows_per_scan=n, rows=rows, reps=a.reps, counts=counts, ranges_ms=spread,
                  array=dict(at_28_bytes=line(med["array"], 28), at_24_bytes=line(med["array"], 24)),
                  column=dict(at_24_bytes=line(med["column"], 24)), zeros=dict(at_28_bytes=line(med["zeros"], 28)), copy=dict(at_24_bytes=line(med["copy"], 24)),
                  torch_float64=dict(equals_the_model_bit_for_bit=torch_equal, ms=med["torch"], rows_per_s=rows / med["torch"] * 1e3, times_the_array_call=med["torch"] / med["array"]))
    print("deskew of %d sweeps x %d rows (%s): array %.3f ms (%.2f G rows/s, %.0f GB/s at 28 B/row, %.0f GB/s at 24, %.0f %% of 6.3 TB/s)   column %.3f ms (%.0f GB/s at 24, %.0f %%)"
          % (a.scans, n, counts, med["array"], rows / med["array"] * 1e-6, rows * 28 / med["array"] * 1e-6, rows * 24 / med["array"] * 1e-6,
             100 * rows * 28 / med["array"] * 1e3 / STREAM_CEILING, med["column"], rows * 24 / med["column"] * 1e-6, 100 * rows * 24 / med["column"] * 1e3 / STREAM_CEILING), flush=True)
    print("            all-zero rows %.3f ms   device copy of 24 B/row %.3f ms (%.0f GB/s)   torch float64 %.1f ms (%.0f x the array call)"
          % (med["zeros"], med["copy"], rows * 24 / med["copy"] * 1e-6, med["torch"], med["torch"] / med["array"]), flush=True)
    dk.close()
    out = json.dumps(result)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
