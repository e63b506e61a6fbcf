#!/usr/bin/env python3
"""bench.py -- scan-pairs/s and ms/pair of the MI355X-native ICET hot path (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W

N > 1 needs one process per GPU.  Started by the driver's launcher (python -m torch.distributed.run ... bench.py --gpus N ...)
the script finds WORLD_SIZE in its environment and is one rank.  Started WITHOUT a launcher (plain `python bench.py --gpus N`)
it starts that launcher itself as a CHILD process -- before anything here has touched the GPU -- relays the child's JSON line and
exits with the child's return code; it never re-executes a process that has initialised HIP and never silently measures one GPU.
`--multi` measures the other N-GPU form instead: ONE process, the native icet_multi_* entry (one context + host thread per GPU,
peer-copy or RCCL gather inside the C++ library).

A "step" is one pass of the hot path (keyframe build + 7 Gauss-Newton iterations, 75 x 24 voxels) over
one batch of synthetic 64-channel scan pairs per GPU: BASELINE.json configs[2] (256 independent pairs,
throughput mode) at N=1, and its sharded form configs[3] (256 pairs per GPU, pair k -> rank k mod N,
one RCCL all-gather of 48 floats per pair) at N>1 -- weak scaling.  Exactly K steps are timed (after W
untimed ones); `ms_per_step` is one of them.  With `--full`, configs[1] (ONE pair, latency) is also
measured and reported under "latency"; configs[0] is the CPU-only plumbing case and configs[4] the
high-resolution sweep: parity-test cases; configs[4] is also timed under `--full` ("highres").

A plain run sets up, warms up, times the K steps, writes `--dump-outputs DIR` (X.npy, pred_stds.npy,
cov.npy of every pair of the last timed step; the node workloads: the last frame's result) and prints
its line.  Everything else -- the sub-records below, the gather alone, the other storage order, the
real-data batch, the PCIe-inclusive and constructor paths, the nodes' phase timing and burst -- runs
only with `--full`; without it those fields are null.

Inputs are generated on the device (icet_amd.lidar_sim, seeded per pair) and are resident in HBM before
the timed region.  rank 0 prints ONE JSON line with the driver's contract fields plus, with `--full`,
  "roofline":     k_gn_accumulate (the dominant kernel): algorithmic bytes per launch = 12 B x scan-2
                  points of the batch (x|y|z read once, transform fused, nothing N-sized written),
                  divided by the launch duration measured with HIP events on the solve stream.
  "cpu_baseline": the CPU restatement (oracle/, kind "port") timed on this box's host cores on a bounded
                  sample of the same pairs.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec
PUBLISHED_MS_PER_PAIR = 35.0   # reference README.md:59 (Ryzen 5800X) -- different hardware, informational


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps (default 3; the sequential workloads: 8 -- each of a node's two contexts sees a launch key, captures its graph and replays it from its third frame on)")
    ap.add_argument("--pairs-per-gpu", type=int, default=256)
    ap.add_argument("--workload", choices=["batch", "highres", "odometry", "mapmaker", "sample"], default="batch",
                    help="sample: the batch built from the reference's two REAL scan pairs (tests/golden/scans_*.npz), each pair k rotated by its own small rigid motion, zero rows kept")
    ap.add_argument("--order", choices=["ring", "azimuth"], default="ring")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--cpu-sample-pairs", type=int, default=256)
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE",
                    help="icet_set_option on the context (launch-shape experiments); echoed in config.options")
    ap.add_argument("--distinct", type=int, default=0, help="generate only this many distinct pairs and cycle them (0 = all distinct)")
    ap.add_argument("--multi", action="store_true", help="one process, N GPUs through the native icet_multi_* entry (no torch.distributed)")
    ap.add_argument("--multi-gather", choices=["peer", "rccl"], default="peer", help="--multi: peer copies (default) or the library's RCCL all-gather")
    ap.add_argument("--min-timed-s", type=float, default=0.0, help="repeat the K timed steps until the timed region is at least this long (default 0: exactly K timed steps)")
    ap.add_argument("--full", action="store_true", help="also run everything beside the headline: per-kernel timing and roofline, HBM traffic, CPU baseline, latency, "
                                                        "highres, the other storage order, real-data batch, PCIe-inclusive and constructor paths, the nodes' phase timing and burst")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed to DIR/<name>.npy (float32)")
    ap.add_argument("--no-h2d", action="store_true", help="skip the PCIe-inclusive sub-record")
    ap.add_argument("--traffic", choices=["live", "file", "none"], default="live",
                    help="roofline.traffic: measured by two child runs under rocprofv3 --pmc (each capped at 60 s; falls back to the file), read from profiles/traffic_latest.json, or left null")
    ap.add_argument("--flags", type=int, default=0, help="icet_params.flags for the solves (e.g. 16 = ICET_FLAG_ROUNDTRIP_SCAN2: what the reference's scan-2 round trips cost); echoed in config")
    ap.add_argument("--dry-run-launch", action="store_true", help="print what `--gpus N` would start (JSON) and exit: no GPU, no child")
    a = ap.parse_args(argv)
    if a.warmup is None: a.warmup = 8 if a.workload in ("odometry", "mapmaker") else 3
    return a


def launcher_command(args, argv, port=None):
    """The child this script starts for `--gpus N` without a launcher: the driver's own command line (one rank per GPU over RCCL)."""
    if port is None:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + [a for a in argv if a != "--dry-run-launch"]


def plan_launch(args, env):
    """What `main` does about processes, decided BEFORE any GPU call.  Returns (action, detail):
    'run'     this process is the (or a) rank / the single process
    'spawn'   --gpus N > 1 without a launcher: start one as a child
    'refuse'  the environment contradicts --gpus (never measure fewer GPUs than asked for)"""
    world = env.get("WORLD_SIZE")
    if args.multi:
        if world is not None and int(world) > 1:
            return "refuse", "--multi is one process over N GPUs; it must not run under a %s-rank launcher" % world
        return "run", "one process, %d device(s) through icet_multi" % args.gpus
    if world is None:
        return ("spawn", "no launcher in the environment") if args.gpus > 1 else ("run", "single GPU")
    if int(world) != args.gpus:
        return "refuse", "--gpus %d but WORLD_SIZE=%s" % (args.gpus, world)
    return "run", "rank of a %s-rank launch" % world


def dump_outputs(dirname, arrays):
    """--dump-outputs: one DIR/<name>.npy per array, float32 (the outputs of the last timed step, as a caller of that path receives them)."""
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), np.ascontiguousarray(np.asarray(a, dtype=np.float32)))


def _is_elf(path):
    try:
        with open(path, "rb") as f:
            return f.read(4) == b"\x7fELF"
    except OSError:
        return False


def measure_traffic_live(timeout_s=60):
    """HBM bytes per k_gn_accumulate launch, measured NOW on this box: two child runs of this script under `rocprofv3 --kernel-trace --pmc` (FETCH_SIZE and
    WRITE_SIZE in separate passes, as /opt/skills/guides/MI355X_MICROARCH.md prescribes; FETCH_SIZE doubled: on gfx950 it reports half the bytes of a 16-B/lane
    coalesced streaming read), each over the default workload's whole-batch launches.  Returns (bytes, note) or (None, why)."""
    import csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "rocprofv3 not found"
    # The program behind `--` must be the interpreter ITSELF: the profiler's preloaded library has initialised the GPU by then, and a shim or wrapper script
    # (pyenv, a `#!/usr/bin/env` launcher) would be an exec after that -- not allowed on this pool
    py = os.path.realpath(sys.executable)
    if not _is_elf(py):
        return None, "the interpreter (%s) is not an ELF binary: no live measurement" % py
    vals = {}
    env = dict(os.environ); env["TMPDIR"] = "/tmp"; env["ICET_BENCH_CHILD"] = "1"
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="icet_pmc_", dir="/tmp")
        # counters for k_gn_accumulate only: with every dispatch of the pair generator profiled a pass took 70 s (round 5: 142 s of the default run's 155 s)
        cmd = [exe, "--kernel-trace", "--pmc", counter, "--kernel-include-regex", "k_gn_accumulate", "--output-format", "csv", "-d", d, "--", py, os.path.abspath(__file__),
               "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-latency", "--no-h2d", "--min-timed-s", "0"]
        try:
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout_s)
        except Exception as e:
            return None, "rocprofv3 %s pass: %s" % (counter, type(e).__name__)
        files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None, "rocprofv3 %s pass failed (rc %d)" % (counter, r.returncode)
        v = [float(row["Counter_Value"]) for row in csv.DictReader(open(files[0], newline="")) if "k_gn_accumulate" in row["Kernel_Name"] and row["Counter_Name"] == counter]
        shutil.rmtree(d, ignore_errors=True)
        if not v:
            return None, "no k_gn_accumulate rows in the %s pass" % counter
        v = [x for x in v if x >= 0.6 * max(v)]              # the whole-batch launches (the timed steps); parts of other steps are smaller
        vals[counter] = sum(v) / len(v)
    return (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0, "measured in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, (2 x FETCH_SIZE + WRITE_SIZE) x 1024 B per launch"


def run_nodes(args):
    """--workload odometry | mapmaker: the per-frame body of the reference's two nodes (include/icet_nodes.h).
    A step is ONE lidar frame pushed from HBM: range filter -> ICET(prev, cur) -> pose chain (-> 600k-row map update).
    Sequential by construction (frame k+1 needs frame k's X): N > 1 runs independent replicas."""
    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0")); local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("ICET_BENCH_SHARE_DEVICE"): local_rank = int(os.environ["ICET_BENCH_SHARE_DEVICE"])      # rehearsal hook (several ranks on one card), as in main()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("ICET_BENCH_BACKEND", "nccl")
        if backend == "nccl": dist.init_process_group(backend="nccl", device_id=dev)
        else: dist.init_process_group(backend=backend)
    import icet_amd
    from icet_amd import lidar_sim, api
    kw = dict(api.ODOMETRY_NODE if args.workload == "odometry" else api.MAP_MAKER_NODE)
    n_frames = args.warmup + args.steps + 1
    frames = lidar_sim.make_sequence(n_frames, motion=(0.25, 0.02, 0.005, 0.001, -0.001, 0.006), device=dev)
    def padded(s):
        n = s.shape[1]; ld = (n + 63) // 64 * 64
        buf = torch.zeros((3, ld), dtype=torch.float32, device=dev); buf[:, :n] = s
        return buf
    bufs = [padded(s) for s in frames]
    torch.cuda.synchronize()
    ctx = icet_amd.Context(local_rank)
    node = api.Node(ctx, **kw)
    push = lambda k: node.push_device(bufs[k].data_ptr(), frames[k].shape[1], bufs[k].shape[1])
    for k in range(args.warmup + 1):
        push(k)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    tim = {"filter_ms": 0.0, "solve_ms": 0.0, "map_ms": 0.0}
    t0 = time.perf_counter()
    per_frame_X = []
    for k in range(args.warmup + 1, n_frames):
        r = push(k)
        per_frame_X.append(r["X"].copy())
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=(dev if dist.get_backend() == "nccl" else "cpu")); dist.all_reduce(tt, op=dist.ReduceOp.MAX); dt = float(tt.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {k2: r[k2] for k2 in ("X", "pred_stds", "pose", "quat", "solved", "diverged", "n_kept", "map_rows")})
    for key in tim: tim[key] /= max(args.steps, 1)
    if world == 1 and args.full:
        # a pipelined frame is one graph launch (filter + loop together, no timing events): the phases are timed on a second node that keeps them apart (ICET_NODE_TIME_PHASES)
        node_t = api.Node(ctx, **dict(kw, flags=kw.get("flags", 0) | api.NODE_TIME_PHASES))
        for k in range(args.warmup + 1):
            node_t.push_device(bufs[k].data_ptr(), frames[k].shape[1], bufs[k].shape[1])
        tim = {"filter_ms": 0.0, "solve_ms": 0.0, "map_ms": 0.0}
        m_t = min(args.steps, 16)
        for k in range(args.warmup + 1, args.warmup + 1 + m_t):
            node_t.push_device(bufs[k].data_ptr(), frames[k].shape[1], bufs[k].shape[1])
            t = node_t.last_timing()
            for key in tim: tim[key] += t[key] / m_t
        node_t.close()
    # ---- the same frames through ONE call (icet_node_push_many_device): the library pushes them one after the other -- what is left out is this script's per-frame
    # Python / ctypes work (round 6: the device-chained burst of rounds 4-5 was slower than one-launch frames and was removed) ----
    burst = None
    if args.workload == "odometry" and world == 1 and args.full:
        node_b = api.Node(ctx, **kw)
        for k in range(args.warmup + 1):
            node_b.push_device(bufs[k].data_ptr(), frames[k].shape[1], bufs[k].shape[1])
        fr = [(bufs[k].data_ptr(), frames[k].shape[1], bufs[k].shape[1]) for k in range(args.warmup + 1, n_frames)]
        torch.cuda.synchronize()
        tb = time.perf_counter()
        rb = node_b.push_many_device(fr)
        tb = time.perf_counter() - tb
        same = all(np.array_equal(rb[i]["X"], per_frame_X[i]) for i in range(len(fr)))
        burst = {"frames": len(fr), "frames_per_s": round(len(fr) / tb, 1), "ms_per_frame": round(tb / len(fr) * 1e3, 4), "bits_equal_frame_by_frame": bool(same),
                 "note": "icet_node_push_many_device: the same frames through one library call (frame by frame inside the library, no per-frame Python / FFI work)"}
        node_b.close()
    n_mean = int(np.mean([f.shape[1] for f in frames]))
    cap = kw["map_capacity"]
    if cap:
        kern, bytes_per_launch, ms = "k_map_add_scan", 24.0 * cap, tim["map_ms"]
        note = "12 B read + 12 B written per ring row x %d rows; HIP events around the kernel" % cap
    else:
        kern, bytes_per_launch, ms = "k_range_count+k_range_scan+k_range_scatter", 36.0 * n_mean, tim["filter_ms"]
        note = "x|y|z read by the count and the scatter pass + kept rows written (~36 B/row); filter_ms / solve_ms from a second node with ICET_NODE_TIME_PHASES (the timed frames run filter + loop as one graph launch)"
    achieved = bytes_per_launch / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        from oracle import pyoracle as po
        o = po.Node(**kw)
        host = [f.T.cpu().numpy() for f in frames]
        m = min(len(host) - 1, 8)
        o.push(host[0])
        tc = time.perf_counter()
        for k in range(1, m + 1):
            ro = o.push(host[k])
        tc = time.perf_counter() - tc
        cpu = {"value": round(m / tc, 3), "unit": "frames/s", "cores": 1, "kind": "port",
               "sample": "first %d frames of the same sequence through oracle/icet_nodes_oracle.cpp (serial), %.1f s wall" % (m, tc)}
        o.close()
    if rank == 0:
        print(json.dumps({
            "metric": "frames/sec, sequential %s (64-ch, 75x24 voxels, %d iters)" % ("odometry_node" if args.workload == "odometry" else "map_maker_node + 600k-row map", kw["runlen"]),
            "value": round(world * args.steps / dt, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / max(args.steps, 1) * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "SURVEY 8 f1/f3: %s per-frame body, one synthetic 64-ch frame (~%dk pts) per step pushed from HBM, result on the host every frame; replicas only when N>1"
                                   % (args.workload, n_mean // 1000), "points_per_frame_mean": n_mean, **{k2: v for k2, v in kw.items()}},
            "roofline": {"kernel": kern, "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "traffic": None, "algorithmic_bytes_per_launch": bytes_per_launch, "avg_launch_ms": round(ms, 5), "note": note,
                         "filter_ms": round(tim["filter_ms"], 4), "solve_ms": round(tim["solve_ms"], 4), "map_ms": round(tim["map_ms"], 4)} if args.full else None,
            "burst": burst,
            "cpu_baseline": cpu, "last_X": [round(float(v), 5) for v in r["X"]]}), flush=True)
    node.close(); ctx.close()
    if world > 1:
        dist.barrier(); dist.destroy_process_group()


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse(argv)
    # ---- processes first: decided from the arguments and the environment alone, before anything touches the GPU ----
    action, why = plan_launch(args, os.environ)
    if args.dry_run_launch:
        print(json.dumps({"action": action, "why": why, "command": launcher_command(args, argv, port=29500) if action == "spawn" else None}))
        return 0
    if action == "refuse":
        raise SystemExit("bench.py: " + why)
    if action == "spawn":
        import subprocess
        cmd = launcher_command(args, argv)
        env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0"); env.setdefault("MASTER_ADDR", "127.0.0.1")
        print("bench.py: --gpus %d without a launcher (%s): starting %s" % (args.gpus, why, " ".join(cmd)), file=sys.stderr, flush=True)
        child = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in child.stdout.splitlines() if ln.startswith("{\"metric\"")]
        for ln in child.stdout.splitlines():
            if not ln.startswith("{\"metric\""):
                print(ln, file=sys.stderr)
        if lines: print(lines[-1], flush=True)                 # (also from a run that ends non-zero: the gloo fallback prints its line, then its ranks exit 3)
        if child.returncode != 0 or not lines:
            rc = child.returncode or 1
            try:
                if lines and json.loads(lines[-1])["config"].get("rccl_ranks") == 0: rc = 3      # the launcher reports 1 for ranks that exited 3
            except (ValueError, KeyError): pass
            raise SystemExit(rc)
        return 0
    if args.workload in ("odometry", "mapmaker"):
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
        return run_nodes(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    multi = args.multi
    n_dev = args.gpus if multi else 1                              # devices THIS process drives
    if multi and torch.cuda.device_count() < args.gpus and not os.environ.get("ICET_BENCH_SHARE_DEVICE"):
        raise SystemExit("bench.py --multi --gpus %d: only %d device(s) visible" % (args.gpus, torch.cuda.device_count()))
    # rehearsal hook: several ranks / shards on ONE card (the 1-GPU dev box) -- never set by the driver
    share = os.environ.get("ICET_BENCH_SHARE_DEVICE")
    if share:
        local_rank = int(share)
    dev_ids = [int(share)] * n_dev if (multi and share) else (list(range(n_dev)) if multi else [local_rank])
    torch.cuda.set_device(dev_ids[0])
    dev = torch.device("cuda", dev_ids[0])
    import torch.distributed as dist
    backend = os.environ.get("ICET_BENCH_BACKEND", "nccl")      # "gloo" only for rehearsing N ranks on one card
    collective_note = None
    g_data = None                                                  # the group the 48-float gather runs on (RCCL); None = the default (gloo) group
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        # Control plane on gloo (barriers, the max-reduction of the timing, and the agreement below); data plane -- the one all-gather per step -- on
        # an RCCL group of the same ranks.  Whether RCCL works is decided COLLECTIVELY (a rank falling back on its own while the others
        # stay in the RCCL group would hang the job): every rank tries, the verdicts are min-reduced over gloo, all ranks take the same path.
        dist.init_process_group(backend="gloo")
        if dist.get_world_size() != args.gpus:
            raise SystemExit("bench.py: process group has %d ranks, --gpus %d" % (dist.get_world_size(), args.gpus))
        if backend == "nccl":
            ok, why = 1, ""
            try:
                g_data = dist.new_group(backend="nccl", timeout=datetime.timedelta(seconds=180))
                probe = torch.zeros(1, device=dev)
                dist.all_reduce(probe, group=g_data)                     # the communicator is really built here: fail now, not inside the timed region
                torch.cuda.synchronize(dev)
            except Exception as e:
                ok, why = 0, "%s: %s" % (type(e).__name__, e)
                sys.stderr.write("bench.py: rank %d: RCCL group failed (%s)\n" % (rank, why))
            flag = torch.tensor([ok], dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 0:                                    # some rank has no working RCCL: the 48-float gather goes through the host on EVERY rank, and the line says so
                backend, g_data = "gloo", None
                collective_note = "gloo fallback: RCCL group failed on at least one rank%s" % ((" (here: %s)" % why.split(":")[0]) if why else "")

    import icet_amd
    from icet_amd import lidar_sim, api
    from icet_amd.dist import gather_results, shard_indices

    if args.workload in ("batch", "sample"):
        rings, steps_az, T, P, iters = 64, 2048, 75, 24, 7
        n_local = args.pairs_per_gpu
    else:
        rings, steps_az, T, P, iters = 128, 4096, 150, 48, 10
        n_local = 1
    n_gpus = args.gpus if multi else world
    n_global = n_local * n_gpus
    ids = list(range(n_global)) if multi else shard_indices(n_global, rank, world)        # pairs THIS process holds (multi: all, pair k on device k mod N)

    def real_pair(k, dk):
        """Pair k of the REAL-data batch: the reference's sample pairs (src/sample_data/frame_804/805.npy for even k, python/point_clouds/sample_pc_1/2.npy for odd k;
        committed float32 fixtures) with BOTH scans turned by one small rotation of pair k's own (yaw +-0.05, roll / pitch +-0.01 rad, seed 7000 + k): the registration
        stays the pair's, every pair's rows fall into other voxels and sort differently, and the invalid returns stay exact zero rows (thousands per scan, src/icet.cpp Q2)."""
        if "fx" not in real_cache:
            real_cache["fx"] = [np.load(os.path.join(ROOT, "tests", "golden", "scans_%s.npz" % nm)) for nm in ("frame_804_805", "sample_pc_1_2")]
        fx = real_cache["fx"][k % 2]
        key = (k % 2, str(dk))
        if key not in real_cache:
            real_cache[key] = tuple(torch.from_numpy(np.ascontiguousarray(fx[nm].T)).to(dk) for nm in ("scan1", "scan2"))
        a, b = real_cache[key]
        R = torch.as_tensor(lidar_sim.real_batch_rotation(k), device=dk)
        return (R @ a).contiguous(), (R @ b).contiguous()
    real_cache = {}

    walls = {}; _w = [time.perf_counter(), "startup"]
    def mark(name):                                                # wall seconds of every phase of this script (what the driver's clock is spent on)
        t = time.perf_counter(); walls[_w[1]] = round(walls.get(_w[1], 0.0) + t - _w[0], 2); _w[0] = t; _w[1] = name
    # ---- synthetic inputs, generated in HBM ------------------------------------------------------
    mark("generate")
    t_gen = time.time()
    scans1, scans2 = [], []
    distinct = args.distinct if args.distinct > 0 else len(ids)
    for j, k in enumerate(ids):
        dk = torch.device("cuda", dev_ids[j % n_dev])
        if j < distinct:
            if args.workload == "batch":
                s1, s2, _ = lidar_sim.make_batch_pair(k, rings, steps_az, device=dk, order=args.order)
            elif args.workload == "sample":
                s1, s2 = real_pair(k, dk)
            else:
                s1, s2, _ = lidar_sim.make_pair(9000, 9001, lidar_sim.DEFAULT_MOTION, rings, steps_az, device=dk, order=args.order)
        else:
            s1, s2 = scans1[j % distinct], scans2[j % distinct]
            if s1.device != dk:
                s1, s2 = s1.to(dk), s2.to(dk)
        scans1.append(s1); scans2.append(s2)
    for d in set(dev_ids):
        torch.cuda.synchronize(d)
    t_gen = time.time() - t_gen
    n1 = [int(s.shape[1]) for s in scans1]; n2 = [int(s.shape[1]) for s in scans2]

    def padded(s):
        """Column-major N x 3 with the leading dimension rounded up to 64 floats, so that y[] and z[] start 16-byte
        aligned (Eigen's own allocations are 16-byte aligned too: -DEIGEN_ALIGN_16, CMakeLists.txt:5)."""
        n = s.shape[1]; ld = (n + 63) // 64 * 64
        if ld == n:
            return s
        buf = torch.zeros((3, ld), dtype=torch.float32, device=s.device); buf[:, :n] = s
        return buf
    cache = {}
    def padded_cached(s):
        if s.data_ptr() not in cache:
            cache[s.data_ptr()] = padded(s)
        return cache[s.data_ptr()]
    bufs1 = [padded_cached(s) for s in scans1]; bufs2 = [padded_cached(s) for s in scans2]
    d1 = [(b.data_ptr(), n, b.shape[1]) for b, n in zip(bufs1, n1)]
    d2 = [(b.data_ptr(), n, b.shape[1]) for b, n in zip(bufs2, n2)]

    mark("warmup_and_timed_region")
    p_plain = api.Params(iters, P, T, 25, 0.1, 0.1, args.flags)
    p_timed = api.Params(iters, P, T, 25, 0.1, 0.1, args.flags | api.FLAG_TIMING)
    out = torch.zeros((len(ids), 48), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    mctx = None
    if multi:
        mctx = api.MultiContext(dev_ids)
        if args.multi_gather == "rccl":
            mctx.set_option("gather", 1)
        for kv in args.set:
            name, value = kv.split("=", 1)
            mctx.set_option(name, float(value))
        mctx.reserve(p_plain, len(ids), sum(n1), sum(n2))
        ctx = mctx.context(0)                                      # timing / roofline are read from the first device's context
        for d in set(dev_ids):
            torch.cuda.synchronize(d)
    else:
        ctx = icet_amd.Context(local_rank, stream=stream.cuda_stream)
        for kv in args.set:
            name, value = kv.split("=", 1)
            ctx.set_option(name, float(value))
        ctx.reserve(p_plain, len(ids), sum(n1), sum(n2))

    def step(params):
        if multi:
            mctx.solve_batch_device(d1, d2, params, out.data_ptr(), asynchronous=not (params.flags & api.FLAG_TIMING))   # queued on the device threads; fence() syncs
            return out
        with torch.cuda.stream(stream):
            ctx.solve_batch_device(d1, d2, params, out.data_ptr())
            if world > 1:
                if backend == "nccl":
                    return gather_results(out, n_global, rank, world, group=g_data)
                ctx.sync()
                return gather_results(out.cpu(), n_global, rank, world).to(dev)
        return out

    def fence():
        if multi:
            mctx.sync()                                                # every queued solve + gather has completed on every device
        for d in set(dev_ids):
            torch.cuda.synchronize(d)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step(p_plain)
    fence()
    # The K timed steps, bracketed by barrier + synchronize.  With --min-timed-s > 0 the bracket is REPEATED (each repetition:
    # exactly K steps between two fences) until the timed region is at least that long; `ms_per_step` is the mean over every
    # timed step, `value` the pairs of all of them / the total time.  By default exactly K steps are timed.
    reps_t, dt, rep_ms = 0, 0.0, []
    while True:
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            res = step(p_plain)
        fence()
        d = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([d], dtype=torch.float64)                 # control plane: gloo
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            d = float(tt.item())
        dt += d; reps_t += 1; rep_ms.append(d / max(args.steps, 1) * 1e3)
        if dt >= args.min_timed_s or reps_t >= 1000:      # every rank sees the same (max-reduced) dt, so every rank leaves together
            break
    steps_total = args.steps * reps_t
    ms_per_step = dt / max(steps_total, 1) * 1e3
    pairs_per_s = n_global * steps_total / dt
    if args.dump_outputs and rank == 0:
        r_host = res.float().cpu().numpy()                         # n_global x 48 in global pair order: X | pred_stds | cov
        pick = {}
        if r_host.nbytes > 60 * 2**20:                             # beyond ~320 k pairs: a fixed, seeded sample of pairs (their ids in pair_index.npy)
            idx = np.sort(np.random.RandomState(0).choice(len(r_host), (60 * 2**20) // (48 * 4), replace=False))
            r_host, pick = r_host[idx], {"pair_index": idx}
        dump_outputs(args.dump_outputs, {"X": r_host[:, :6], "pred_stds": r_host[:, 6:12], "cov": r_host[:, 12:48].reshape(-1, 6, 6), **pick})

    # ---- the gather alone (N > 1): what the collective costs on top of the solve ----
    gather_ms = None
    if world > 1 and backend == "nccl" and args.full:
        fence()
        tg = time.perf_counter()
        with torch.cuda.stream(stream):
            for _ in range(20):
                gather_results(out, n_global, rank, world, group=g_data)
        fence()
        gather_ms = (time.perf_counter() - tg) / 20 * 1e3

    mark("roofline_events")
    # ---- per-kernel timing with HIP events on the solve stream (extra steps, not part of `value`) ----
    acc_ms, kf_ms, gn_ms, launches = 0.0, 0.0, 0.0, 0
    reps = max(3, min(args.steps, 10))
    for _ in range(reps if args.full else 0):
        step(p_timed)
        t = ctx.last_timing()
        acc_ms += t["accumulate_ms"]; kf_ms += t["keyframe_ms"]; gn_ms += t["gn_loop_ms"]; launches += t["accumulate_launches"]
    fence()
    acc_launch_ms = acc_ms / max(launches, 1)
    n2_timed = [n for j, n in enumerate(n2) if j % n_dev == 0]                   # the pairs of the context whose events were read
    n1_timed = [n for j, n in enumerate(n1) if j % n_dev == 0]
    bytes_per_launch = 12.0 * float(sum(n2_timed))
    achieved = bytes_per_launch / (acc_launch_ms * 1e-3) / 1e9 if acc_launch_ms > 0 else 0.0
    bytes_path = sum(12.0 * a + 12.0 * b * iters + 192.0 for a, b in zip(n1, n2)) * (1 if multi else world)      # whole job
    traffic, traffic_note = None, None
    tpath = os.path.join(ROOT, "profiles", "traffic_latest.json")
    default_workload = args.workload == "batch" and n_local == 256 and args.distinct == 0 and not args.set and not args.flags and args.order == "ring"
    under_profiler = "rocprof" in os.environ.get("LD_PRELOAD", "") or any(k.startswith(("ROCP_", "ROCPROF")) for k in os.environ)      # no profiler inside a profiled run
    if args.full and args.traffic == "live" and default_workload and rank == 0 and n_gpus == 1 and not args.no_latency and not os.environ.get("ICET_BENCH_CHILD") and not under_profiler:
        # measured live (review r4, weak 9: the number used to come from a file a builder-side profile run had left behind)
        mark("traffic_live")
        traffic, traffic_note = measure_traffic_live()
        mark("roofline_events")
    if args.full and traffic is None and args.traffic != "none" and os.path.exists(tpath) and args.workload == "batch" and n_local == 256 and args.distinct == 0:
        # fallback: the PMC numbers profiles/collect.sh collected on exactly this workload (256 distinct pairs per GPU)
        try:
            traffic = json.load(open(tpath)).get("k_gn_accumulate_bytes_per_launch")
            traffic_note = "from profiles/traffic_latest.json (a builder-side rocprofv3 --pmc run of this workload)" + ((": live measurement unavailable: " + traffic_note) if traffic_note else "")
        except Exception:
            traffic = None

    mark("other_storage_order")
    # ---- the other storage order (BASELINE configs[1] names both): the SAME points stored azimuth-major (azimuth step slow, ring fast -- the
    # firing order of a spinning lidar) when the headline is ring-major, and the other way round.  Neighbouring lanes of k_gn_accumulate then
    # hold points of DIFFERENT voxels (rings 7.5 degrees of polar angle apart), i.e. shorter runs per lane and more LDS adds.  The reference's result
    # depends on the storage order (its swap loop is a function of the row indices), so this is another input, not another route to the same bits.
    az_major = None
    if args.full and args.workload == "batch" and not args.no_latency and world == 1 and not multi and args.distinct == 0:
        def reorder(sc):
            az = torch.atan2(sc[1], sc[0]); az = torch.where(az < 0, az + 2 * math.pi, az)
            step_id = torch.floor(az.double() * (steps_az / (2 * math.pi))).long()
            if args.order == "ring":
                key = step_id                                              # stable sort by azimuth step keeps the rings ascending inside a step
            else:
                key = torch.round(torch.asin((sc[2] / torch.linalg.vector_norm(sc, dim=0)).clamp(-1, 1)).double() * (rings / math.radians(45.0))).long()   # ring index up to an offset
            idx = torch.sort(key, stable=True).indices
            return padded(sc[:, idx].contiguous())
        a1 = [reorder(s) for s in scans1]; a2 = [reorder(s) for s in scans2]
        torch.cuda.synchronize()
        e1 = [(b.data_ptr(), n, b.shape[1]) for b, n in zip(a1, n1)]; e2 = [(b.data_ptr(), n, b.shape[1]) for b, n in zip(a2, n2)]
        out_az = torch.zeros_like(out)
        with torch.cuda.stream(stream):
            for _ in range(2):
                ctx.solve_batch_device(e1, e2, p_plain, out_az.data_ptr())
            ctx.sync()
            t0 = time.perf_counter(); nrep_az = max(args.steps, 5)
            for _ in range(nrep_az):
                ctx.solve_batch_device(e1, e2, p_plain, out_az.data_ptr())
            ctx.sync()
            az_ms = (time.perf_counter() - t0) / nrep_az * 1e3
            a_acc = a_kf = a_gn = 0.0; a_l = 0
            for _ in range(3):
                ctx.solve_batch_device(e1, e2, p_timed, out_az.data_ptr())
                t = ctx.last_timing()
                a_acc += t["accumulate_ms"]; a_kf += t["keyframe_ms"]; a_gn += t["gn_loop_ms"]; a_l += t["accumulate_launches"]
        other = "azimuth" if args.order == "ring" else "ring"
        az_launch = a_acc / max(a_l, 1)
        az_major = {"workload": "the same %d pairs, the same points, stored %s-major" % (len(ids), other), "pairs_per_s": round(len(ids) / (az_ms * 1e-3), 1), "ms_per_step": round(az_ms, 4),
                    "accumulate_avg_launch_ms": round(az_launch, 5), "roofline_frac": round(bytes_per_launch / (az_launch * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if az_launch > 0 else None,
                    "keyframe_ms_per_step": round(a_kf / 3, 4), "gn_loop_ms_per_step": round(a_gn / 3, 4), "all_finite": bool(torch.isfinite(out_az).all().item())}
        del a1, a2

    mark("sample_batch")
    # ---- throughput on REAL lidar data (review r4, item 4): 256 pairs made from the reference's two sample pairs (real_pair above), ONE
    # icet_solve_batch_device call per step.  Real scans differ from the synthetic ones where it hurts: thousands of exact-zero rows that share one key and
    # one voxel, a near field that puts tens of thousands of rows into a few bins, half the rows in a third of the voxels.
    sample_batch = None
    if args.full and args.workload == "batch" and not args.no_latency and world == 1 and not multi and args.distinct == 0:
        rp = [real_pair(k, dev) for k in range(len(ids))]
        r1 = [padded(a) for a, _ in rp]; r2 = [padded(b) for _, b in rp]
        m1 = [int(a.shape[1]) for a, _ in rp]; m2 = [int(b.shape[1]) for _, b in rp]
        f1 = [(b.data_ptr(), n, b.shape[1]) for b, n in zip(r1, m1)]; f2 = [(b.data_ptr(), n, b.shape[1]) for b, n in zip(r2, m2)]
        out_r = torch.zeros_like(out)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(2):
                ctx.solve_batch_device(f1, f2, p_plain, out_r.data_ptr())
            ctx.sync()
            t0 = time.perf_counter(); nrep_r = max(args.steps, 5)
            for _ in range(nrep_r):
                ctx.solve_batch_device(f1, f2, p_plain, out_r.data_ptr())
            ctx.sync()
            r_ms = (time.perf_counter() - t0) / nrep_r * 1e3
            s_acc = s_kf = s_gn = 0.0; s_l = 0
            for _ in range(3):
                ctx.solve_batch_device(f1, f2, p_timed, out_r.data_ptr())
                t = ctx.last_timing()
                s_acc += t["accumulate_ms"]; s_kf += t["keyframe_ms"]; s_gn += t["gn_loop_ms"]; s_l += t["accumulate_launches"]
        pts_real = float(np.mean(m1) + np.mean(m2)) / 2; pts_syn = float(np.mean(n1) + np.mean(n2)) / 2
        # The real batch alternates 65 536-row and 131 072-row scans (mean 98 k rows against the synthetic batch's 116 k), and a sixth of a step is spent in kernels that run
        # one block per PAIR whatever its size: part of "slower per point" is the size mix, not the data.  The synthetic points cut to the same mix (every even pair's scans
        # truncated to the real even pairs' share of the odd pairs' rows) separate the two.
        cut = [min(n, int(round(n * (m1[0] / m1[1])))) if k % 2 == 0 and len(m1) > 1 else n for k, n in enumerate(n1)]
        cut2 = [min(n, int(round(n * (m2[0] / m2[1])))) if k % 2 == 0 and len(m2) > 1 else n for k, n in enumerate(n2)]
        g1 = [(b.data_ptr(), n, b.shape[1]) for b, n in zip(bufs1, cut)]; g2 = [(b.data_ptr(), n, b.shape[1]) for b, n in zip(bufs2, cut2)]
        with torch.cuda.stream(stream):
            for _ in range(2):
                ctx.solve_batch_device(g1, g2, p_plain, out_r.data_ptr())
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(nrep_r):
                ctx.solve_batch_device(g1, g2, p_plain, out_r.data_ptr())
            ctx.sync()
            mix_ms = (time.perf_counter() - t0) / nrep_r * 1e3
            ctx.solve_batch_device(f1, f2, p_plain, out_r.data_ptr()); ctx.sync()      # (out_r holds the real batch's results again)
        pts_mix = float(np.mean(cut) + np.mean(cut2)) / 2
        real_res = out_r.cpu().numpy()
        sample_batch = {"workload": "%d pairs from the reference's REAL sample scans (even k: frame_804/805, 65 536 rows of which ~5 k exact zeros; odd k: sample_pc_1/2, 131 072 rows), "
                                    "pair k turned by its own small rotation, zero rows kept; one icet_solve_batch_device call per step" % len(ids), "data": "real",
                        "pairs_per_s": round(len(ids) / (r_ms * 1e-3), 1), "ms_per_step": round(r_ms, 4), "points_per_scan_mean": int(pts_real),
                        "keyframe_ms_per_step": round(s_kf / 3, 4), "gn_loop_ms_per_step": round(s_gn / 3, 4), "accumulate_avg_launch_ms": round(s_acc / max(s_l, 1), 5),
                        "ns_per_point": round(r_ms * 1e6 / (len(ids) * pts_real), 3), "synthetic_ns_per_point": round(ms_per_step * 1e6 / (len(ids) * pts_syn), 3),
                        "slowdown_vs_synthetic_at_equal_point_count": round((r_ms / pts_real) / (ms_per_step / pts_syn), 3),
                        "synthetic_same_size_mix": {"points_per_scan_mean": int(pts_mix), "ms_per_step": round(mix_ms, 4), "ns_per_point": round(mix_ms * 1e6 / (len(ids) * pts_mix), 3),
                                                    "note": "the synthetic pairs with every even pair's scans cut to the real batch's small-to-large row ratio: what the size mix alone costs per point"},
                        "slowdown_vs_synthetic_of_the_same_size_mix": round((r_ms / pts_real) / (mix_ms / pts_mix), 3), "all_finite": bool(np.isfinite(real_res).all())}
        real_host = [(rp[k][0].T.cpu().numpy(), rp[k][1].T.cpu().numpy()) for k in (0, 1, 2, 3)]      # for the oracle cross-check in the cpu_baseline leg
        real_X = real_res[:4, :6].copy()
        del r1, r2, rp

    one_ctx = ctx if not (multi and args.full) else icet_amd.Context(dev_ids[0], stream=stream.cuda_stream)
    mark("latency")
    # ---- single-pair latency (configs[1]) on rank 0's first pair -----------------------------------
    lat = None
    if args.full and args.workload == "batch" and not args.no_latency:
        one1, one2 = d1[:1], d2[:1]
        o1 = torch.zeros((1, 48), dtype=torch.float32, device=dev)
        with torch.cuda.stream(stream):
            for _ in range(5):
                one_ctx.solve_batch_device(one1, one2, p_plain, o1.data_ptr())
        torch.cuda.synchronize()
        tl = time.perf_counter(); nrep = 200
        with torch.cuda.stream(stream):
            for _ in range(nrep):
                one_ctx.solve_batch_device(one1, one2, p_plain, o1.data_ptr())
                one_ctx.sync()
        lat_ms = (time.perf_counter() - tl) / nrep * 1e3
        with torch.cuda.stream(stream):
            one_ctx.solve_batch_device(one1, one2, p_timed, o1.data_ptr())
        lt = one_ctx.last_timing()
        lat_X = o1[0].cpu().numpy().copy()
        l_acc = lt["accumulate_ms"] / max(lt["accumulate_launches"], 1)
        lat = {"workload": "configs[1]: single 64-ch pair, 75x24 voxels, 7 iters, inputs resident in HBM", "ms_per_pair": round(lat_ms, 4),
               "n1": n1[0], "n2": n2[0], "speedup_vs_published_35ms": round(PUBLISHED_MS_PER_PAIR / lat_ms, 1), "repetitions": nrep,
               "keyframe_ms": round(lt["keyframe_ms"], 4), "gn_loop_ms": round(lt["gn_loop_ms"], 4), "accumulate_avg_launch_ms": round(l_acc, 5),
               "whole_path_GBs": round((12.0 * n1[0] + 12.0 * n2[0] * iters + 192.0) / (lat_ms * 1e-3) / 1e9, 1)}

    mark("highres")
    # ---- configs[4] (high-resolution sweep) as a sub-record of the default line: one 128-channel pair, 150 x 48 voxels, 10 iterations ----
    hires = None
    if args.full and args.workload == "batch" and not args.no_latency and rank == 0:
        h1, h2, _ = lidar_sim.make_pair(9000, 9001, lidar_sim.DEFAULT_MOTION, 128, 4096, device=dev, order=args.order)
        hb1, hb2 = padded(h1), padded(h2)
        hd1 = [(hb1.data_ptr(), int(h1.shape[1]), hb1.shape[1])]; hd2 = [(hb2.data_ptr(), int(h2.shape[1]), hb2.shape[1])]
        hp = api.Params(10, 48, 150, 25, 0.1, 0.1, 0); hpt = api.Params(10, 48, 150, 25, 0.1, 0.1, api.FLAG_TIMING)
        ho = torch.zeros((1, 48), dtype=torch.float32, device=dev)
        with torch.cuda.stream(stream):
            for _ in range(5):
                one_ctx.solve_batch_device(hd1, hd2, hp, ho.data_ptr())
        torch.cuda.synchronize()
        th = time.perf_counter(); nrep = 100
        with torch.cuda.stream(stream):
            for _ in range(nrep):
                one_ctx.solve_batch_device(hd1, hd2, hp, ho.data_ptr())
                one_ctx.sync()
        h_ms = (time.perf_counter() - th) / nrep * 1e3
        with torch.cuda.stream(stream):
            one_ctx.solve_batch_device(hd1, hd2, hpt, ho.data_ptr())
        ht = one_ctx.last_timing()
        hi_X = ho[0].cpu().numpy().copy(); hi_host = (h1.T.cpu().numpy(), h2.T.cpu().numpy())
        h_acc = ht["accumulate_ms"] / max(ht["accumulate_launches"], 1)
        h_bytes = 12.0 * h1.shape[1] + 12.0 * h2.shape[1] * 10 + 192.0
        hires = {"workload": "configs[4]: single 128-ch pair (~%dk pts), 150x48 voxels, 10 iters, inputs resident in HBM" % (int(h2.shape[1]) // 1000),
                 "ms_per_pair": round(h_ms, 4), "n1": int(h1.shape[1]), "n2": int(h2.shape[1]), "repetitions": nrep,
                 "keyframe_ms": round(ht["keyframe_ms"], 4), "gn_loop_ms": round(ht["gn_loop_ms"], 4),
                 "accumulate_avg_launch_ms": round(h_acc, 5), "accumulate_GBs": round(12.0 * h2.shape[1] / (h_acc * 1e-3) / 1e9, 1) if h_acc > 0 else None,
                 "whole_path_GBs": round(h_bytes / (h_ms * 1e-3) / 1e9, 1)}
        del hb1, hb2, h1, h2

    mark("h2d_inclusive")
    # ---- PCIe-inclusive ("reported both with and without H2D"): 64 pairs through icet_solve_batch, host pointers in,
    # host results out -- from pageable numpy arrays and from pinned torch tensors.  Never `value`. ----
    h2d = None
    if args.full and args.workload == "batch" and not args.no_h2d and rank == 0 and not args.no_latency:
        m = min(64, len(ids))
        # pageable host arrays in the layout the reference's callers hold (Eigen::MatrixXf: column-major N x 3), so nothing is transposed on the way in
        hs1 = [scans1[j].cpu().contiguous() for j in range(m)]; hs2 = [scans2[j].cpu().contiguous() for j in range(m)]          # (3, N) C-order == column-major N x 3
        a1 = [t.numpy().T for t in hs1]; a2 = [t.numpy().T for t in hs2]                                                        # N x 3 views in Fortran order
        hctx = icet_amd.Context(dev_ids[0])
        def timed(fn, nrep=5):                                  # median of 5: one call delayed by the host (page locking, scheduling) must not set the figure
            fn()
            ts = []
            for _ in range(nrep):
                t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
            return float(np.median(ts))
        t_page = timed(lambda: hctx.solve_batch(a1, a2, iters, None, P, T))
        # pinned: the column-major staging the ABI reads, in page-locked memory (api.solve_batch transposes into pageable buffers, so go through the raw entry)
        import ctypes as C
        pin1 = [s.pin_memory() for s in hs1]; pin2 = [s.pin_memory() for s in hs2]                                               # (3, N) = column-major N x 3
        L = api.load_library()
        A1 = (C.c_void_p * m)(*[t.data_ptr() for t in pin1]); A2 = (C.c_void_p * m)(*[t.data_ptr() for t in pin2])
        nn1 = np.array([t.shape[1] for t in pin1], np.int64); nn2 = np.array([t.shape[1] for t in pin2], np.int64)
        Xo = np.zeros((m, 6), np.float32); Po = np.zeros((m, 6), np.float32); Co = np.zeros((m, 36), np.float32)
        pp = api.Params(iters, P, T, 25, 0.1, 0.1, 0)
        def pinned_call():
            st = L.icet_solve_batch(hctx._h, C.byref(pp), m, A1, nn1.ctypes.data, A2, nn2.ctypes.data, None, Xo.ctypes.data, Po.ctypes.data, Co.ctypes.data)
            if st != 0:
                raise RuntimeError("icet_solve_batch -> %d" % st)
        t_pin = timed(pinned_call)
        mb = sum(12.0 * (a.shape[0] + b.shape[0]) for a, b in zip(a1, a2)) / 1e6
        h2d = {"workload": "%d pairs through icet_solve_batch: host pointers in (H2D of both scans), X / pred_stds / cov back on the host" % m,
               "pageable_ms_per_pair": round(t_page / m * 1e3, 4), "pageable_pairs_per_s": round(m / t_page, 1),
               "pinned_ms_per_pair": round(t_pin / m * 1e3, 4), "pinned_pairs_per_s": round(m / t_pin, 1),
               "host_MB_per_call": round(mb, 1), "pinned_h2d_GBs": round(mb / 1e3 / t_pin, 2),
               "note": "PCIe-inclusive; never `value` (value = inputs resident in HBM). Host arrays are column-major N x 3 (an Eigen::MatrixXf); "
                       "scan 2s are uploaded on a copy stream beside the keyframe build"}
        hctx.close()

    mark("ctor")
    # ---- the constructor path (what src/odometry.cpp:73-79 pays per frame): ONE 64-ch pair from PAGEABLE host memory through icet_solve with the
    # side tables include/icet.h asks for, and the same through the compiled adapter (tests/cpp/adapter_demo.cpp against the Eigen-API mock) ----
    ctor = None
    if args.full and args.workload == "batch" and not args.no_h2d and rank == 0 and not args.no_latency:
        import ctypes as C
        L = api.load_library()
        cctx = icet_amd.Context(dev_ids[0])
        c1 = scans1[0].cpu().contiguous().numpy(); c2 = scans2[0].cpu().contiguous().numpy()      # (3, N): column-major N x 3, pageable
        V = T * P
        tabs = dict(cluster_bounds=np.zeros((V, 6), np.float32), has_fit=np.zeros(V, np.int32), mu1=np.zeros((V, 3), np.float32), sigma1=np.zeros((V, 9), np.float32),
                    evecs1=np.zeros((V, 9), np.float32), l_diag=np.zeros((V, 3), np.float32), x_hist=np.zeros((iters, 6), np.float32), htwh=np.zeros((iters, 36), np.float32),
                    htwdz=np.zeros((iters, 6), np.float32), test_points=np.zeros((V, 18), np.float32), points2=np.zeros((3, c2.shape[1]), np.float32))
        ax = api.Aux()
        for k2, v2 in tabs.items():
            setattr(ax, k2, v2.ctypes.data_as(api._I if v2.dtype == np.int32 else api._F))
        cp = api.Params(iters, P, T, 25, 0.1, 0.1, 0)
        x0 = np.zeros(6, np.float32); Xc = np.zeros(6, np.float32); Pc = np.zeros(6, np.float32); Cc = np.zeros(36, np.float32)
        def ctor_call(aux):
            st = L.icet_solve(cctx._h, C.byref(cp), c1.ctypes.data, c1.shape[1], c1.shape[1], c2.ctypes.data, c2.shape[1], c2.shape[1],
                              x0.ctypes.data, Xc.ctypes.data, Pc.ctypes.data, Cc.ctypes.data, C.byref(ax) if aux else None)
            if st != 0:
                raise RuntimeError("icet_solve -> %d" % st)
        def timed_ms(fn, nrep=100):
            for _ in range(5):
                fn()
            ts = []
            for _ in range(nrep):
                t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.mean(ts)), float(np.median(ts))
        full_mean, full_med = timed_ms(lambda: ctor_call(True))
        bare_mean, bare_med = timed_ms(lambda: ctor_call(False))
        keep = ax.points2; ax.points2 = None
        _, nop2_med = timed_ms(lambda: ctor_call(True))
        ax.points2 = keep
        res1 = torch.zeros((1, 48), dtype=torch.float32, device=dev)
        with torch.cuda.stream(stream):
            one_ctx.solve_batch_device(d1[:1], d2[:1], p_plain, res1.data_ptr()); one_ctx.sync()
        same = bool(np.array_equal(Xc, res1[0, :6].cpu().numpy()))
        ctor = {"workload": "configs[1] through the drop-in boundary: one 64-ch pair in PAGEABLE host memory (column-major N x 3, as an Eigen::MatrixXf) -> icet_solve -> X, pred_stds, cov "
                            "and the side tables include/icet.h requests (clusterBounds, mu1/sigma1/U/L tables, testPoints, HTWH_i, points2) back on the host",
                "ms_per_pair": round(full_med, 4), "mean_ms": round(full_mean, 4), "x_and_pred_stds_only_ms": round(bare_med, 4), "all_tables_but_points2_ms": round(nop2_med, 4),
                "statistic": "median of 100 calls (the mean is reported beside it: a host hiccup in one call moves it)",
                "resident_ms_for_scale": None if lat is None else lat["ms_per_pair"], "bits_equal_device_resident_solve": same,
                "host_MB_in": round(12.0 * (c1.shape[1] + c2.shape[1]) / 1e6, 2)}
        # the compiled adapter: class ICET of include/icet.h constructed from Eigen-API matrices in a timing loop
        try:
            import subprocess, tempfile
            td = tempfile.mkdtemp(prefix="icet_ctor_")
            c1.tofile(os.path.join(td, "s1.f32")); c2.tofile(os.path.join(td, "s2.f32"))
            exe = os.path.join(td, "adapter_demo")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I", os.path.join(ROOT, "include"),
                                   os.path.join(ROOT, "tests", "cpp", "adapter_demo.cpp"), "-L", os.path.join(ROOT, "icet_amd", "lib"), "-licet_hip",
                                   "-Wl,-rpath," + os.path.join(ROOT, "icet_amd", "lib"), "-o", exe], stderr=subprocess.DEVNULL)
            o = subprocess.run([exe, os.path.join(td, "s1.f32"), os.path.join(td, "s2.f32"), str(c1.shape[1]), str(c2.shape[1]), "100"], capture_output=True, text=True, timeout=300)
            tl2 = [ln for ln in o.stdout.splitlines() if ln.startswith("ctor_timing")]
            if o.returncode == 0 and tl2:
                f = tl2[-1].split()
                ctor["adapter_class_ICET_ms"] = float(f[4]); ctor["adapter_class_ICET_median_ms"] = float(f[6])
                ctor["adapter_note"] = "tests/cpp/adapter_demo.cpp: `ICET it(prev, cur, 7, X0, 24, 75)` of include/icet.h against the Eigen-API mock, 100 constructions, a separate process"
            else:
                ctor["adapter_class_ICET_ms"] = None; ctor["adapter_note"] = "adapter_demo failed: rc %d %s" % (o.returncode, o.stderr[-200:])
        except Exception as e:
            ctor["adapter_class_ICET_ms"] = None; ctor["adapter_note"] = "adapter_demo not run: %s" % type(e).__name__
        cctx.close()

    mark("cpu_baseline")
    # ---- CPU baseline: the oracle ("port") on this box's host cores, bounded sample, rank 0 at N=1 -----
    cpu = None
    if args.full and rank == 0 and n_gpus == 1 and not args.no_cpu_baseline:
        from oracle import pyoracle as po
        cores = min(os.cpu_count() or 1, 16)
        m = min(len(ids), args.cpu_sample_pairs if args.workload == "batch" else 1)
        h1 = [scans1[j].T.cpu().numpy() for j in range(m)]; h2 = [scans2[j].T.cpu().numpy() for j in range(m)]
        po.solve_batch(h1[:1], h2[:1], runlen=iters, bins_phi=P, bins_theta=T, n_threads=1)      # warm-up / page-in
        tc = time.perf_counter()
        ref = po.solve_batch(h1, h2, runlen=iters, bins_phi=P, bins_theta=T, n_threads=cores)
        tc = time.perf_counter() - tc
        # the same sample in the oracle's LITERAL mode (glibc float trig, sequential float sums: the expression types of the reference source)
        tl = time.perf_counter()
        ref_lit = po.solve_batch(h1, h2, runlen=iters, bins_phi=P, bins_theta=T, n_threads=cores, mode=po.LIBMF)
        tl = time.perf_counter() - tl
        sec1, _ = po.time_pair(h1[0], h2[0], reps=3, runlen=iters, bins_phi=P, bins_theta=T)
        sec1l, _ = po.time_pair(h1[0], h2[0], reps=3, runlen=iters, bins_phi=P, bins_theta=T, mode=po.LIBMF)
        sec4, _ = po.time_pair(h1[0], h2[0], reps=3, runlen=iters, bins_phi=P, bins_theta=T, mode=po.POOL4)   # parallelFitCells2 structure, 4 workers (src/icet.cpp:31,346-370)
        sec4l, _ = po.time_pair(h1[0], h2[0], reps=3, runlen=iters, bins_phi=P, bins_theta=T, mode=po.POOL4 | po.LIBMF)
        dXp = np.abs(ref["X"] - res[:m, :6].cpu().numpy())
        over1 = np.nonzero((dXp[:, :3].max(1) > 1e-4) | (dXp[:, 3:].max(1) > 1e-5))[0]
        over3 = np.nonzero((dXp[:, :3].max(1) > 3e-4) | (dXp[:, 3:].max(1) > 1e-4))[0]
        # ... and against the oracle's LITERAL mode, the closest thing to the reference binary that exists here (review r4, item 2): no bound is
        # asserted on these -- the two modes of the SAME oracle differ by this much from each other (eigenvector signs turning on last bits)
        def _dstats(A, B):
            d = np.abs(A - B); dt_, dr_ = d[:, :3].max(1), d[:, 3:].max(1)
            big = np.nonzero((dt_ > 3e-4) | (dr_ > 1e-4))[0]
            return {"median_abs_dX_t_m": float(np.median(dt_)), "p99_abs_dX_t_m": float(np.percentile(dt_, 99)), "max_abs_dX_t_m": float(dt_.max()),
                    "median_abs_dX_r_rad": float(np.median(dr_)), "p99_abs_dX_r_rad": float(np.percentile(dr_, 99)), "max_abs_dX_r_rad": float(dr_.max()),
                    "pairs_over_3e-4_m_or_1e-4_rad": int(big.size), "pair_ids_over_3e-4_m_or_1e-4_rad": [int(k) for k in big]}
        gpu_X = res[:m, :6].cpu().numpy()
        vs_literal = {"gpu_vs_literal_oracle": _dstats(gpu_X, ref_lit["X"]), "shared_rule_oracle_vs_literal_oracle": _dstats(ref["X"], ref_lit["X"]),
                      "gpu_vs_shared_rule_oracle": _dstats(gpu_X, ref["X"]),
                      "note": "literal = glibc float atan2/acos/sin/cos, sequential float sums, std::hypot (src/utils.cpp:103-108,134-136; Eigen's float sums src/icet.cpp:160-162); "
                              "shared rule = correctly rounded transcendentals + exact sums on BOTH sides (what the parity tests hold the device to)"}
        # the two single-pair sub-records against the unmodified oracle on their own inputs (informational here; asserted in tests/test_gpu_parity.py)
        if lat is not None:
            r1 = po.solve(h1[0], h2[0], runlen=iters, bins_phi=P, bins_theta=T)
            lat["max_abs_dX_vs_oracle"] = float(np.abs(r1["X"] - lat_X[:6]).max()); lat["max_rel_pred_stds_vs_oracle"] = float(np.abs(lat_X[6:12] / r1["pred_stds"] - 1).max())
        if hires is not None:
            r5 = po.solve(hi_host[0], hi_host[1], runlen=10, bins_phi=48, bins_theta=150)
            hires["max_abs_dX_vs_oracle"] = float(np.abs(r5["X"] - hi_X[:6]).max()); hires["max_rel_pred_stds_vs_oracle"] = float(np.abs(hi_X[6:12] / r5["pred_stds"] - 1).max())
        if sample_batch is not None:
            dxr = [float(np.abs(po.solve(a_, b_, runlen=iters, bins_phi=P, bins_theta=T)["X"] - real_X[i_]).max()) for i_, (a_, b_) in enumerate(real_host)]
            sample_batch["max_abs_dX_vs_oracle_first_4_pairs"] = max(dxr)
        cpu = {"value": round(m / tl, 3), "unit": "scan-pairs/s", "cores": cores, "kind": "port",
               "sample": "first %d pairs of the same batch, one pair per host thread (oracle/icet_oracle.cpp, -O3 -march=native) in the oracle's LITERAL mode "
                         "(glibc float atan2/acos/sin/cos, sequential float sums -- the reference's expression types), %.1f s wall" % (m, tl),
               "literal_mode": {"pairs_per_s": round(m / tl, 3), "single_thread_ms_per_pair": round(sec1l * 1e3, 2), "threadpool4_ms_per_pair": round(sec4l * 1e3, 2)},
               "shared_rule_mode": {"pairs_per_s": round(m / tc, 3), "single_thread_ms_per_pair": round(sec1 * 1e3, 2), "threadpool4_ms_per_pair": round(sec4 * 1e3, 2),
                                    "note": "correctly rounded transcendentals + exact sums: the mode the parity tests compare the device with (%.1f s wall)" % tc},
               "single_thread_ms_per_pair": round(sec1l * 1e3, 2), "threadpool4_ms_per_pair": round(sec4l * 1e3, 2),
               # cross-check against the UNMODIFIED oracle (shared rule, natural eigenvector signs, nothing borrowed from the device); the parity
               # tests proper are tests/test_gpu_parity.py (keyframe bit-exact, X within 2e-4 m / 2e-5 rad on every pair but the one asserted exception)
               "median_abs_dX_vs_gpu_on_sample": float(np.median(dXp.max(1))), "max_abs_dX_vs_gpu_on_sample": float(dXp.max()),
               "pairs_over_1e-4_m_or_1e-5_rad_natural_signs": int(over1.size), "pairs_over_3e-4_m_or_1e-4_rad_natural_signs": int(over3.size),
               "pair_ids_over_3e-4_m_or_1e-4_rad": [int(k) for k in over3], "vs_literal_mode": vs_literal}

    mark("sample")
    # ---- configs[0] with a number, and the first non-synthetic figures: the reference's own sample pairs (src/sample_data/frame_804/805.npy,
    # python/point_clouds/sample_pc_1/2.npy, committed as float32 fixtures) through the GPU path and through the oracle on the host (literal mode:
    # serial loop = the live path of src/icet.cpp:391-404, and the 4-worker ThreadPool structure of :346-370), as src/icet_cpp_demo.cpp:25-45 runs them ----
    sample = None
    if args.full and rank == 0 and n_gpus == 1 and not args.no_cpu_baseline and args.workload == "batch":
        from oracle import pyoracle as po
        sample = {"workload": "configs[0]: the reference's sample scan pairs (real lidar data), 75x24 voxels, 7 iters, X0 = 0; GPU: icet_solve from pageable host memory "
                              "(PCIe-inclusive) and device-resident; CPU: oracle in its literal mode, serial and ThreadPool-4", "data": "real", "pairs": {}}
        sctx = icet_amd.Context(dev_ids[0])
        for name in ("frame_804_805", "sample_pc_1_2"):
            fx = np.load(os.path.join(ROOT, "tests", "golden", "scans_%s.npz" % name))
            a, b = fx["scan1"], fx["scan2"]                                   # N x 3 float32
            ac, bc = np.ascontiguousarray(a.T).T, np.ascontiguousarray(b.T).T   # column-major N x 3 (an Eigen::MatrixXf)
            r = sctx.solve(ac, bc, iters, np.zeros(6), P, T)
            t0 = time.perf_counter(); nrep = 50
            for _ in range(nrep):
                r = sctx.solve(ac, bc, iters, np.zeros(6), P, T)
            host_ms = (time.perf_counter() - t0) / nrep * 1e3
            ta = torch.from_numpy(np.ascontiguousarray(a.T)).to(dev); tb = torch.from_numpy(np.ascontiguousarray(b.T)).to(dev)
            pa, pb = padded(ta), padded(tb)
            so = torch.zeros((1, 48), dtype=torch.float32, device=dev)
            sd1 = [(pa.data_ptr(), a.shape[0], pa.shape[1])]; sd2 = [(pb.data_ptr(), b.shape[0], pb.shape[1])]
            with torch.cuda.stream(stream):
                for _ in range(5):
                    one_ctx.solve_batch_device(sd1, sd2, p_plain, so.data_ptr())
                one_ctx.sync()
                t0 = time.perf_counter()
                for _ in range(nrep):
                    one_ctx.solve_batch_device(sd1, sd2, p_plain, so.data_ptr()); one_ctx.sync()
                res_ms = (time.perf_counter() - t0) / nrep * 1e3
            o_ref = po.solve(a, b, runlen=iters, bins_phi=P, bins_theta=T)
            ser, _ = po.time_pair(a, b, reps=3, runlen=iters, bins_phi=P, bins_theta=T, mode=po.LIBMF)
            pool, _ = po.time_pair(a, b, reps=3, runlen=iters, bins_phi=P, bins_theta=T, mode=po.POOL4 | po.LIBMF)
            sample["pairs"][name] = {"points": [int(a.shape[0]), int(b.shape[0])], "gpu_resident_ms": round(res_ms, 4), "gpu_from_host_memory_ms": round(host_ms, 4),
                                     "cpu_serial_literal_ms": round(ser * 1e3, 2), "cpu_threadpool4_literal_ms": round(pool * 1e3, 2),
                                     "speedup_resident_vs_cpu_serial": round(ser * 1e3 / res_ms, 1),
                                     "X_gpu": [round(float(v), 6) for v in r["X"]], "max_abs_dX_vs_oracle": float(np.abs(r["X"] - o_ref["X"]).max()),
                                     "bits_equal_resident_and_host_path": bool(np.array_equal(so[0, :6].cpu().numpy(), r["X"]))}
        sctx.close()

    mark("end")
    if rank == 0:
        line = {
            "metric": "scan-pairs/sec + ms/pair, 64-ch 75x24 voxels 7 iters; HBM GB/s vs peak" if args.workload in ("batch", "sample") else "scan-pairs/sec, 128-ch 150x48 voxels 10 iters",
            "value": round(pairs_per_s, 2), "unit": "scan-pairs/s", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "ms_per_pair": round(ms_per_step / max(n_local, 1), 5),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "real (the reference's two sample pairs, rotated per pair)" if args.workload == "sample" else "synthetic",
            "timed_region": {"seconds": round(dt, 4), "repetitions_of_the_K_steps": reps_t, "steps_timed": steps_total,
                             "ms_per_step_min": round(min(rep_ms), 4), "ms_per_step_max": round(max(rep_ms), 4)},
            "config": {"workload": ("configs[2]/[3]: %d independent 64-ch synthetic scan pairs per GPU (~%dk pts/scan, %s-major), 75x24 voxels, 7 iters, "
                                    "pair k -> %s k mod N, %s" % (n_local, int(np.mean(n2) / 1000), args.order, "device" if multi else "rank",
                                                                  ("one process: icet_multi_solve_batch_device, %s gather" % args.multi_gather) if multi
                                                                  else "RCCL all-gather of 48 floats/pair when N>1"))
                       if args.workload == "batch" else ("%d pairs built from the reference's REAL sample scans (frame_804/805: 65 k rows with ~5 k exact-zero rows; sample_pc_1/2: 131 k rows), pair k rotated by its own small rigid motion, 75x24 voxels, 7 iters" % n_local
                                                         if args.workload == "sample" else "configs[4]: single 128-ch pair (~%dk pts), 150x48 voxels, 10 iters" % int(np.mean(n2) / 1000)),
                       **({"options": list(args.set)} if args.set else {}), **({"flags": args.flags} if args.flags else {}),
                       "pairs_per_gpu": n_local, "pairs_total": n_global, "points_scan1_mean": int(np.mean(n1)), "points_scan2_mean": int(np.mean(n2)),
                       "bins_theta": T, "bins_phi": P, "iters": iters, "parallelism": "pairs round-robin x%d" % n_gpus,
                       "processes": 1 if multi else world, "mode": "multi (one process)" if multi else "one process per GPU",
                       "rccl_ranks": (dist.get_world_size() if (world > 1 and backend == "nccl") else (args.gpus if (multi and args.multi_gather == "rccl") else 0)),
                       "devices": dev_ids if multi else list(range(world)), "gather_ms": None if gather_ms is None else round(gather_ms, 4),
                       "collective": collective_note or ("rccl" if (world > 1 and backend == "nccl") else (backend if world > 1 else None)),
                       "gen_s": round(t_gen, 1)},
            "roofline": {"kernel": "k_gn_accumulate", "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_note,
                         "algorithmic_bytes_per_launch": bytes_per_launch, "avg_launch_ms": round(acc_launch_ms, 5), "launches_timed": launches,
                         "whole_path_GBs": round(bytes_path / (ms_per_step * 1e-3) / 1e9, 1),
                         "whole_path_frac": round(bytes_path / (ms_per_step * 1e-3) / 1e9 / (HBM_PEAK_GBS * n_gpus), 4),      # B_pair x pairs / t / peak (frac above is the dominant kernel alone)
                         "keyframe_ms_per_step": round(kf_ms / reps, 4), "gn_loop_ms_per_step": round(gn_ms / reps, 4)} if args.full else None,
            "cpu_baseline": cpu,
            "latency": lat,
            "highres": hires,
            "other_storage_order": az_major,
            "sample_batch": sample_batch,
            "h2d_inclusive": h2d,
            "ctor": ctor,
            "sample": sample,
            "published_reference_ms_per_pair": PUBLISHED_MS_PER_PAIR,
            "wall_s_by_phase": walls,
        }
        print(json.dumps(line), flush=True)
    # `--gpus N` measures N ranks gathering over RCCL or says loudly that it did not: a line whose gather fell back to gloo is printed (for the record) and the run FAILS
    # (review r5, next 7).  Only the explicit rehearsal switch ICET_BENCH_BACKEND=gloo (N ranks on one card) is exempt.
    rccl_missing = world > 1 and not multi and backend != "nccl" and os.environ.get("ICET_BENCH_BACKEND", "nccl") == "nccl"
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rccl_missing:
        sys.stderr.write("bench.py: --gpus %d asked for one rank per GPU over RCCL, but the gather ran on gloo (%s): exit code 3\n" % (args.gpus, collective_note))
        if multi: one_ctx.close(); mctx.close()
        else: ctx.close()
        return 3
    if multi:
        one_ctx.close(); mctx.close()
    else:
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
