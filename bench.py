#!/usr/bin/env python3
"""Benchmark: device-resident batched Internet checksums (µC/TCP-IP net_util.c path) on MI355X.

BASELINE.json metric: "GiB/s checksummed, device-resident, batched 1500 B TCP segments @1/2/4/8 GPU".
Workload at N=1 (configs[1], "C2"): 1 048 576 uniform 1500-B TCP segments + one 12-B IPv4 pseudo-
header each, resident in HBM; one STEP = one NetUtil_MI355X_ChkSumBatchStrided launch producing
all 1 M DataCalc checksums. At N>1 (configs[4], "C5"): each rank owns a 16 M-segment shard of the
global 128 M x 1500 B batch (contiguous index ranges), one launch per step. Weak
scaling: distinct bytes per rank, no collective on the data path; the only communication is the
barrier and the max-over-ranks of the timed region.

Clock ramp: the first ~100 launches after an idle gap run up to 25 % slower, so before
the W counted warm-up steps the step is repeated untimed for --ramp-seconds (default 0.5 s).

value     = Σ_ranks n_seg*(1500+12) bytes * steps / max_rank(wall time of the K timed steps) / 2^30
roofline  = dominant kernel (the form the library picks for C2: seg_stream_kernel) algorithmic bytes
            per launch n_seg*(1500+12+2) / mean HIP-event duration of that launch on its stream, vs the
            8.0 TB/s HBM3E spec peak; `traffic` = HBM bytes per launch from rocprofv3 PMC,
            FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE: measured live at N=1 (--pmc live: two
            rocprofv3 --pmc passes over a short child run of this bench at the same size), else
            from the committed profiles/*pmc*.json whose kernel form and source hash match, or null.
cpu_baseline = the oracle's restatement of the reference C path (gcc -O2, same per-segment
            NetUtil_16BitOnesCplChkSumDataCalc call on a one-buffer NET_BUF) timed on this host's
            cores on a bounded sample of the same workload (rank 0, N=1 only).

A plain run sets up, ramps, warms up, times the K steps and prints `value` with the run's configuration.
`roofline`, `cpu_baseline` and every other figure or check beside the headline (the parity sample
against the oracle, the read probes, the C5 shard point, the C1 per-datagram figures, the per-rank
records at N > 1) take runs of their own after the timed region and are made only with --full.
--dump-outputs DIR writes the checksums of the last timed step to DIR/checksums.npy (float32).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]   (torchrun for N>1)
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
# CPU baseline: the OpenMP workers are pinned (OMP_PROC_BIND=close over cores); set
# before torch loads libgomp, which reads them once. Single-rank runs only (the baseline is rank 0 at
# N = 1; ranks of an N > 1 run would pin their threads onto the same cores).
_OMP_PINNED_HERE = []
if os.environ.get("WORLD_SIZE", "1") == "1":
    for _k, _v in (("OMP_PROC_BIND", "close"), ("OMP_PLACES", "cores")):
        if _k not in os.environ:
            os.environ[_k] = _v
            _OMP_PINNED_HERE.append(_k)
sys.path.insert(0, os.path.join(REPO, "uc-tcp-ip_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

METRIC = "GiB/s checksummed, device-resident, batched 1500 B TCP segments @1/2/4/8 GPU"
HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)
SEED = 0x5EED0001


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--segments", type=int, default=None,
                    help="segments per GPU (default: C2's 1 M at N=1, C5's 16 M shard at N>1)")
    ap.add_argument("--ramp-seconds", type=float, default=0.5,
                    help="untimed clock-ramp phase before the counted warm-up (same launch)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline: the event-timed roofline pass, "
                         "the read probes, roofline.traffic (PMC), the parity sample against the oracle, the C5 "
                         "shard point, the CPU baseline and the C1 per-datagram figures (a plain run only sets up, "
                         "warms up, times the K steps and prints the headline line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the checksums of the last timed step to DIR/<name>.npy "
                         "(float32; a fixed seeded sample, with its indices, of a batch above 1 Mi segments)")
    ap.add_argument("--seg-len", type=int, default=1500)
    ap.add_argument("--pseudo-len", type=int, default=12)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=2.0, help="wall seconds of the CPU sample")
    ap.add_argument("--traffic-json", default=None, help="PMC summary (default: newest profiles/*pmc*.json)")
    ap.add_argument("--pmc", choices=["live", "file", "off"], default="live",
                    help="roofline.traffic source: live rocprofv3 --pmc passes over a child run (rank 0, N=1; "
                         "falls back to the committed summaries), committed file only, or none")
    ap.add_argument("--tune", action="append", default=[], help="key=value launch tuning (grid/group/nt/block/kernel/chunks/tile/mult/xcd/touch/waves)")
    ap.add_argument("--no-c5-point", action="store_true",
                    help="N=1: skip the same-workload retention point (the C5 16 M-segment shard on this GPU)")
    # below the driver's own 600-s limit on a bench run, so that a hung rank is named by the launcher
    # (with its last stage marker) before the driver kills the whole run
    ap.add_argument("--launch-timeout", type=float, default=540.0,
                    help="launcher (--gpus N > 1 without WORLD_SIZE): seconds before the rank processes are killed")
    # CPU test of the launcher only: each rank prints its rendezvous environment and exits before any
    # torch import ("ok"), rank 1 exits 3 ("fail1"), or rank 1 stops after its "process group up" marker
    # while rank 0 waits in the timed region's closing barrier ("hang1"); tests/test_bench_launch_cpu.py
    ap.add_argument("--launcher-selftest", choices=["ok", "fail1", "hang1"], default=None, help=argparse.SUPPRESS)
    return ap.parse_args()


RANK_ENV = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")
STAGE_TAG = "bench-stage"
STAGES = ("start", "torch imported", "process group up", "shard generated", "warm-up done", "timed region done",
          "reported")
_T_START = time.monotonic()


def stage(name):
    """A rank's progress marker on stderr (one line, flushed): the launcher names the last one a hung or
    failed rank reached. Stages: start, torch imported, process group up, shard generated, warm-up
    done, timed region done, reported."""
    print(f"{STAGE_TAG} rank={os.environ.get('RANK', '0')} stage={name} t={time.monotonic() - _T_START:.1f}s",
          file=sys.stderr, flush=True)


def parse_stage(line):
    """(rank, stage) of a stage-marker line, else None."""
    if not line.startswith(STAGE_TAG + " "):
        return None
    f = dict(kv.split("=", 1) for kv in line[len(STAGE_TAG) + 1:].split(" ") if "=" in kv)
    rest = line.split(" stage=", 1)[1].rsplit(" t=", 1)[0] if " stage=" in line else None
    return (int(f["rank"]), rest) if "rank" in f and rest else None


def rank_environments(n, port, base=None):
    """The environment of each of the N rank processes the launcher starts: one rank per GPU of this
    node, rendezvous over 127.0.0.1 (torch.distributed env:// reads these six variables)."""
    base = dict(os.environ if base is None else base)
    for k in _OMP_PINNED_HERE:                      # the CPU-baseline pinning is for a single rank only
        base.pop(k, None)
    envs = []
    for r in range(n):
        e = dict(base)
        e.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                  "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
        envs.append(e)
    return envs


def world_check(gpus, env=None):
    """--gpus N against the rank environment: returns "launch" (no WORLD_SIZE and N > 1: this process
    starts the N ranks), "rank" (run as one rank) or raises SystemExit(2) when an externally launched
    world (torchrun) disagrees with --gpus — the run would otherwise measure a different N than asked."""
    env = os.environ if env is None else env
    if gpus < 1:
        raise SystemExit(f"bench.py: --gpus {gpus} must be >= 1")
    ws = env.get("WORLD_SIZE")
    if ws is None:
        return "launch" if gpus > 1 else "rank"
    if int(ws) != gpus:
        print(f"bench.py: WORLD_SIZE={ws} but --gpus {gpus}: refusing to measure a different world size than "
              f"asked", file=sys.stderr, flush=True)
        raise SystemExit(2)
    return "rank"


def launch_ranks(args):
    """--gpus N > 1 with no WORLD_SIZE: start N fresh rank processes of this script (one per GPU),
    wait for all of them, print rank 0's JSON line and return non-zero if any rank failed or timed out.
    This process never touches the GPU (no torch import): the ranks own the devices."""
    import signal
    import socket
    import subprocess
    import tempfile
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    argv = [sys.executable, "-u", os.path.abspath(__file__)] + sys.argv[1:]
    procs, outs, errs = [], [], []
    t0 = time.monotonic()
    last = {}                                    # rank -> (stage, monotonic time the marker arrived)
    for r, env in enumerate(rank_environments(args.gpus, port)):
        f = tempfile.TemporaryFile(mode="w+")
        outs.append(f)
        ef = tempfile.NamedTemporaryFile(mode="w+", delete=False, prefix=f"bench_rank{r}_", suffix=".err")
        errs.append([ef, 0, ""])                 # file, read offset, partial line
        procs.append(subprocess.Popen(argv, env=env, stdout=f, stderr=ef, start_new_session=True))

    def pump():
        """Forward every rank's new stderr lines (live, prefixed) and note its stage markers."""
        for r, e in enumerate(errs):
            with open(e[0].name) as fh:
                fh.seek(e[1])
                chunk = fh.read()
                e[1] = fh.tell()
            text = e[2] + chunk
            lines = text.split("\n")
            e[2] = lines.pop()
            for ln in lines:
                st = parse_stage(ln)
                if st is not None:
                    last[r] = (st[1], time.monotonic())
                print(f"[rank {r}] {ln}", file=sys.stderr, flush=True)

    def stage_report():
        now = time.monotonic()
        return "; ".join(f"rank {r}: " + (f"last stage '{last[r][0]}' ({now - last[r][1]:.0f} s ago)" if r in last
                                          else "no stage marker") + (" [still running]" if rc[r] is None else
                                                                     f" [exit {rc[r]}]")
                         for r in range(len(procs)))

    deadline = t0 + args.launch_timeout
    rc = [None] * len(procs)
    failed = None
    while any(c is None for c in rc):
        pump()
        for r, p in enumerate(procs):
            if rc[r] is None:
                rc[r] = p.poll()
                if rc[r] not in (None, 0) and failed is None:
                    failed = f"rank {r} exited {rc[r]}" + (f" after stage '{last[r][0]}'" if r in last else "")
        if failed or time.monotonic() > deadline:
            if failed is None:
                hung = [r for r in range(len(procs)) if rc[r] is None]
                # the hung rank is the one furthest behind: the earliest stage in STAGES (or no marker at
                # all); ranks ahead of it wait for it in a collective
                order = sorted(hung, key=lambda r: (STAGES.index(last[r][0]) if r in last and last[r][0] in STAGES
                                                    else -1, last[r][1] if r in last else -1.0))
                failed = (f"timeout after {args.launch_timeout:.0f} s: rank {order[0]} hung"
                          + (f" after stage '{last[order[0]][0]}'" if order[0] in last else " before its first stage marker")
                          + f" ({len(hung)} rank(s) still running)")
            report = stage_report()
            for r, p in enumerate(procs):        # end every rank's own process group, nothing else
                if p.poll() is None:
                    try:
                        os.killpg(p.pid, signal.SIGKILL)
                    except ProcessLookupError:
                        pass
            for r, p in enumerate(procs):
                rc[r] = p.wait()
            print(f"bench.py launcher: {report}", file=sys.stderr, flush=True)
            break
        time.sleep(0.05)
    pump()
    for e in errs:
        if e[2]:
            print(e[2], file=sys.stderr, flush=True)
        e[0].close()
        os.unlink(e[0].name)
    line = None
    for r, f in enumerate(outs):
        f.seek(0)
        text = f.read()
        if r == 0:
            lines = [x for x in text.splitlines() if x.startswith("{")]
            line = lines[-1] if lines else None
            rest = [x for x in text.splitlines() if not x.startswith("{")]
            if rest:
                print("\n".join(rest), file=sys.stderr, flush=True)
        elif text.strip():
            print("\n".join(f"[rank {r}] {x}" for x in text.splitlines()), file=sys.stderr, flush=True)
    if failed or any(c != 0 for c in rc):
        print(f"bench.py launcher: {failed or 'a rank failed'}; exit codes {rc}", file=sys.stderr, flush=True)
        return 1
    if line is None:
        print("bench.py launcher: rank 0 printed no JSON line", file=sys.stderr, flush=True)
        return 1
    print(line, flush=True)
    return 0


def launcher_selftest(mode):
    """Rank side of --launcher-selftest: report the rendezvous environment, no torch, no GPU."""
    rank = int(os.environ["RANK"])
    if mode == "fail1" and rank == 1:
        print("selftest: rank 1 fails on purpose", file=sys.stderr, flush=True)
        return 3
    if mode == "hang1":
        stage("process group up")
        if rank == 1:                            # e.g. stuck generating its shard
            time.sleep(3600)
        stage("shard generated")
        stage("warm-up done")
        time.sleep(3600)                         # rank 0: waits in the barrier for rank 1
    print(json.dumps({k: os.environ.get(k) for k in RANK_ENV}), flush=True)
    return 0


def c2_pseudo_headers(start, n, L, plen):
    """IPv4 TCP pseudo-headers (net_tcp.h:1545-1551 layout) for global segments [start, start+n):
    src = 10.x.y.z from the index, dst from a hashed index, zero, protocol 6, big-endian length."""
    import numpy as np
    g = np.arange(start, start + n, dtype=np.uint64)
    h = (g * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    ph = np.zeros((n, 12), np.uint8)
    for b in range(4):
        ph[:, b] = ((g >> np.uint64(8 * (3 - b))) & np.uint64(0xFF)).astype(np.uint8)
        ph[:, 4 + b] = ((h >> np.uint64(8 * (3 - b))) & np.uint64(0xFF)).astype(np.uint8)
    ph[:, 0] |= 0x0A
    ph[:, 9] = 6
    ph[:, 10] = (L >> 8) & 0xFF
    ph[:, 11] = L & 0xFF
    return np.ascontiguousarray(ph[:, :plen]).reshape(-1)


def shard_range(rank, n_per_rank):
    """Weak scaling: rank r owns global segments [r*n, (r+1)*n) of one global synthetic batch."""
    return rank * n_per_rank, n_per_rank


def make_c2_shard(torch, netcsum, start, n, L, plen, dev):
    """Device-resident C2 shard: segment bytes generated ON the device as the slice
    [start*L, (start+n)*L) of the global splitmix64 stream; pseudo-headers from the global index."""
    seg = torch.empty(n * L + 256, dtype=torch.uint8, device=dev)
    netcsum.fill(seg, n * L, SEED, 0, first_byte=start * L)
    ph = torch.from_numpy(c2_pseudo_headers(start, n, L, plen)).to(dev) if plen else None
    torch.cuda.synchronize()
    return seg, ph


def host_c2_shard(oracle, start, n, L, plen):
    """The same shard regenerated on the host (test / parity use)."""
    return oracle.fill(start * L, n * L, SEED, 0), (c2_pseudo_headers(start, n, L, plen) if plen else None)


C5_SHARD = 1 << 24                  # BASELINE configs[4]: 128 M segments over 8 GPUs = 16 M per GPU
DUMP_MAX_SEGMENTS = 1 << 20         # --dump-outputs: checksums written over all ranks (4 MB as float32)


def dump_outputs(torch, path, out, rank, world):
    """--dump-outputs: what the step's caller receives, the n checksums of this rank's shard as the
    last timed step left them in `out`, as float32 (u16 values, exact) in DIR/checksums.npy
    (DIR/checksums_rank<r>.npy at N > 1). A shard above DUMP_MAX_SEGMENTS / N segments is sampled at
    fixed indices (seeded by SEED and the rank, sorted), themselves written to <name>_index.npy (float64),
    so that two builds given the same arguments write arrays that compare element for element."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    name = "checksums" if world == 1 else f"checksums_rank{rank}"
    n, cap = out.numel(), max(1, DUMP_MAX_SEGMENTS // world)
    if n > cap:
        idx = np.sort(np.random.default_rng([SEED, rank]).choice(n, size=cap, replace=False))
        vals = out[torch.from_numpy(idx).to(out.device)].cpu().numpy()
        np.save(os.path.join(path, name + "_index.npy"), idx.astype(np.float64))
    else:
        vals = out.cpu().numpy()
    np.save(os.path.join(path, name + ".npy"), vals.view(np.uint16).astype(np.float32))


def read_probes(torch, netcsum, seg, n16, stream, reps=20):
    """Measured read ceilings over the first n16 bytes of `seg` (HIP events on `stream`, mean of reps
    launches after reps untimed): the LDS-DMA grid-stride probe (TUNE_PROBE 1) and read_run_kernel, the
    checksum kernel's own access pattern with no arithmetic (TUNE_PROBE 2). Returns (lds, run) GB/s."""
    sink = torch.zeros(1, dtype=torch.int64, device=seg.device)
    ms = {}
    for probe in (1, 2):
        netcsum.tune(netcsum.TUNE_PROBE, probe)
        for _ in range(reps):
            netcsum.read_stream(seg, n16, sink, stream=stream)
        rs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in rs:
            a.record(stream)
            netcsum.read_stream(seg, n16, sink, stream=stream)
            b.record(stream)
        torch.cuda.synchronize()
        ms[probe] = sum(a.elapsed_time(b) for a, b in rs) / len(rs)
    netcsum.tune(netcsum.TUNE_PROBE, 1)
    return n16 / (ms[1] * 1e-3) / 1e9, n16 / (ms[2] * 1e-3) / 1e9


# One rank's own measurements at N > 1, all-gathered in this field order (float64 tensor).
RANK_FIELDS = ("rank", "local_rank", "device", "wall_s", "kernel_ms", "per_gpu_GiBps", "run_stream_read_probe_GBps",
               "read_stream_probe_GBps", "frac_of_run_stream_read_probe", "parity_sample_ok")


def rank_records(dist, tensor_dev, own, world):
    """All-gather every rank's `own` record (RANK_FIELDS) over the process group; list in rank order.
    tensor_dev: "cpu" for gloo, the rank's GPU for RCCL."""
    import torch
    t = torch.tensor([float(own[k]) for k in RANK_FIELDS], dtype=torch.float64, device=tensor_dev)
    got = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(got, t)
    return [dict(zip(RANK_FIELDS, x.cpu().tolist())) for x in got]


def rank_summary(recs):
    """The N > 1 line's self-explaining part: each rank's per-GPU rate (its own
    wall time over the K timed launches), event-timed kernel ms and read ceilings over its own shard,
    the slowest and fastest rank, and the spread. The aggregate `value` is set by the slowest rank (max
    over ranks of the wall time), so a slow device is named here by its LOCAL_RANK."""
    per = []
    for r in recs:
        per.append({"rank": int(r["rank"]), "local_rank": int(r["local_rank"]), "device": int(r["device"]),
                    "per_gpu_GiBps": round(r["per_gpu_GiBps"], 2), "wall_s": round(r["wall_s"], 6),
                    "kernel_ms": round(r["kernel_ms"], 5),
                    "run_stream_read_probe_GBps": round(r["run_stream_read_probe_GBps"], 1),
                    "read_stream_probe_GBps": round(r["read_stream_probe_GBps"], 1),
                    "frac_of_run_stream_read_probe": round(r["frac_of_run_stream_read_probe"], 4),
                    "parity_sample_ok": bool(r["parity_sample_ok"])})
    slow = min(per, key=lambda x: x["per_gpu_GiBps"])
    fast = max(per, key=lambda x: x["per_gpu_GiBps"])
    return {"per_rank": per, "min_per_gpu": slow["per_gpu_GiBps"], "max_per_gpu": fast["per_gpu_GiBps"],
            "slowest_rank": slow["rank"], "slowest_local_rank": slow["local_rank"],
            "fastest_rank": fast["rank"], "spread_max_over_min": round(fast["per_gpu_GiBps"] / slow["per_gpu_GiBps"], 4),
            "min_frac_of_run_stream_read_probe": min(x["frac_of_run_stream_read_probe"] for x in per)}


def c5_point(torch, netcsum, args, dev, stream):
    """Same-workload retention denominator, measured at N = 1 OUTSIDE the timed region: the per-GPU
    rate of one C5 shard (16 M x 1500 B + 12 B, rank 0's slice of the global batch) on this GPU, by
    the headline's own method (K launches between two synchronizes, wall clock) and by HIP events on
    the launch stream. The driver's N > 1 runs measure exactly this workload per rank, so
    per-GPU@N / this value is retention on ONE workload (the headline's N = 1 point is C2)."""
    import numpy as np
    L, plen, n = args.seg_len, args.pseudo_len, C5_SHARD
    seg, ph = make_c2_shard(torch, netcsum, 0, n, L, plen, dev)
    out = torch.empty(n, dtype=torch.int16, device=dev)

    def step():
        netcsum.batch_strided(seg, L, L, ph, plen, plen, n, out, netcsum.OP_DATA_CALC, stream=stream)
    t = time.perf_counter()
    while time.perf_counter() - t < 1.0:          # clock ramp, untimed
        step()
        torch.cuda.synchronize()
    k = max(10, min(args.steps, 50))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        step()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]
    for a, b in evs:
        a.record(stream)
        step()
        b.record(stream)
    torch.cuda.synchronize()
    kern_ms = sum(a.elapsed_time(b) for a, b in evs) / k
    parity = None
    try:
        import oracle
        sample = np.sort(np.random.default_rng(5).choice(n, size=64, replace=False))
        sidx = torch.from_numpy(sample).to(dev)
        segs = seg[: n * L].view(n, L)[sidx].cpu().numpy().reshape(-1)
        phs = ph.view(n, plen)[sidx].cpu().numpy().reshape(-1) if plen else None
        want = oracle.batch_strided(segs, L, L, phs, plen, plen, len(sample), 0)
        parity = bool(np.array_equal(out.cpu().numpy().view(np.uint16)[sample], want))
    except Exception as e:                        # noqa: BLE001
        parity = f"unchecked: {e}"
    desc = "netcsum::" + netcsum.last_launch()
    # diagnostic (after the parity check, which reads `out`): the same launches without the pseudo-header stream (a second address stream)
    for a, b in evs:
        a.record(stream)
        netcsum.batch_strided(seg, L, L, None, 0, 0, n, out, netcsum.OP_DATA_CALC, stream=stream)
        b.record(stream)
    torch.cuda.synchronize()
    nop_ms = sum(a.elapsed_time(b) for a, b in evs) / k
    # the read ceilings over the same 25 GB (a box whose C5 rate falls while these
    # hold loses it in the kernel, one whose probes fall with it loses it in the access pattern)
    n16 = (n * L) // 16 * 16
    lds_gbps, run_gbps = read_probes(torch, netcsum, seg, n16, stream)
    del seg, ph, out
    torch.cuda.empty_cache()
    algo = n * (L + plen + 2)
    ach = algo / (kern_ms * 1e-3) / 1e9
    return {"workload": f"C5 shard: {n} x {L} B TCP segments + {plen} B pseudo-header on one GPU "
                        "(rank 0's slice of the 128 M global batch)",
            "value_per_gpu": round(n * (L + plen) * k / wall / 2 ** 30, 2), "unit": "GiB/s",
            "ms_per_step": round(wall / k * 1e3, 4), "steps": k, "kernel": desc,
            "kernel_ms": round(kern_ms, 4), "roofline_frac": round(ach / HBM_PEAK_GBPS, 4),
            "run_stream_read_probe_GBps": round(run_gbps, 1), "frac_of_run_stream_read_probe": round(ach / run_gbps, 4),
            "read_stream_probe_GBps": round(lds_gbps, 1), "frac_of_read_stream_probe": round(ach / lds_gbps, 4),
            "kernel_ms_no_pseudo_headers": round(nop_ms, 4),
            "parity_sample_ok": parity,
            "use": "retention denominator for the driver's N > 1 runs (same workload per GPU)"}


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def _time_cpu(fn, seconds):
    fn()                                             # warm (first touch, thread pool)
    reps, t0 = 0, time.perf_counter()
    while True:
        fn()
        reps += 1
        el = time.perf_counter() - t0
        if el >= seconds:
            return reps, el


def host_cpus():
    """CPUs this process may use: the affinity mask, capped by a cgroup v2 CPU quota and by the
    OMP_NUM_THREADS share the GPU box sets for one GPU (its mask shows every CPU of a shared host;
    running past the share only throttles or starves neighbours). Returns (threads, details)."""
    nproc = os.cpu_count() or 1
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = nproc
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = max(1, int(int(q) // int(per)))
    except (OSError, ValueError):
        pass
    threads = min(aff, quota) if quota else aff
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:
        threads = min(threads, int(omp))
    return threads, {"nproc": nproc, "affinity_cpus": aff, "cgroup_cpu_quota": quota,
                     "omp_num_threads_env": os.environ.get("OMP_NUM_THREADS")}


def c1_per_call(oracle, netcsum, gpu):
    """Config C1 (BASELINE configs[0]): one 64-B UDP datagram of the loopback echo (UDP length 72,
    IPv4 total 92), the per-datagram sequence DataCalc -> HdrCalc -> HdrVerify -> DataVerify
    (SURVEY §3.1/§3.2). CPU: the oracle's C loop (reference C path restatement, 1 thread). GPU: the
    product's four drop-in functions called from Python (ctypes, ~0.3 us per call included)."""
    import struct
    payload = bytes((k * 13) & 0xFF for k in range(64))
    src, dst = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])
    ip = struct.pack("!BBHHHBBH4s4s", 0x45, 0, 92, 1, 0x4000, 64, 17, 0, src, dst)
    frame = ip + struct.pack("!HHHH", 5000, 7, 72, 0) + payload
    ch = netcsum.Chain([{"data": frame, "proto": netcsum.NET_PROTOCOL_TYPE_UDP_V4, "transport_ix": 20,
                         "transport_hdr_len": 8, "data_len": 64}])
    ph = netcsum.HostBytes(struct.pack("!4s4sBBH", src, dst, 0, 17, 72))
    hb = netcsum.HostBytes(ip)
    iters = 200_000
    oracle.c1_loop(ch.ptr, ph.ptr, 12, hb.ptr, 1000)
    t0 = time.perf_counter()
    oracle.c1_loop(ch.ptr, ph.ptr, 12, hb.ptr, iters)
    cpu_us = (time.perf_counter() - t0) / (iters * 4) * 1e6
    res = {"datagram": "64-B UDP payload, UDP length 72, IPv4 total 92, 12-B pseudo-header",
           "sequence": "DataCalc, HdrCalc, HdrVerify, DataVerify", "cpu_us_per_call": round(cpu_us, 4),
           "cpu_kind": "port (oracle/net_util_oracle.c -O2, 1 thread, C loop)"}
    if gpu:
        want = (oracle.data_calc(ch.ptr, ph.ptr, 12), oracle.hdr_calc(hb.ptr, 20))
        got = (netcsum.DataCalc(ch.ptr, ph.ptr, 12), netcsum.HdrCalc(hb.ptr, 20))
        reps = 500
        t0 = time.perf_counter()
        for _ in range(reps):
            netcsum.DataCalc(ch.ptr, ph.ptr, 12)
            netcsum.HdrCalc(hb.ptr, 20)
            netcsum.HdrVerify(hb.ptr, 20)
            netcsum.DataVerify(ch.ptr, ph.ptr, 12)
        gpu_us = (time.perf_counter() - t0) / (reps * 4) * 1e6
        res.update({"gpu_dropin_us_per_call": round(gpu_us, 3), "gpu_matches_oracle": got == want,
                    "gpu_over_cpu": round(gpu_us / cpu_us, 1)})
        res["crc32_mac_per_call"] = crc_per_call(oracle, netcsum)
    return res


def crc_per_call(oracle, netcsum):
    """The drivers' per-call CRC-32 (NetUtil_32BitCRC_CalcCpl of one 6-B multicast MAC address, the
    reference's only CRC use): the drop-in (host table below 4 KiB, net_util_mi355x.c), the GPU round
    trip the drop-in no longer takes for it (NetUtil_MI355X_CRC32Host: launch + D2H + sync), and the
    oracle's C restatement, all called from Python through ctypes (the call overhead is in all three)."""
    import ctypes
    mac = bytes([0x01, 0x00, 0x5E, 0x00, 0x00, 0xFB])
    hb = netcsum.HostBytes(mac)
    want = oracle.crc32_calc(mac, cpl=True)[0]
    reps = 2000

    def per_call(fn):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps * 1e6
    out = ctypes.c_uint32()
    lib = netcsum.lib()
    dropin_us = per_call(lambda: netcsum.CRC32Calc(hb.ptr, 6, cpl=True))
    gpu_us = per_call(lambda: lib.NetUtil_MI355X_CRC32Host(hb.ptr, 6, ctypes.byref(out)))
    cpu_us = per_call(lambda: oracle.crc32_calc(mac, cpl=True))
    got = netcsum.CRC32Calc(hb.ptr, 6, cpl=True)[0]
    return {"address": "01:00:5e:00:00:fb", "dropin_us_per_call": round(dropin_us, 3),
            "gpu_round_trip_us_per_call": round(gpu_us, 3), "oracle_us_per_call": round(cpu_us, 3),
            "dropin_matches_oracle": got == want}


def cpu_baseline(oracle, n_seg_full, L, plen, seconds):
    """Oracle (reference C path restatement) on a bounded sample of the C2 workload: gcc -O2 on all
    usable host CPUs (the reported value), gcc -O2 on one thread, and the same source built -O3
    -march=native for this host on all threads ("best CPU")."""
    import tempfile
    threads, cpu_info = host_cpus()
    n = 1 << 18                                      # 256 Ki segments = 396 MB: larger than the host LLC
    # first-touched by the workers that will read them (the batch's static partition)
    seg = oracle.fill_parallel(0, n * L, SEED, 0, n_threads=threads, unit=L)
    ph = c2_pseudo_headers(0, n, L, plen) if plen else None
    sample_b = n * (L + plen)
    reps, el = _time_cpu(lambda: oracle.batch_strided(seg, L, L, ph, plen, plen, n, 0, n_threads=threads), seconds)
    gib = reps * sample_b / el / 2 ** 30
    r1, e1 = _time_cpu(lambda: oracle.batch_strided(seg, L, L, ph, plen, plen, n, 0, n_threads=1), seconds / 4)
    best = None
    try:
        with tempfile.TemporaryDirectory() as td:
            path = oracle.build_native(td)
            want = oracle.batch_strided(seg, L, L, ph, plen, plen, 4096, 0, n_threads=threads)
            if (oracle.batch_strided_with(path, seg, L, L, ph, plen, plen, 4096, 0, threads) == want).all():
                rb, eb = _time_cpu(lambda: oracle.batch_strided_with(path, seg, L, L, ph, plen, plen, n, 0, threads),
                                   seconds / 2)
                best = round(rb * sample_b / eb / 2 ** 30, 3)
    except Exception as e:                           # noqa: BLE001 — a missing compiler only drops this line
        best = f"unavailable: {e}"
    cpu_info.update({"omp_proc_bind": os.environ.get("OMP_PROC_BIND"), "omp_places": os.environ.get("OMP_PLACES"),
                     "first_touch": "OpenMP workers (static partition of the batch)"})
    return {"value": round(gib, 3), "unit": "GiB/s", "cores": threads, "kind": "port", **cpu_info,
            "value_per_core": round(gib / threads, 3),
            "value_1thread": round(r1 * sample_b / e1 / 2 ** 30, 3),
            "value_best_cpu_O3_native": best, "cpu_model": cpu_model(),
            "sample": f"{reps} passes x {n} segments x ({L}+{plen}) B (C2 shape, {sample_b / 1e6:.0f} MB), "
                      f"oracle/net_util_oracle.c -O2 OpenMP static, {el:.2f} s wall x {threads} threads "
                      f"= {el * threads:.0f} core-s; 1-thread line {r1} passes in {e1:.2f} s; best-CPU line "
                      f"= same source -O3 -march=native on {threads} threads; threads = affinity mask "
                      f"capped by the cgroup CPU quota"}


# Sources that define each dominant kernel: a PMC summary is valid only for the exact sources it was
# collected from (tools/pmc_summary.py records their hash; bench.py recomputes it here).
KERNEL_SOURCES = {
    "seg_stream_kernel": ["netcsum_stream.hip", "netcsum_stream.h", "netcsum_device.h", "netcsum_kernels.h"],
}


def kernel_src_sha(kernel_fn):
    import hashlib
    files = KERNEL_SOURCES.get(kernel_fn)
    if not files:
        return None
    h = hashlib.sha256()
    for f in files:
        h.update(open(os.path.join(REPO, "uc-tcp-ip_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def live_traffic(args, n, kernel_desc):
    """HBM bytes per launch of the dominant kernel measured NOW: two rocprofv3 passes (--pmc FETCH_SIZE,
    --pmc WRITE_SIZE; one counter group per pass, MI355X_MICROARCH.md §HBM) over a child run of this
    bench (3 launches, same size and tuning). The child is a separate process started after this one's
    timing; rocprofv3 runs the Python interpreter directly after `--`. Returns (bytes, source, problem)."""
    import shutil
    import statistics
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, None, "rocprofv3 not on PATH"
    kfn = kernel_desc.split("::")[-1].split("<")[0] + "<"
    tmp = tempfile.mkdtemp(prefix="bench_pmc_", dir="/tmp")
    child = [sys.executable, os.path.abspath(__file__), "--full", "--steps", "3", "--warmup", "1", "--ramp-seconds", "0",
             "--no-cpu-baseline", "--no-c5-point", "--pmc", "off", "--segments", str(n), "--seg-len", str(args.seg_len),
             "--pseudo-len", str(args.pseudo_len)] + [x for kv in args.tune for x in ("--tune", kv)]
    vals = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        cmd = ["timeout", "-s", "KILL", "120", exe, "--pmc", counter, "-d", os.path.join(tmp, counter), "-o", counter,
               "--output-format", "csv", "--"] + child
        r = subprocess.run(cmd, cwd="/tmp", env={**os.environ, "TMPDIR": "/tmp"}, capture_output=True, text=True)
        if r.returncode != 0:
            return None, None, f"rocprofv3 --pmc {counter} exited {r.returncode}: {r.stderr.strip()[-300:]}"
        rows = []
        for f in glob.glob(os.path.join(tmp, counter, "**", f"{counter}_counter_collection.csv"), recursive=True):
            import csv
            rows += [float(x["Counter_Value"]) for x in csv.DictReader(open(f))
                     if kfn in x["Kernel_Name"] and x["Counter_Name"] == counter]
        if not rows:
            return None, None, f"no {counter} rows for {kfn} in the rocprofv3 output"
        vals[counter] = statistics.median(rows)
    shutil.rmtree(tmp, ignore_errors=True)
    b = vals["FETCH_SIZE"] * 1024 * 2 + vals["WRITE_SIZE"] * 1024
    return b, (f"live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over a 3-launch child run "
               f"(median per launch: FETCH_SIZE {vals['FETCH_SIZE']:.0f} KB x2, WRITE_SIZE {vals['WRITE_SIZE']:.0f} KB)"), None


C5_COUNTERS = ("TCP_UTCL1_TRANSLATION_MISS_sum", "TCP_UTCL1_REQUEST_sum", "TCP_UTCL1_STALL_INFLIGHT_MAX_sum",
               "TCP_TCC_READ_REQ_LATENCY_sum", "GRBM_UTCL2_BUSY", "GRBM_GUI_ACTIVE", "TCC_EA0_RDREQ_sum", "TCC_TAG_STALL_sum")


def live_c5_counters(args):
    """VERDICT r5 next #1, on whatever box runs the bench: one rocprofv3 --pmc pass (4 TCP, 2 GRBM, 2 TCC
    counters: within one pass's limits) over a child run of the C5 shard (3 launches, then the bench's
    two read probes over the same 25 GB), so that the record says, for the checksum kernel and for
    read_run_kernel (its access pattern, no arithmetic), how many address translations missed the
    UTCL1, how busy the UTCL2 was and the L2's HBM read requests — a box where the kernel falls behind
    the probe shows there which of them differs. Returns {kernel short name: {counter: median}}."""
    import csv
    import shutil
    import statistics
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not on PATH"}
    tmp = tempfile.mkdtemp(prefix="bench_c5pmc_", dir="/tmp")
    child = [sys.executable, os.path.abspath(__file__), "--full", "--steps", "3", "--warmup", "1", "--ramp-seconds", "0",
             "--no-cpu-baseline", "--no-c5-point", "--pmc", "off", "--segments", str(C5_SHARD), "--seg-len",
             str(args.seg_len), "--pseudo-len", str(args.pseudo_len)]
    cmd = ["timeout", "-s", "KILL", "180", exe, "--pmc", *C5_COUNTERS, "-d", tmp, "-o", "c5", "--output-format", "csv",
           "--"] + child
    r = subprocess.run(cmd, cwd="/tmp", env={**os.environ, "TMPDIR": "/tmp"}, capture_output=True, text=True)
    if r.returncode != 0:
        shutil.rmtree(tmp, ignore_errors=True)
        return {"error": f"rocprofv3 exited {r.returncode}: {r.stderr.strip()[-300:]}"}
    vals = {}
    for f in glob.glob(os.path.join(tmp, "**", "c5_counter_collection.csv"), recursive=True):
        for x in csv.DictReader(open(f)):
            k = next((n for n in ("seg_stream_kernel", "read_run_kernel", "read_stream_lds_kernel") if n in x["Kernel_Name"]), None)
            if k:
                vals.setdefault(k, {}).setdefault(x["Counter_Name"], []).append(float(x["Counter_Value"]))
    shutil.rmtree(tmp, ignore_errors=True)
    out = {k: {c: statistics.median(v) for c, v in cs.items()} for k, cs in vals.items()}
    for k, d in out.items():
        if d.get("TCP_UTCL1_REQUEST_sum"):
            d["utcl1_miss_per_request"] = round(d.get("TCP_UTCL1_TRANSLATION_MISS_sum", 0.0) / d["TCP_UTCL1_REQUEST_sum"], 7)
        if d.get("GRBM_GUI_ACTIVE"):
            d["utcl2_busy_frac"] = round(d.get("GRBM_UTCL2_BUSY", 0.0) / d["GRBM_GUI_ACTIVE"], 5)
    return out or {"error": "no counter rows for the C5 kernels"}


def load_traffic(path, n_seg, kernel_desc):
    """HBM bytes per launch of THIS kernel (name, template form, launch geometry and source hash)
    at this size, from a rocprofv3 PMC summary under profiles/. Returns (bytes, source, problem):
    a summary whose kernel or sources differ from the launched one is refused and reported."""
    kernel_fn = kernel_desc.split("::")[-1].split("<")[0]
    sha = kernel_src_sha(kernel_fn)
    cands = [path] if path else sorted(glob.glob(os.path.join(REPO, "profiles", "*pmc*.json")))
    stale = []
    for p in reversed(cands):
        try:
            d = json.load(open(p))
        except Exception:
            continue
        if d.get("n_seg") != n_seg or "hbm_bytes_per_launch" not in d:
            continue
        if d.get("kernel_desc") != kernel_desc:
            continue
        if d.get("kernel_src_sha") != sha:
            stale.append(os.path.relpath(p, REPO))
            continue
        return float(d["hbm_bytes_per_launch"]), os.path.relpath(p, REPO), None
    why = (f"no PMC summary for {kernel_desc} at n_seg={n_seg} with kernel_src_sha={sha}"
           + (f" (stale: {', '.join(stale)})" if stale else ""))
    print(f"[bench] roofline.traffic unavailable: {why} — run tools/gpu_run.sh to re-collect",
          file=sys.stderr, flush=True)
    return None, None, why


def headline(args, world, n, wall, ramp_launches, backend, ndev):
    """The result line of a plain run (rank 0): the headline figure from the timed region alone (`wall` =
    max over ranks of the wall time of the K timed steps) and the run's configuration. --full adds its
    own measurements to it."""
    L, plen = args.seg_len, args.pseudo_len
    value = world * n * (L + plen) * args.steps / wall / 2 ** 30
    return {
        "metric": METRIC,
        "value": round(value, 2),
        "unit": "GiB/s",
        "value_per_gpu": round(value / world, 2),
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ramp_launches": ramp_launches,
        "ms_per_step": round(wall / args.steps * 1e3, 5),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u16",
        "data": "synthetic (device-generated splitmix64 bytes, seed 0x5EED0001, rank shard = slice of one global stream; IPv4 pseudo-headers from the global index)",
        "config": {"workload": (("C2: 1 M x " if world == 1 and n == 1 << 20 else
                                 f"C5 shard: {n} x " if n == C5_SHARD else f"{n} x ")
                                + f"{L} B TCP segments + {plen} B IPv4 pseudo-header per GPU, device-resident, "
                                "NetUtil_16BitOnesCplChkSumDataCalc per segment"),
                   "segments_per_gpu": n, "seg_len": L, "pseudo_len": plen,
                   "global_batch": n * world, "parallelism": f"shard{world} (no collective)",
                   "dist": "single rank" if world == 1 else f"{world} ranks, backend {backend}, devices: " + (
                       "one per rank" if backend == "nccl" else f"{ndev} shared (rehearsal)")},
    }


def main():
    args = parse()
    if args.steps < 1:
        raise SystemExit(f"bench.py: --steps {args.steps} must be >= 1")
    if world_check(args.gpus) == "launch":
        return launch_ranks(args)
    stage("start")
    if args.launcher_selftest:
        return launcher_selftest(args.launcher_selftest)
    import torch
    import torch.distributed as dist

    import netcsum
    stage("torch imported")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    local_env = local                              # (the device index may be folded below: gloo rehearsal)
    # RCCL ("nccl") carries the barrier and the two reductions; NETCSUM_BENCH_DIST_BACKEND=gloo (host
    # tensors) lets several ranks share one GPU to rehearse the N > 1 path (RCCL refuses duplicate GPUs)
    backend = os.environ.get("NETCSUM_BENCH_DIST_BACKEND", "nccl")
    # one rank per GPU: only the gloo rehearsal may fold several ranks onto fewer devices
    ndev = torch.cuda.device_count()
    if local >= ndev:
        if backend != "gloo" or ndev == 0:
            print(f"bench.py: rank {rank} has LOCAL_RANK {local} but this node shows {ndev} GPU(s); refusing to "
                  f"fold ranks onto shared devices (only NETCSUM_BENCH_DIST_BACKEND=gloo rehearses that)",
                  file=sys.stderr, flush=True)
            return 2
        local = local % ndev
    if world > 1:
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)
        stage("process group up")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    keymap = {"grid": netcsum.TUNE_GRID_BLOCKS, "group": netcsum.TUNE_GROUP_LANES,
              "nt": netcsum.TUNE_NT_LOADS, "block": netcsum.TUNE_BLOCK_THREADS, "kernel": netcsum.TUNE_KERNEL,
              "chunks": netcsum.TUNE_CHUNKS, "tile": netcsum.TUNE_TILE, "mult": netcsum.TUNE_GRID_MULT,
              "xcd": netcsum.TUNE_STREAM_XCD, "touch": netcsum.TUNE_STREAM_TOUCH, "waves": netcsum.TUNE_STREAM_WAVES}
    for kv in args.tune:
        k, v = kv.split("=")
        netcsum.tune(keymap[k], int(v))

    n, L, plen = args.segments, args.seg_len, args.pseudo_len
    if n is None:
        n = (1 << 20) if world == 1 else C5_SHARD         # C2 at N=1; the C5 shard (16 M) at N>1
    start, n = shard_range(rank, n)
    seg, ph = make_c2_shard(torch, netcsum, start, n, L, plen, dev)
    out = torch.empty(n, dtype=torch.int16, device=dev)
    stream = torch.cuda.current_stream(dev)
    stage("shard generated")

    def step():
        netcsum.batch_strided(seg, L, L, ph, plen, plen, n, out, netcsum.OP_DATA_CALC, stream=stream)

    # untimed clock ramp (by time, independent of --warmup), then the W counted warm-up steps
    t_ramp, ramp_launches = time.perf_counter(), 0
    while time.perf_counter() - t_ramp < args.ramp_seconds or ramp_launches < 8:
        for _ in range(8):
            step()
        ramp_launches += 8
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    kernel_desc = "netcsum::" + netcsum.last_launch()
    stage("warm-up done")

    # timed region: exactly K steps, barrier + synchronize on both sides, nothing else enqueued
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    wall = time.perf_counter() - t0
    stage("timed region done")
    if args.dump_outputs:                          # `out` is as the last timed step left it
        dump_outputs(torch, args.dump_outputs, out, rank, world)

    if not args.full:                              # plain run: the headline line only
        if world > 1:
            t = torch.tensor([wall], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            wall = float(t.item())
        if rank == 0:
            print(json.dumps(headline(args, world, n, wall, ramp_launches, backend, ndev)), flush=True)
        stage("reported")
        if world > 1:
            dist.destroy_process_group()
        return 0

    # roofline pass (untimed for `value`): HIP events on the launch stream around each of K launches
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for a, b in evs:
        a.record(stream)
        step()
        b.record(stream)
    torch.cuda.synchronize()
    kern = sorted(a.elapsed_time(b) for a, b in evs)
    kern_ms = sum(kern) / len(kern)
    kern_med_ms = kern[len(kern) // 2]

    wall_own = wall
    if world > 1:
        t = torch.tensor([wall], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())

    # parity spot check of this rank's output (outside the timed region), against the oracle
    parity_ok = None
    try:
        import numpy as np
        import oracle
        rng = np.random.default_rng(rank)
        sample = np.sort(rng.choice(n, size=min(256, n), replace=False))
        sidx = torch.from_numpy(sample).to(dev)
        segs = seg[: n * L].view(n, L)[sidx].cpu().numpy().reshape(-1)
        phs = ph.view(n, plen)[sidx].cpu().numpy().reshape(-1) if plen else None
        want = oracle.batch_strided(segs, L, L, phs, plen, plen, len(sample), 0)
        parity_ok = bool(np.array_equal(out.cpu().numpy().view(np.uint16)[sample], want))
    except Exception as e:  # oracle missing on this host: report, never substitute
        parity_ok = f"unchecked: {e}"

    # measured read-stream rates over the same bytes (roofline probes), same stream & events: the
    # LDS-DMA grid-stride probe (TUNE_PROBE 1) and the run-stream form of the checksum kernel with no
    # arithmetic (TUNE_PROBE 2, netcsum_stream.hip read_run_kernel)
    n16 = (n * L) // 16 * 16
    lds_probe_gbps, run_probe_gbps = read_probes(torch, netcsum, seg, n16, stream)
    achieved = n * (L + plen + 2) / (kern_ms * 1e-3) / 1e9

    # N > 1: every rank's own numbers, gathered (rank order), so that the record names a slow device
    ranks = None
    if world > 1:
        own = {"rank": rank, "local_rank": local_env, "device": local, "wall_s": wall_own, "kernel_ms": kern_ms,
               "per_gpu_GiBps": n * (L + plen) * args.steps / wall_own / 2 ** 30,
               "run_stream_read_probe_GBps": run_probe_gbps, "read_stream_probe_GBps": lds_probe_gbps,
               "frac_of_run_stream_read_probe": achieved / run_probe_gbps,
               "parity_sample_ok": 1.0 if parity_ok is True else 0.0}
        ranks = rank_summary(rank_records(dist, dev if backend == "nccl" else "cpu", own, world))

    c5 = None
    if world == 1 and not args.no_c5_point and n != C5_SHARD:
        del seg, ph, out
        torch.cuda.empty_cache()
        try:
            c5 = c5_point(torch, netcsum, args, dev, stream)
        except Exception as e:                    # noqa: BLE001 — report, the headline stands without it
            c5 = {"error": str(e)}

    parity_all = parity_ok
    if world > 1:                                  # every rank's sample must match its oracle
        t = torch.tensor([1 if parity_ok is True else 0], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        parity_all = bool(t.item()) if not isinstance(parity_ok, str) else parity_ok

    if rank == 0:
        algo_bytes = n * (L + plen + 2)
        traffic, traffic_src = None, None
        traffic_err = "--pmc off" if args.pmc == "off" else None
        live_err = None
        if args.pmc == "live" and world == 1:
            traffic, traffic_src, live_err = live_traffic(args, n, kernel_desc)
        if traffic is None and args.pmc != "off":
            traffic, traffic_src, traffic_err = load_traffic(args.traffic_json, n, kernel_desc)
            if live_err:
                traffic_err = f"live PMC failed ({live_err}); " + (traffic_err or "committed summary used")
        line = headline(args, world, n, wall, ramp_launches, backend, ndev)
        line.update({
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBPS, 4),
                         "traffic": round(traffic) if traffic is not None else None,
                         "traffic_over_algorithmic": round(traffic / algo_bytes, 4) if traffic else None,
                         "kernel": kernel_desc,
                         "kernel_ms": round(kern_ms, 5), "kernel_ms_median": round(kern_med_ms, 5),
                         "algorithmic_bytes_per_launch": algo_bytes,
                         "traffic_source": traffic_src,
                         "traffic_error": traffic_err,
                         "kernel_src_sha": kernel_src_sha(kernel_desc.split("::")[-1].split("<")[0]),
                         "read_stream_probe_GBps": round(lds_probe_gbps, 1),
                         "frac_of_read_stream_probe": round(achieved / lds_probe_gbps, 4),
                         "run_stream_read_probe_GBps": round(run_probe_gbps, 1),
                         "frac_of_run_stream_read_probe": round(achieved / run_probe_gbps, 4)},
            "parity_sample_ok": parity_all,
        })
        if c5 is not None:
            if args.pmc == "live" and "error" not in c5:
                c5["pmc_live"] = live_c5_counters(args)
            line["c5_shard_point"] = c5
        if ranks is not None:
            line["ranks"] = ranks
        if world == 1 and not args.no_cpu_baseline:
            try:
                import oracle
                line["cpu_baseline"] = cpu_baseline(oracle, n, L, plen, args.cpu_seconds)
            except Exception as e:
                line["cpu_baseline"] = {"value": None, "error": str(e)}
            try:
                import oracle
                line["c1_per_datagram"] = c1_per_call(oracle, netcsum, gpu=True)
            except Exception as e:
                line["c1_per_datagram"] = {"error": str(e)}
        print(json.dumps(line), flush=True)
    stage("reported")

    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
