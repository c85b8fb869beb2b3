#!/usr/bin/env python3
"""NetUtil_MI355X_RxBurstSums against NetUtil_MI355X_RxBurst on a ring of 1520-B pool slots (frame at
+14, 1 Mi frames of 1500 B), one session, the calls of each pair alternating:

  (a) unfragmented IPv4/TCP frames: RxBurstSums against RxBurst on the same ring. The bytes streamed
      are identical; the sums launch adds one 4-B store per frame (0.3 % more traffic).
  (b) IPv4 fragments with 1480-B payloads: RxBurstSums on the ring of fragments against RxBurst on the
      ring of unfragmented frames of the same total length. A fragment is now read as an unfragmented
      frame is (RxBurst alone stops at its IP header: `frag_rx_burst_ms`, for scale).
  (c) with --parent-lib PATH (a libnetcsum_mi355x.so built from the parent commit): RxBurst of that
      library against RxBurst of this one on the ring of (a); the instantiations RxBurst launches are
      meant to be unchanged.

One JSON line per pass (median of 20 launches per figure after a timed warm-up, device events):

  python tools/rx_sums_bench.py [--parent-lib PATH] [--frames N] [--passes K] >> profiles/TAG_rx_sums_bench.jsonl

Every pass also checks the results it timed: the actions of both calls, and every frame's record
against the record the oracle gives for that frame.
"""
import argparse
import ctypes
import json
import os
import random
import struct
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("uc-tcp-ip_amd", "oracle", "", "tools", "tests"):
    sys.path.insert(0, os.path.join(REPO, sub))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import netcsum  # noqa: E402
import oracle  # noqa: E402
import oracle_packets as op  # noqa: E402
from bench import SEED  # noqa: E402
from bench_configs import events_ms  # noqa: E402

STRIDE, LEAD, TOT, KINDS = 1520, 14, 1500, 256


def tcp_frame(rng):
    l4 = struct.pack("!HHIIBBHHH", rng.getrandbits(16), rng.getrandbits(16), rng.getrandbits(32), rng.getrandbits(32),
                     5 << 4, 0x18, 0xFFFF, 0, 0) + rng.randbytes(TOT - 40)
    hdr = struct.pack("!BBHHHBBH4s4s", 0x45, 0, TOT, rng.getrandbits(16), 0x4000, 64, 6, 0, rng.randbytes(4), rng.randbytes(4))
    return op.tx_finalize(hdr + l4)[0]


def fragment(rng):
    hdr = struct.pack("!BBHHHBBH4s4s", 0x45, 0, TOT, rng.getrandbits(16), 0x2000 | rng.randint(0, 40) * 185, 64, 6, 0,
                      rng.randbytes(4), rng.randbytes(4))
    return op.tx_finalize(hdr + rng.randbytes(TOT - 20))[0]


def record(frame):
    ch = netcsum.Chain([{"data": frame[20:TOT], "proto": netcsum.NET_PROTOCOL_TYPE_TCP_V4}])
    return ((~oracle.data_calc(ch.ptr, None, 0)[0]) & 0xFFFF) | ((TOT - 20) << 16)


def ring(frames, n, dev):
    """n slots holding frames[i % KINDS] at +LEAD, the rest of each slot filled by the library's generator."""
    buf = torch.empty(LEAD + n * STRIDE + 256, dtype=torch.uint8, device=dev)
    netcsum.fill(buf, buf.numel() & ~7, SEED, 0)
    img = np.zeros((KINDS, STRIDE), np.uint8)
    keep = torch.ones(STRIDE, dtype=torch.bool, device=dev)
    keep[:TOT] = False
    for k, f in enumerate(frames):
        img[k, :TOT] = np.frombuffer(f, np.uint8)
    slots = buf[LEAD:LEAD + n * STRIDE].view(n, STRIDE)
    tiled = torch.from_numpy(img).to(dev).repeat((n + KINDS - 1) // KINDS, 1)[:n]
    slots.copy_(torch.where(keep, slots, tiled))
    return buf


def parent_rx_burst(path):
    L = ctypes.CDLL(path)
    vp, u16, u32, u64 = ctypes.c_void_p, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64
    L.NetUtil_MI355X_RxBurst.argtypes = [vp, vp, vp, u64, u16, u32, u32, vp, vp, vp]
    L.NetUtil_MI355X_RxBurst.restype = ctypes.c_int

    def call(base, n, act, st):
        err = L.NetUtil_MI355X_RxBurst(base.data_ptr(), None, None, STRIDE, TOT, n, 0, act.data_ptr(), None, st.cuda_stream)
        assert err == netcsum.NET_UTIL_ERR_NONE, err
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    n = a.frames
    rng = random.Random(SEED)
    tcp = [tcp_frame(rng) for _ in range(KINDS)]
    frg = [fragment(rng) for _ in range(KINDS)]
    want = torch.from_numpy(np.array([record(f) for f in frg], np.uint32).view(np.int32)).to(dev)
    ring_tcp, ring_frg = ring(tcp, n, dev), ring(frg, n, dev)
    act0, act1 = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
    sums = torch.empty(n, dtype=torch.int32, device=dev)
    parent = parent_rx_burst(a.parent_lib) if a.parent_lib else None

    def rx(r, act):
        netcsum.rx_burst(r[LEAD:], n, act, stride=STRIDE, pkt_len=TOT, stream=st)

    def rxs(r, act):
        netcsum.rx_burst_sums(r[LEAD:], n, act, sums, stride=STRIDE, pkt_len=TOT, stream=st)

    for p in range(a.passes):
        r = {"pass": p, "frames": n, "stride": STRIDE, "lead": LEAD, "frame_bytes": TOT}
        r["a_rx_burst_ms"] = events_ms(lambda: rx(ring_tcp, act0), st)
        r["kernel_rx_burst"] = netcsum.last_launch()
        r["a_rx_burst_sums_ms"] = events_ms(lambda: rxs(ring_tcp, act1), st)
        r["kernel_rx_burst_sums"] = netcsum.last_launch()
        ok = bool((act0 == 0).all()) and bool((act1 == 0).all()) and bool((sums == 0).all())
        r["b_frag_rx_burst_sums_ms"] = events_ms(lambda: rxs(ring_frg, act1), st)
        r["kernel_frag_rx_burst_sums"] = netcsum.last_launch()
        ok = ok and bool((act1 == netcsum.RX_DELIVER_L4_UNVERIFIED).all())
        ok = ok and bool((sums.view(-1) == want.repeat((n + KINDS - 1) // KINDS)[:n]).all())
        r["b_unfrag_rx_burst_ms"] = events_ms(lambda: rx(ring_tcp, act0), st)
        r["frag_rx_burst_ms"] = events_ms(lambda: rx(ring_frg, act0), st)
        ok = ok and bool((act0 == netcsum.RX_DELIVER_L4_UNVERIFIED).all())
        if parent:
            base = ring_tcp[LEAD:]
            r["c_parent_rx_burst_ms"] = events_ms(lambda: parent(base, n, act1, st), st)
            ok = ok and bool((act1 == 0).all())
            r["c_this_rx_burst_ms"] = events_ms(lambda: rx(ring_tcp, act0), st)
            r["c_this_over_parent"] = round(r["c_this_rx_burst_ms"] / r["c_parent_rx_burst_ms"], 4)
        r["a_sums_over_rx_burst"] = round(r["a_rx_burst_sums_ms"] / r["a_rx_burst_ms"], 4)
        r["b_frag_sums_over_unfrag_rx_burst"] = round(r["b_frag_rx_burst_sums_ms"] / r["b_unfrag_rx_burst_ms"], 4)
        r["b_frag_read_GBps"] = round(n * TOT / r["b_frag_rx_burst_sums_ms"] / 1e6, 1)
        r["results_ok"] = ok
        for k in list(r):
            if k.endswith("_ms"):
                r[k] = round(r[k], 4)
        print(json.dumps(r), flush=True)
        if not ok:
            sys.exit("rx_sums_bench: a timed call's results are wrong")


if __name__ == "__main__":
    main()
