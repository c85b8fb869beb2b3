#!/usr/bin/env python3
"""What frame-level input costs: NetUtil_MI355X_RxBurstEther against NetUtil_MI355X_RxBurst on one ring
of 1520-B slots holding 1 Mi Ethernet II IPv4/TCP frames of 1514 octets (frame at +0, a received-length
array), one session, the three calls alternating:

  ether    RxBurstEther on the ring itself (slots at a pitch + the received lengths);
  strided  RxBurst strided at +14, 1500 octets per slot: the shortcut for rings known to carry only
           Ethernet II IP. ether - strided is the whole price of frame-level input (the demux pass and
           the offset/length form of the packet pass instead of the strided one);
  offlen   RxBurst offset/length over precomputed descriptors {i * 1520 + 14, 1500}: the packet pass
           RxBurstEther runs, without its front pass. ether - offlen is the demux pass alone.

The demux pass reads one 64-B sector per frame here (a frame's 23 octets at +0 of a 1520-B slot never
straddle a sector) and writes 11 B per frame; `demux_sector_bytes` is that read, from the shapes.

One JSON line per pass (median of 20 launches per figure after a timed warm-up, device events):

  python tools/ether_burst_bench.py [--frames N] [--passes K] >> profiles/ether_burst_bench.jsonl

With --sums a fourth call alternates with them: `ether_sums`, RxBurstEtherSums on the same ring (the
same two launches with the SUMS instantiation of the packet pass and 4 B more written per frame; no frame
of this ring is a fragment, so every record is {0, 0}); ether_sums - ether is what the records cost.

Every pass also checks the results it timed: all the calls' actions, the classes, and the records.
"""
import argparse
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
import oracle_packets as op  # noqa: E402
from bench import SEED  # noqa: E402
from bench_configs import events_ms  # noqa: E402

STRIDE, HDR, TOT, KINDS = 1520, 14, 1500, 256
FRAME = HDR + TOT
HW = bytes.fromhex("02a1b2c3d4e5")


def tcp_frame(rng):
    l4 = struct.pack("!HHIIBBHHH", rng.getrandbits(16), rng.getrandbits(16), rng.getrandbits(32), rng.getrandbits(32),
                     5 << 4, 0x18, 0xFFFF, 0, 0) + rng.randbytes(TOT - 40)
    hdr = struct.pack("!BBHHHBBH4s4s", 0x45, 0, TOT, rng.getrandbits(16), 0x4000, 64, 6, 0, rng.randbytes(4), rng.randbytes(4))
    return HW + b"\x02" + rng.randbytes(5) + b"\x08\x00" + op.tx_finalize(hdr + l4)[0]


def ring(frames, n, dev):
    """n slots holding frames[i % KINDS] at +0, the rest of each slot filled by the library's generator."""
    buf = torch.empty(n * STRIDE + 256, dtype=torch.uint8, device=dev)
    netcsum.fill(buf, buf.numel() & ~7, SEED, 0)
    img = np.zeros((KINDS, STRIDE), np.uint8)
    keep = torch.ones(STRIDE, dtype=torch.bool, device=dev)
    keep[:FRAME] = False
    for k, f in enumerate(frames):
        img[k, :FRAME] = np.frombuffer(f, np.uint8)
    slots = buf[:n * STRIDE].view(n, STRIDE)
    tiled = torch.from_numpy(img).to(dev).repeat((n + KINDS - 1) // KINDS, 1)[:n]
    slots.copy_(torch.where(keep, slots, tiled))
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--sums", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    n = a.frames
    rng = random.Random(SEED)
    r0 = ring([tcp_frame(rng) for _ in range(KINDS)], n, dev)
    lens = torch.full((n,), FRAME, dtype=torch.int16, device=dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * STRIDE + HDR
    ip_lens = torch.full((n,), TOT, dtype=torch.int16, device=dev)
    act_e, act_s, act_o, l2 = (torch.full((n,), 0xEE, dtype=torch.uint8, device=dev) for _ in range(4))

    def ether():
        netcsum.rx_burst_ether(r0, n, act_e, l2, lens=lens, stride=STRIDE, hw_addr=HW, stream=st)

    act_es, l2s = (torch.full((n,), 0xEE, dtype=torch.uint8, device=dev) for _ in range(2))
    rec = torch.full((n if a.sums else 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)

    def ether_sums():
        netcsum.rx_burst_ether_sums(r0, n, act_es, l2s, rec, lens=lens, stride=STRIDE, hw_addr=HW, stream=st)

    def strided():
        netcsum.rx_burst(r0[HDR:], n, act_s, stride=STRIDE, pkt_len=TOT, stream=st)

    def offlen():
        netcsum.rx_burst(r0, n, act_o, off=off, lens=ip_lens, stream=st)

    for p in range(a.passes):
        r = {"pass": p, "frames": n, "stride": STRIDE, "frame_bytes": FRAME}
        calls = (("ether", ether), ("strided", strided), ("offlen", offlen)) + ((("ether_sums", ether_sums),) if a.sums else ())
        for name, fn in calls:
            r[f"{name}_ms"] = events_ms(fn, st)
            r[f"kernel_{name}"] = netcsum.last_launch()
        torch.cuda.synchronize()
        ok = all(bool((x == netcsum.RX_DELIVER).all()) for x in (act_e, act_s, act_o))
        ok = ok and bool((l2 == netcsum.L2_ETHER_IPV4).all())
        if a.sums:
            ok = ok and bool((act_es == netcsum.RX_DELIVER).all()) and bool((l2s == netcsum.L2_ETHER_IPV4).all())
            ok = ok and bool((rec == 0).all())
            r["ether_sums_minus_ether_ms"] = r["ether_sums_ms"] - r["ether_ms"]
        r["ether_minus_strided_ms"] = r["ether_ms"] - r["strided_ms"]          # frame-level input, all of it
        r["ether_minus_offlen_ms"] = r["ether_ms"] - r["offlen_ms"]            # the demux pass alone
        r["ether_over_strided"] = round(r["ether_ms"] / r["strided_ms"], 4)
        r["ether_over_offlen"] = round(r["ether_ms"] / r["offlen_ms"], 4)
        r["demux_sector_bytes"] = 64 * n                                      # one sector per frame on this ring
        r["results_ok"] = ok
        for k in list(r):
            if k.endswith("_ms"):
                r[k] = round(r[k], 4)
        print(json.dumps(r), flush=True)
        if not ok:
            sys.exit("ether_burst_bench: a timed call's results are wrong")


if __name__ == "__main__":
    main()
