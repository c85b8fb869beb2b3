#!/usr/bin/env python3
"""What frame-level input costs on the Tx side: NetUtil_MI355X_TxBurstEther on one device-resident ring of
1520-B slots holding 1 Mi Ethernet II IPv4/TCP frames of 1514 octets (frame at +0, a length array) against
NetUtil_MI355X_TxBurst over precomputed {off + 14, len - 14} descriptors — the Tx demux pass alone. The two
calls alternate, five repetitions of 20 timed calls; one JSON line per repetition (median, min, max in ms).
DESIGN §8."""
import json
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uc-tcp-ip_amd"))
import numpy as np
import torch

import netcsum

N, SLOT, FRAME = 1 << 20, 1520, 1514
rng = np.random.default_rng(7)
slot = rng.integers(0, 256, SLOT, dtype=np.uint8)
slot[0:12] = np.frombuffer(bytes.fromhex("02c0ffee000102a1b2c3d4e5"), np.uint8)
slot[12:14] = (0x08, 0x00)
ip = bytearray(struct.pack("!BBHHHBBH4s4s", 0x45, 0, 1500, 7, 0x4000, 64, 6, 0, b"\x0a\x00\x00\x01", b"\x0a\x00\x00\x02"))
slot[14:34] = np.frombuffer(bytes(ip), np.uint8)
slot[14 + 20 + 12] = 0x50
slot[14 + 20 + 16:14 + 20 + 18] = 0
ring = torch.from_numpy(slot).cuda().repeat(N)
lens = torch.full((N,), FRAME, dtype=torch.int16, device="cuda")
off2 = (torch.arange(N, dtype=torch.int64, device="cuda") * SLOT + 14)
len2 = torch.full((N,), FRAME - 14, dtype=torch.int16, device="cuda")
l2 = torch.zeros(N, dtype=torch.uint8, device="cuda")

def t_ms(fn, k=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]

ether = lambda: netcsum.tx_burst_ether(ring, N, l2, lens=lens, stride=SLOT)
plain = lambda: netcsum.tx_burst(ring, N, off=off2, lens=len2)
for rep in range(5):
    e = t_ms(ether); le = netcsum.last_launch()
    p = t_ms(plain); lp = netcsum.last_launch()
    print(json.dumps({"rep": rep, "frames": N, "tx_burst_ether_ms": [round(x, 4) for x in e], "tx_burst_offlen_ms": [round(x, 4) for x in p],
                      "order": "median,min,max of 20", "launch_ether": le, "launch_offlen": lp}), flush=True)
assert int((l2 != netcsum.L2_ETHER_IPV4).sum()) == 0
