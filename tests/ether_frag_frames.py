"""Ethernet-frame bursts with a raised share of IP fragments, for the RxBurstEtherSums tests
(include/netcsum_mi355x.h (2b''''): RxBurstEther with the fragment payload sums of (2b''')).

Built from what the two features' own tests use: the fragments of test_gpu_fragsum.py (v4_fragment,
v6_fragment, V6_CHAINS, PAYLOADS, fragment_mix) behind the headers of ether_frames.py (ether2, snap), and
the whole of ether_frames.frame_mix for everything that is not a fragment. Seeded; the same burst for
every test that asks for (layout, n).

What a burst holds (the CPU test test_ether_sums_cpu.py asserts it, so the mix cannot erode):
  * fragments behind both headers, Ethernet II (+14) and 802.3 + LLC/SNAP (+22);
  * IPv4 with IHL 5 / 6 / 15, payloads of 0, 1, 7, 8, 9, 1479, 1480 octets where the frame stays within
    1514 octets, all-zero payloads, some with a bad header checksum;
  * IPv6 fragments behind every chain of V6_CHAINS, the (60, 130) chain past the kernels' window among
    them (the extension-header walk writes that record);
  * short fragments padded to 60 octets with random NON-ZERO octets (a sum taken to the received length
    instead of the IP header's would include them);
  * every class of ether_frames.frame_mix (ARP, every INV_*, the type / version mismatches);
  * a frame of type 0x0800 that carries a well-formed IPv6 fragment and one of type 0x86DD that carries an
    IPv4 fragment: no datagram is handed to the checksum pass, so the record is {0, 0}.

Expectations: classes, flags and actions from ether_frames.expect; the record is
test_gpu_fragsum.want_record of the datagram ether_frames.ip_datagram finds, 0 where it finds none.
"""
from __future__ import annotations

import functools
import random

import numpy as np

import ether_frames as ef
from test_gpu_fragsum import PAYLOADS, V6_CHAINS, fragment_mix, v4_fragment, v6_fragment, want_record

MAX_FRAME = 1514
SNAP_ROOM = MAX_FRAME - 22 - 4              # datagram octets behind LLC/SNAP with the 4 FCS octets
LAYOUTS = ["packed1", "slot1520", "fixed"]
WALK_CHAIN = ((60, 130),)                   # 1040 octets of options: the Fragment header lies past the window


def _nonzero(rng, k):
    return bytes(rng.randint(1, 255) for _ in range(k))


def frame_e2(rng, dgram, etype=None, dst=ef.HW):
    """Ethernet II; a short frame is padded to 60 octets with random non-zero octets."""
    etype = (ef.T_IPV6 if dgram[0] >> 4 == 6 else ef.T_IPV4) if etype is None else etype
    used = 14 + len(dgram)
    return ef.ether2(dgram, etype, dst=dst)[:used] + _nonzero(rng, max(0, 60 - used))


def frame_snap(rng, dgram, dst=ef.HW):
    """802.3 + LLC/SNAP; padded to 60 with random non-zero octets, else 4 FCS octets behind the datagram."""
    f = ef.snap(dgram, ef.T_IPV6 if dgram[0] >> 4 == 6 else ef.T_IPV4, dst=dst, rng=rng)
    used = 22 + len(dgram)
    return f[:used] + _nonzero(rng, 60 - used) if used < 60 else f


@functools.lru_cache(maxsize=None)
def pools():
    """-> (essentials, fragments, others): lists of (name, frame). `essentials` are in every burst of more
    than a few frames; `fragments` all have a non-zero expected record at the interface's address."""
    rng = random.Random(4242)
    frags = []
    k = 0

    def add(name, dgram, force=None):
        nonlocal k
        k += 1
        use_snap = (k % 2 == 0 if force is None else force == "snap") and len(dgram) <= SNAP_ROOM
        frags.append((f"{'snap' if use_snap else 'e2'} frag {name}", (frame_snap if use_snap else frame_e2)(rng, dgram)))

    for ihl in (5, 6, 15):
        for pay in PAYLOADS:
            if pay and ihl * 4 + pay <= 1500:
                frag = rng.choice([0x2000, rng.randint(1, 0x1FFF), 0x2000 | rng.randint(1, 0x1FFF)])
                add(f"v4 ihl{ihl} pay{pay}", v4_fragment(rng, _nonzero(rng, pay), ihl, frag, rng.choice([6, 17, 1])))
                if pay < 20:                                             # the padded ones behind the other header too
                    add(f"v4 ihl{ihl} pay{pay} b", v4_fragment(rng, _nonzero(rng, pay), ihl, frag, 17))
    for ihl in (5, 6, 15):
        add(f"v4 ihl{ihl} bad ip csum", v4_fragment(rng, _nonzero(rng, 64 + ihl), ihl, 0x2000, 17, bad_ip=True))
    for chain in V6_CHAINS:
        room = 1500 - 48 - 8 * sum(u for _, u in chain)
        for pay in [p for p in PAYLOADS if 0 < p <= room] + [room]:
            add(f"v6 chain{chain} pay{pay}", v6_fragment(rng, _nonzero(rng, pay), chain, rng.choice([6, 17, 58]), rng.choice([1, 8, 0x5B9])))
    ess = []
    # the walk behind SNAP and behind Ethernet II; a padded fragment behind each header
    for force in ("snap", "e2"):
        add("essential v6 walk", v6_fragment(rng, _nonzero(rng, 200), WALK_CHAIN, 17, 1), force)
        ess.append(frags.pop())
        add("essential v4 pay7 padded", v4_fragment(rng, _nonzero(rng, 7), 5, 0x2000, 17), force)
        ess.append(frags.pop())
    # a full-size SNAP frame: its length field (1496) is the one the rule accepts in the fixed-length layout too
    add("essential v4 pay1468 full snap", v4_fragment(rng, _nonzero(rng, SNAP_ROOM - 20), 5, 0x2000, 6), "snap")
    ess.append(frags.pop())
    assert len(ess[-1][1]) == MAX_FRAME
    # type / version mismatches that carry well-formed fragments: nothing to check, record {0, 0}
    ess.append(("mismatch type v4, v6 fragment", frame_e2(rng, v6_fragment(rng, _nonzero(rng, 300)), ef.T_IPV4)))
    ess.append(("mismatch type v6, v4 fragment", frame_e2(rng, v4_fragment(rng, _nonzero(rng, 300)), ef.T_IPV6)))
    # a fragment for another station (INV_ADDR_DEST unless promiscuous): record 0 at the interface's address
    ess.append(("other station, v4 fragment", frame_e2(rng, v4_fragment(rng, _nonzero(rng, 100)), dst=ef.OTHER)))
    others = []
    for ihl in (5, 6, 15):                                               # empty and all-zero payloads: record 0 / sum 0
        others.append((f"e2 frag v4 ihl{ihl} pay0", frame_e2(rng, v4_fragment(rng, b"", ihl))))
    others.append(("snap frag v4 all-zero 1400", frame_snap(rng, v4_fragment(rng, bytes(1400)))))
    others.append(("e2 frag v4 all-zero 1480", frame_e2(rng, v4_fragment(rng, bytes(1480)))))
    others.append(("e2 frag v6 all-zero 64", frame_e2(rng, v6_fragment(rng, bytes(64)))))
    others.append(("snap frag v6 pay0", frame_snap(rng, v6_fragment(rng, b""))))
    mix = ef.frame_mix(rng)
    ess += [m for m in mix if m[0] in ("e2 arp", "snap arp", "snap dsap", "received 59")]
    others += mix
    for i, d in enumerate(fragment_mix(rng, 96)):                        # the packet generators' kinds, and more fragments
        fr = frame_snap if i % 2 and len(d) <= SNAP_ROOM else frame_e2
        others.append((f"{'snap' if fr is frame_snap else 'e2'} fragment_mix[{i}]", fr(rng, d)))
    # every frame that carries a fragment stays within 1514 octets (ether_frames' own mix holds one 802.3
    # frame of 1518, which the 1520-B slots still take)
    assert all(len(f) <= MAX_FRAME for _, f in ess + frags) and all(len(f) <= 1518 for _, f in others)
    return ess, frags, others


class Burst:
    """As test_gpu_ether.Burst: buf, lead, off / lens / stride / frame_len, start[i], present[i], names[i]."""


@functools.lru_cache(maxsize=None)
def burst(layout, n):
    """n frames: the essentials, then fragments and other frames alternately, shuffled by seed. `fixed`:
    1514 octets per 1536-B slot, each frame with the slot's stale octets behind it."""
    rng = random.Random(7000 + 10 * n + len(layout))
    ess, frags, others = (list(p) for p in pools())
    if layout == "fixed":                                                # (a slot holds frame_len octets)
        others = [m for m in others if len(m[1]) <= MAX_FRAME]
    rng.shuffle(frags)
    rng.shuffle(others)
    if n == 1:
        picked = [frags[0]]
    else:
        picked = ess[:n]
        i = 0
        while len(picked) < n:
            picked.append(frags[(i // 2) % len(frags)] if i % 2 == 0 else others[(i // 2) % len(others)])
            i += 1
        rng.shuffle(picked)
    b = Burst()
    b.n = n
    b.names = [nm for nm, _ in picked]
    b.off = b.lens = None
    b.stride = b.frame_len = 0
    if layout == "fixed":
        b.present = [f + rng.randbytes(MAX_FRAME - len(f)) for _, f in picked]
    else:
        b.present = [f for _, f in picked]
    if layout.startswith("packed"):
        b.lead = 0
        pos = int(layout[-1])
        b.start = []
        for f in b.present:
            b.start.append(pos)
            pos += len(f)
        b.off = np.array(b.start, np.uint64)
        b.lens = np.array([len(f) for f in b.present], np.uint16)
        size = pos
    else:
        b.stride, b.lead = (1520, 0) if layout == "slot1520" else (1536, 2)
        b.start = [i * b.stride for i in range(n)]
        if layout == "fixed":
            b.frame_len = MAX_FRAME
        else:
            b.lens = np.array([len(f) for f in b.present], np.uint16)
        size = b.lead + b.start[-1] + len(b.present[-1])
    b.buf = np.frombuffer(rng.randbytes(size), np.uint8).copy()
    for s, f in zip(b.start, b.present):
        b.buf[b.lead + s:b.lead + s + len(f)] = np.frombuffer(f, np.uint8)
    assert b.lead + b.start[-1] + len(b.present[-1]) == b.buf.size       # the last frame ends the allocation
    return b


@functools.lru_cache(maxsize=None)
def _record(dgram: bytes) -> int:
    return want_record(dgram) if dgram else 0


def expect_frames(frames, eth_cfg=0, hw=ef.HW, rx_cfg=0):
    """-> (classes, header lengths (0: no datagram), flags, actions, records as uint32 sum | len << 16)."""
    l2, hdr, fl, act = ef.expect(frames, eth_cfg, hw, rx_cfg)
    rec = np.array([_record(ef.ip_datagram(f, eth_cfg, hw)[2]) for f in frames], np.uint32)
    return l2, hdr, fl, act, rec


@functools.lru_cache(maxsize=None)
def expect(layout, n, eth_cfg=0, hw=ef.HW, rx_cfg=0):
    """expect_frames of burst(layout, n), computed once per configuration and shared."""
    out = expect_frames(burst(layout, n).present, eth_cfg, hw, rx_cfg)
    for a in out:
        a.setflags(write=False)
    return out


def mix_counts(b, eth_cfg=0, hw=ef.HW):
    """What the condition on the mix counts in burst b."""
    l2, hdr, _, _, rec = expect_frames(b.present, eth_cfg, hw)
    nz = rec != 0
    return dict(
        fragments=int(nz.sum()),
        behind_snap=int((nz & (hdr == 22)).sum()),
        walk=sum(1 for i, nm in enumerate(b.names) if nz[i] and ("walk" in nm or "(60, 130)" in nm or "(60, 1)" in nm)),
        non_ip=int((~np.isin(l2, ef.IP_CLASSES)).sum()),
        mismatch=sum(1 for i, nm in enumerate(b.names) if nm.startswith("mismatch") and rec[i] == 0 and hdr[i] == 0
                     and l2[i] in ef.IP_CLASSES),
        mismatch_names={nm for nm in b.names if nm.startswith("mismatch")},
    )
