"""Ethernet frames for the frame-level Tx burst tests (include/netcsum_mi355x.h (2b''''')): a Python
restatement of the Tx frame rule written from the reference's transmit path (IF/net_if_802x.c:2643-2778:
NetIF_802x_Tx writes an Ethernet II header — destination, the interface's own source address, the type of
the protocol above, :2691-2761 — and NetIF_802x_TxPktPrepareFrame pads the frame with zeros to 60 octets,
:2764-2778), on octets, independently of the C rule in include/netcsum_ether.h; a builder of the frames a
driver's Tx queue holds under the checksum-offload flags; and what a Tx burst must leave of each.

A frame: a datagram of packets.make_packet / make_packet_v6 (the kinds of test_gpu_offload._tx_frames), put
into the stack's offload form (oracle_offload.tx_stack_offload: 0 in the fields left to the offload, the
UDP placeholder 0xFFFF, 0 for "no UDP checksum"), behind ether_frames.ether2's header. The expected frame
is frame[:14] + the Tx adapter's rule on frame[14:len] (oracle_offload.tx_burst_model) for an IP class
whose datagram's version nibble is the one the type names, and the frame unchanged otherwise.
"""
from __future__ import annotations

import functools
import random
import struct

import numpy as np

import ether_frames as ef
import oracle_offload as oo
import oracle_packets as op
from packets import make_packet, make_packet_v6

DST = bytes.fromhex("02c0ffee0001")         # what ARP resolved for the next hop (arbitrary)
V4_KINDS = ["tcp", "udp", "udp", "icmp", "igmp", "other", "frag"]
V6_KINDS = ["tcp", "udp", "udp", "icmp_echo", "icmp_err", "icmp_nd", "other", "ext_ok", "ext_frag", "ext_long"]
V6_LOOPBACK_UNSURE = ("icmp_err", "ext_ok", "ext_long", "ext_frag")   # the Tx and Rx oracles disagree on some


# ------------------------------------------------------------------------------------- the rule, in Python
def classify(frame: bytes, length: int | None = None):
    """-> (class, header length 14 / 0) of a frame of `length` octets to transmit (default len(frame))."""
    n = len(frame) if length is None else length
    if n < 60:                                                  # not NetIF_802x_TxPktPrepareFrame's work
        return ef.INV_FRAME_SIZE, 0
    (t,) = struct.unpack("!H", frame[12:14])                    # the only octets that decide
    if t == ef.T_IPV4:
        return ef.ETHER_IPV4, 14
    if t == ef.T_IPV6:
        return ef.ETHER_IPV6, 14
    if t == ef.T_ARP:
        return ef.ETHER_ARP, 14
    return ef.INV_ETHER_TYPE, 0


def datagram(frame: bytes):
    """(class, the octets the Tx checksum pass is given: frame[14:] or b"")."""
    cls, _ = classify(frame)
    if cls == ef.ETHER_IPV4 and frame[14] >> 4 != 6:
        return cls, bytes(frame[14:])
    if cls == ef.ETHER_IPV6 and frame[14] >> 4 == 6:
        return cls, bytes(frame[14:])
    return cls, b""


@functools.lru_cache(maxsize=None)
def tx_model(dgram: bytes):
    """(finalized octets, flags) of TxBurst on one datagram: oracle_offload.tx_burst_model with the flags
    the same oracle call gives (a UDP field of 0 means "no checksum" and stays 0)."""
    v6 = len(dgram) and dgram[0] >> 4 == 6
    if v6:
        p = op._parse6(dgram)
        udp_none = p is not None and not p[0] and p[3] == 17 and dgram[p[1] + 6:p[1] + 8] == b"\x00\x00"
    else:
        p = op._parse(dgram)
        udp_none = p is not None and not p[2] and p[3] == 17 and dgram[p[0] + 6:p[0] + 8] == b"\x00\x00"
    fin, fl = op.tx_finalize_ip(dgram, udp_tx_csum=not udp_none)
    assert fin == oo.tx_burst_model(dgram)
    return fin, fl


def expect(frames):
    """Per frame: class (uint8 array), flags (uint8 array), the frame as the burst must leave it."""
    l2, fl, out = [], [], []
    for f in frames:
        c, d = datagram(f)
        fin, g = tx_model(d)
        assert len(fin) == len(d)
        l2.append(c), fl.append(g), out.append(bytes(f[:14]) + fin if d else bytes(f))
    return np.array(l2, np.uint8), np.array(fl, np.uint8), out


# ------------------------------------------------------------------------------------------ frame builders
def ip_frame(rng: random.Random, v6: bool, kind: str, payload: int, csum: bool = True):
    """(name, the frame in the driver's queue, the frame the reference builds with the offload flags off);
    at most 1514 octets (a datagram that came out longer — options, a long chain — is drawn again)."""
    while True:
        pkt = make_packet_v6(rng, kind, payload=payload) if v6 else make_packet(rng, kind, payload=payload)
        if len(pkt) <= 1500:
            break
        payload = payload * 3 // 4
    etype = ef.T_IPV6 if v6 else ef.T_IPV4
    name = f"{'v6' if v6 else 'v4'} {kind}"
    return (name, ef.ether2(oo.tx_stack_offload(pkt, csum), etype, dst=DST, src=ef.HW),
            ef.ether2(op.tx_finalize_ip(pkt, csum)[0], etype, dst=DST, src=ef.HW))


def special_frames(rng: random.Random):
    """[(name, frame)]: the rows the Tx rule and the byte contract distinguish."""
    m = []
    add = lambda name, f: m.append((name, bytes(f)))
    t4 = oo.tx_stack_offload(ef._tcp4(rng, 300))
    t6 = oo.tx_stack_offload(ef._tcp6(rng, 222))
    add("arp", ef.ether2(ef.arp_request(rng), ef.T_ARP, dst=ef.BCAST, src=ef.HW))
    add("type 0x88cc", ef.ether2(t4, 0x88CC, dst=DST, src=ef.HW))
    add("type 0x8100", ef.ether2(t4, 0x8100, dst=DST, src=ef.HW))
    add("snap v4 tcp", ef.snap(t4, dst=DST, src=ef.HW, rng=rng))           # the 802.3 length form: never sent
    add("snap v4 udp 60",ef.snap(oo.tx_stack_offload(ef._udp4_tiny(rng)), dst=DST, src=ef.HW))
    ack = oo.tx_stack_offload(ef._tcp4(rng, 0))
    full = ef.ether2(ack, dst=DST, src=ef.HW)
    assert len(full) == 60 and len(ack) == 40
    add("runt 59", full[:59])
    add("exactly 60 (ack, 6 octets of padding)", full)
    add("type v4, nibble 6", ef.ether2(t6, ef.T_IPV4, dst=DST, src=ef.HW))
    add("type v6, nibble 4", ef.ether2(t4, ef.T_IPV6, dst=DST, src=ef.HW))
    add("v4 udp, field 0", ef.ether2(oo.tx_stack_offload(make_packet(rng, "udp", payload=77), False), dst=DST, src=ef.HW))
    add("v6 udp, field 0", ef.ether2(oo.tx_stack_offload(make_packet_v6(rng, "udp", payload=78), False), ef.T_IPV6,
                                     dst=DST, src=ef.HW))
    add("v6 ext_long", ip_frame(rng, True, "ext_long", 200)[1])
    big = ef.ether2(oo.tx_stack_offload(ef._tcp4(rng, 1460)), dst=ef.MCAST, src=ef.HW)
    assert len(big) == 1514
    add("v4 tcp 1514", big)
    add("src null (no address check)", ef.ether2(t4, dst=DST, src=ef.NULL))
    return m


def frame_mix(rng: random.Random, n_ip: int = 120, max_payload: int = 1400, loopback_only: bool = False):
    """[(name, frame)]: n_ip IP frames over the kinds, alternating versions, a fifth of the UDP ones with
    the checksum off, and the special rows (without them and the kinds the oracles disagree on when
    loopback_only)."""
    m = []
    for i in range(n_ip):
        v6 = not (i % 2)
        kinds = [k for k in V6_KINDS if not (loopback_only and k in V6_LOOPBACK_UNSURE)] if v6 else V4_KINDS
        nm, f, _ = ip_frame(rng, v6, rng.choice(kinds), rng.choice([rng.randint(0, 40), rng.randint(0, max_payload)]),
                            rng.random() < 0.8)
        m.append((nm, f))
    return m if loopback_only else m + special_frames(rng)


class Ring:
    """buf: the allocation; lead: the base pointer's offset in it; off / lens / stride / frame_len: the
    call's arguments; start[i]: frame i's offset from the base; frames[i]: its octets; guard: octets
    behind the last frame that no call may touch."""


GUARD = 96


@functools.lru_cache(maxsize=None)
def ring(layout: str, n: int, seed: int = 0, loopback_only: bool = False) -> Ring:
    """packed: off + lens, random gaps of 0-9 octets so that starts hit every residue mod 4 and straddle
    64-B sectors; slot0 / slot2: 1520-B slots with the frame at +0 / +2, lens only; fixed: 2048-B slots
    of 1514 octets (frame, then the slot's stale octets), neither off nor lens."""
    rng = random.Random(1000 * n + 7 * len(layout) + seed)
    mix = list(_mix(loopback_only))
    rng.shuffle(mix)
    if n == 1:
        mix = [m for m in mix if m[0].startswith("v4 udp")][:1]
    picked = [mix[i % len(mix)] for i in range(n)]
    rng.shuffle(picked)
    b = Ring()
    b.n, b.names = n, [nm for nm, _ in picked]
    b.frames = [f for _, f in picked]
    b.off = b.lens = None
    b.stride = b.frame_len = b.lead = 0
    assert all(len(f) <= 1514 for f in b.frames)                        # (frames never overlap)
    if layout == "packed":
        pos, b.start = rng.randint(0, 3), []
        for f in b.frames:
            b.start.append(pos)
            pos += len(f) + rng.randint(0, 9)
        b.off = np.array(b.start, np.uint64)
        b.lens = np.array([len(f) for f in b.frames], np.uint16)
        size = b.start[-1] + len(b.frames[-1])
    elif layout in ("slot0", "slot2"):
        b.stride, b.lead = 1520, int(layout[-1])
        b.start = [i * b.stride for i in range(n)]
        b.lens = np.array([len(f) for f in b.frames], np.uint16)
        size = b.lead + n * b.stride
    else:
        assert layout == "fixed"
        b.stride, b.frame_len = 2048, 1514
        b.start = [i * b.stride for i in range(n)]
        b.frames = [f + rng.randbytes(1514 - len(f)) for f in b.frames]   # the frame is the slot's 1514 octets
        size = (n - 1) * b.stride + 1514
    b.buf = np.frombuffer(rng.randbytes(size + GUARD), np.uint8).copy()    # stale octets in gaps and guard
    for s, f in zip(b.start, b.frames):
        b.buf[b.lead + s:b.lead + s + len(f)] = np.frombuffer(f, np.uint8)
    b.want_l2, b.want_fl, b.want_frames = expect(b.frames)
    b.want = b.buf.copy()
    for s, f in zip(b.start, b.want_frames):
        b.want[b.lead + s:b.lead + s + len(f)] = np.frombuffer(f, np.uint8)
    return b


@functools.lru_cache(maxsize=None)
def _mix(loopback_only):
    return tuple(frame_mix(random.Random(31 + loopback_only), loopback_only=loopback_only))


def call_args(b: Ring, to):
    kw = dict(stride=b.stride, frame_len=b.frame_len)
    if b.off is not None:
        kw["off"] = to(b.off.astype(np.int64))
    if b.lens is not None:
        kw["lens"] = to(b.lens.view(np.int16))
    return kw
