"""Ethernet frames for the frame-level Rx burst tests (include/netcsum_mi355x.h (2b'''')): builders
around the datagrams of packets.py, a Python restatement of the reference's 802.x receive checks
(IF/net_if_802x.c:548-554, :1673-1685 frame size; :1982-2026 addresses; :2037-2050 type / length split;
:2155-2187 Ethernet II types; :2266-2352 802.3 length, LLC, SNAP) written from those lines, on octets,
independently of the C rules in include/netcsum_ether.h, and the mixes the tests run.

Received lengths: an Ethernet II frame is padded with zeros to 60 octets. An 802.3 frame shorter than
60 octets is padded to 60 (its length field keeps the LLC data's octets: the reference skips the
length check below 64 octets received); a longer one carries 4 FCS octets, so that its length field
equals the octets received - 18, which is what the reference's check assumes (:2268).
"""
from __future__ import annotations

import functools
import random
import struct

import numpy as np

import netcsum
import oracle_offload as oo
import oracle_packets as op
from packets import _ext_chain, make_packet, make_packet_v6

HW = bytes.fromhex("02a1b2c3d4e5")          # the interface's address in the tests
OTHER = bytes.fromhex("02a1b2c3d4e6")       # another station (differs in the last octet only)
OTHER_HI = bytes.fromhex("06a1b2c3d4e5")    # ... and one that differs in the first
SRC = bytes.fromhex("0250607080a0")
BCAST = b"\xff" * 6
MCAST = bytes.fromhex("01005e0000fb")
NULL = bytes(6)
T_IPV4, T_IPV6, T_ARP = 0x0800, 0x86DD, 0x0806

(ETHER_IPV4, ETHER_IPV6, SNAP_IPV4, SNAP_IPV6, ETHER_ARP, SNAP_ARP, INV_FRAME_SIZE, INV_ADDR_DEST, INV_ADDR_SRC,
 INV_ETHER_TYPE, INV_LEN_FRAME, INV_LLC_DSAP, INV_LLC_SSAP, INV_LLC_CTRL, INV_SNAP_CODE, INV_SNAP_TYPE) = range(16)
IP_CLASSES = (ETHER_IPV4, ETHER_IPV6, SNAP_IPV4, SNAP_IPV6)


# ------------------------------------------------------------------------------------- the rules, in Python
def classify(frame: bytes, eth_cfg: int = 0, hw: bytes | None = HW, length: int | None = None):
    """-> (class, header length 14 / 22 / 0) of a frame of `length` octets received (default len(frame))."""
    n = len(frame) if length is None else length
    if n < 60:                                                  # NetIF_802x_PktSizeIsValid
        return INV_FRAME_SIZE, 0
    dst, src = frame[0:6], frame[6:12]
    if hw is not None:                                          # (NULL: promiscuous, no destination check)
        if dst == BCAST:
            pass
        elif (eth_cfg & 1) and (dst[0] & 0x01):                 # NET_MCAST_RX_MODULE_EN
            pass
        elif dst != hw:
            return INV_ADDR_DEST, 0
    if src == NULL or src == BCAST:                             # NetIF_802x_AddrHW_IsValid
        return INV_ADDR_SRC, 0
    (tl,) = struct.unpack("!H", frame[12:14])
    by_type = {T_IPV4: 0, T_IPV6: 1, T_ARP: 2}
    if tl > 1500:                                               # Ethernet II
        k = by_type.get(tl)
        return ((ETHER_IPV4, ETHER_IPV6, ETHER_ARP)[k], 14) if k is not None else (INV_ETHER_TYPE, 0)
    if n >= 64 and tl != ((n - 14 - 4) & 0xFFFF):               # IEEE 802.3 length, FCS assumed present
        return INV_LEN_FRAME, 0
    if frame[14] != 0xAA:
        return INV_LLC_DSAP, 0
    if frame[15] != 0xAA:
        return INV_LLC_SSAP, 0
    if frame[16] != 0x03:
        return INV_LLC_CTRL, 0
    if frame[17] or frame[18] or frame[19]:
        return INV_SNAP_CODE, 0
    k = by_type.get(struct.unpack("!H", frame[20:22])[0])
    return ((SNAP_IPV4, SNAP_IPV6, SNAP_ARP)[k], 22) if k is not None else (INV_SNAP_TYPE, 0)


def ip_datagram(frame: bytes, eth_cfg: int = 0, hw: bytes | None = HW, length: int | None = None):
    """The octets the IP checksum pass is to see for this frame: frame[hdr:length] for an IP class whose
    version nibble is the one the frame type names, else b"" (ARP, INV_*, type / version mismatch)."""
    n = len(frame) if length is None else length
    cls, hdr = classify(frame, eth_cfg, hw, n)
    if cls not in IP_CLASSES:
        return cls, hdr, b""
    v6 = frame[hdr] >> 4 == 6
    if v6 != (cls in (ETHER_IPV6, SNAP_IPV6)):
        return cls, hdr, b""
    return cls, hdr, bytes(frame[hdr:n])


@functools.lru_cache(maxsize=None)
def ip_verdict(dgram: bytes, rx_cfg: int = 0):
    """(flags, action) RxBurst gives a datagram: the packet oracle's verdict and the action of it."""
    f = op.rx_validate_ip(dgram)
    return f, netcsum.rx_action(f, oo.transport_proto(dgram), len(dgram) > 0 and dgram[0] >> 4 == 6, rx_cfg)


def expect(frames, eth_cfg=0, hw=HW, rx_cfg=0):
    """Per frame (the octets received): class, header length, flags, action, as uint8 / int arrays."""
    l2, hdr, fl, act = [], [], [], []
    for fr in frames:
        c, h, d = ip_datagram(fr, eth_cfg, hw)
        f, a = ip_verdict(d, rx_cfg) if d else (netcsum.PKT_MALFORMED, netcsum.RX_DELIVER)
        l2.append(c), hdr.append(h if d else 0), fl.append(f), act.append(a)
    return np.array(l2, np.uint8), np.array(hdr, np.int64), np.array(fl, np.uint8), np.array(act, np.uint8)


# ------------------------------------------------------------------------------------------ frame builders
def ether2(dgram: bytes, etype: int = T_IPV4, dst: bytes = HW, src: bytes = SRC) -> bytes:
    f = dst + src + struct.pack("!H", etype) + dgram
    return f + bytes(max(0, 60 - len(f)))


def snap(dgram: bytes, etype: int = T_IPV4, dst: bytes = HW, src: bytes = SRC, dsap=0xAA, ssap=0xAA, ctrl=0x03,
         code=b"\0\0\0", length_delta: int = 0, rng: random.Random | None = None) -> bytes:
    body = bytes([dsap, ssap, ctrl]) + code + struct.pack("!H", etype) + dgram
    f = dst + src + struct.pack("!H", (len(body) + length_delta) & 0xFFFF) + body
    if len(f) < 60:
        return f + bytes(60 - len(f))                           # 60 octets received: no length check
    return f + (rng.randbytes(4) if rng else b"\xde\xad\xbe\xef")   # the FCS octets


def _tcp4(rng, payload, kind="tcp"):
    """An IPv4/TCP datagram with IHL 5 and a 20-octet TCP header (checksum field at +36)."""
    while True:
        p = make_packet(rng, kind, payload=payload)
        if p[0] == 0x45 and p[32] >> 4 == 5:
            return p


def _udp4_tiny(rng):
    """IPv4/UDP, IHL 5, 5 octets of payload: 33 octets, so that an 802.3 frame of it is padded to 60."""
    while True:
        p = make_packet(rng, "udp", payload=5)
        if p[0] == 0x45:
            return p


def _tcp6(rng, payload):
    while True:
        p = make_packet_v6(rng, "tcp", payload=payload)
        if p[52] >> 4 == 5:
            return p


def _flip(b: bytes, k: int, mask: int = 0x01) -> bytes:
    x = bytearray(b)
    x[k] ^= mask
    return bytes(x)


def v6_ext_chain(rng, units_dest: int, payload: int) -> bytes:
    """IPv6: Hop-by-Hop (8 octets), Destination Options (units_dest * 8 octets), TCP — finalized."""
    body = _tcp6(rng, payload)[40:]
    nh, ext = _ext_chain(rng, [(0, 1), (60, units_dest)], 6)
    hdr = struct.pack("!IHBB16s16s", (6 << 28) | rng.getrandbits(20), len(ext) + len(body), nh, 64, rng.randbytes(16),
                      rng.randbytes(16))
    return op.tx_finalize_v6(hdr + ext + body)[0]


def arp_request(rng) -> bytes:
    return struct.pack("!HHBBH", 1, T_IPV4, 6, 4, 1) + SRC + rng.randbytes(4) + NULL + rng.randbytes(4)


def frame_mix(rng: random.Random):
    """[(name, frame octets as received)]: at least one frame of every row the feature distinguishes."""
    m = []
    add = lambda name, f: m.append((name, bytes(f)))
    t4, t6 = _tcp4(rng, 700), _tcp6(rng, 333)
    # Ethernet II, IPv4
    add("e2 v4 tcp", ether2(t4))
    add("e2 v4 tcp bad l4", ether2(_flip(t4, 36)))
    add("e2 v4 tcp bad ip csum", ether2(make_packet(rng, "corrupt_ip", payload=211)))
    add("e2 v4 udp0", ether2(make_packet(rng, "udp0", payload=97)))
    add("e2 v4 icmp", ether2(make_packet(rng, "icmp", payload=56)))
    add("e2 v4 igmp", ether2(make_packet(rng, "igmp")))
    add("e2 v4 frag", ether2(make_packet(rng, "frag", payload=808)))
    ack = _tcp4(rng, 0)
    assert len(ack) == 40
    add("e2 v4 ack padded", ether2(ack))
    add("e2 v4 tcp 1500", ether2(_tcp4(rng, 1460)))
    # Ethernet II, IPv6
    add("e2 v6 tcp", ether2(t6, T_IPV6))
    add("e2 v6 udp", ether2(make_packet_v6(rng, "udp", payload=512), T_IPV6))
    add("e2 v6 icmp", ether2(make_packet_v6(rng, "icmp_echo", payload=64), T_IPV6))
    add("e2 v6 hbh+dest", ether2(v6_ext_chain(rng, 2, 100), T_IPV6))
    add("e2 v6 hbh+dest long (walk)", ether2(v6_ext_chain(rng, 131, 200), T_IPV6))
    # 802.3 + LLC/SNAP
    add("snap v4 tcp", snap(t4, rng=rng))
    add("snap v4 tcp bad l4", snap(_flip(t4, 36, 0x40), rng=rng))
    add("snap v6 tcp", snap(t6, T_IPV6, rng=rng))
    add("snap v6 tcp bad l4", snap(_flip(t6, 56, 0x02), T_IPV6, rng=rng))
    add("snap arp", snap(arp_request(rng), T_ARP))
    add("snap v4 ack", snap(ack, rng=rng))
    tiny = _udp4_tiny(rng)
    add("snap v4 udp padded to 60", snap(tiny))
    add("e2 arp", ether2(arp_request(rng), T_ARP))
    # frame types
    for t in (0x8035, 0x8100, 0x88CC, 1501, 1535, 0xFFFF):
        add(f"e2 type {t:#06x}", ether2(t4, t))
    f1500 = bytearray(snap(rng.randbytes(1500 - 8), rng=rng))           # type/length word 1500: the SNAP path
    assert struct.unpack("!H", f1500[12:14])[0] == 1500
    add("len 1500 (snap path, v4 garbage)", f1500)
    # SNAP with one field wrong
    add("snap dsap", snap(t4, dsap=0xAB, rng=rng))
    add("snap ssap", snap(t4, ssap=0x2A, rng=rng))
    add("snap ctrl", snap(t4, ctrl=0x13, rng=rng))
    for k in range(3):
        add(f"snap code[{k}]", snap(t4, code=bytes(0x80 if j == k else 0 for j in range(3)), rng=rng))
    add("snap type", snap(t4, 0x8035, rng=rng))
    add("snap dsap+ssap", snap(t4, dsap=0, ssap=0, rng=rng))
    # SNAP frame length
    add("snap len+1", snap(t4, length_delta=1, rng=rng))
    add("snap len-1", snap(t4, length_delta=-1, rng=rng))
    add("snap len+1 dsap", snap(t4, length_delta=1, dsap=0, rng=rng))   # the length check comes first
    short = snap(tiny, length_delta=6)                                  # (no length 60 .. 64 - 18 makes it right)
    assert len(short) == 60 and len(snap(arp_request(rng), T_ARP, length_delta=-3)) == 60
    add("snap arp 60 octets, wrong len field", snap(arp_request(rng), T_ARP, length_delta=-3))
    add("snap 60 octets, wrong len field", short)
    add("snap 63 octets, wrong len field", short + bytes(3))
    add("snap 64 octets, wrong len field", short + bytes(4))
    # received length
    full = ether2(t4)
    for n in (0, 14, 59, 60):
        add(f"received {n}", full[:n])
    add("received 60 v4 garbage tail", ether2(ack)[:60])
    # destination address
    for name, d in (("bcast", BCAST), ("mcast", MCAST), ("hw", HW), ("other", OTHER), ("other hi", OTHER_HI)):
        add(f"dst {name} v4", ether2(t4, dst=d))
        add(f"dst {name} snap v6 bad l4", snap(_flip(t6, 57), T_IPV6, dst=d, rng=rng))
    # source address
    add("src null", ether2(t4, src=NULL))
    add("src bcast", ether2(t4, src=BCAST))
    add("src almost null", ether2(t4, src=bytes(5) + b"\x01"))
    add("src almost bcast", ether2(t4, src=b"\x7f" + b"\xff" * 5))
    # two checks failing at once: the earlier one wins
    add("dst other + src null", ether2(t4, dst=OTHER, src=NULL))
    add("src bcast + bad type", ether2(t4, 0x8100, src=BCAST))
    add("src null + snap dsap", snap(t4, dsap=1, src=NULL, rng=rng))
    # type / version mismatch
    add("type v4, nibble 6", ether2(t6, T_IPV4))
    add("type v6, nibble 4", ether2(t4, T_IPV6))
    add("type v6, nibble 7", ether2(_flip(t6, 0, 0x10), T_IPV6))
    add("type v4, nibble 5", ether2(_flip(t4, 0, 0x10), T_IPV4))
    add("snap type v4, nibble 6", snap(t6, T_IPV4, rng=rng))
    add("snap type v6, nibble 4", snap(t4, T_IPV6, rng=rng))
    return m


def fixed_len_mix(rng: random.Random, frame_len: int = 1514):
    """Slot contents of frame_len octets for a ring without received lengths: the mix's frames with the
    slot's stale octets behind them, and 802.3 frames whose length field the rule accepts at frame_len."""
    m = [(name, f + rng.randbytes(frame_len - len(f))) for name, f in frame_mix(rng) if len(f) <= frame_len]
    room = frame_len - 18 - 8                                        # LLC data octets - LLC/SNAP = the datagram's
    t4, t6 = _tcp4(rng, room - 40), _tcp6(rng, room - 60)
    for name, f in (("snap v4 tcp", snap(t4, rng=rng)), ("snap v4 tcp bad l4", snap(_flip(t4, 36), rng=rng)),
                    ("snap v6 tcp", snap(t6, T_IPV6, rng=rng)), ("snap v6 tcp bad l4", snap(_flip(t6, 56), T_IPV6, rng=rng)),
                    ("snap arp", snap(arp_request(rng) + bytes(room - 28), T_ARP, rng=rng)),
                    ("snap dsap", snap(t4, dsap=0xAB, rng=rng)), ("snap ssap", snap(t4, ssap=0, rng=rng)),
                    ("snap ctrl", snap(t4, ctrl=0, rng=rng)), ("snap code", snap(t4, code=b"\0\x01\0", rng=rng)),
                    ("snap type", snap(t4, 0x8100, rng=rng))):
        assert len(f) == frame_len, (name, len(f))
        m.append((f"fixed {name}", f))
    return m


def random_frame(rng: random.Random) -> bytes:
    """Random octets, 0-1600 of them, with octets 0-22 biased towards the values that reach each check."""
    n = rng.choice([rng.randint(0, 1600), rng.randint(56, 68), rng.randint(0, 1600)])
    f = bytearray(rng.randbytes(n))

    def put(k, b):
        f[k:k + len(b)] = b
        del f[n:]

    r = rng.random
    put(0, rng.choice([HW, HW, HW, BCAST, MCAST, OTHER, OTHER_HI, rng.randbytes(6)]))
    if r() < 0.1:
        put(6, rng.choice([NULL, BCAST, bytes(5) + b"\x01", b"\xff" * 5 + b"\xfe"]))
    c = r()
    if c < 0.3:
        put(12, struct.pack("!H", rng.choice([T_IPV4, T_IPV6, T_ARP, 0x8035, 0x8100, 1501, 1536])))
    elif c < 0.9:
        tl = rng.choice([(n - 18) & 0xFFFF, (n - 18) & 0xFFFF, (n - 18) & 0xFFFF, (n - 17) & 0xFFFF, 1500, 0, rng.randint(0, 1500)])
        put(12, struct.pack("!H", tl if tl <= 1500 else 1500))
        for k, good in ((14, 0xAA), (15, 0xAA), (16, 0x03), (17, 0), (18, 0), (19, 0)):
            if r() < 0.9:
                put(k, bytes([good]))
        if r() < 0.9:
            put(20, struct.pack("!H", rng.choice([T_IPV4, T_IPV6, T_ARP, T_ARP + 1])))
    if r() < 0.5:
        put(rng.choice([14, 22]), bytes([rng.choice([0x45, 0x60, 0x75, 0x4F])]))
    return bytes(f)
