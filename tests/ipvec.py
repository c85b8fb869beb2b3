"""Reader of tests/golden/reference_ip_vectors.json: what the reference's own NetIPv4_Rx (IP/IPv4/net_ipv4.c
with net_icmpv4.c, net_igmp.c, Source/net_udp.c, net_tcp.c over net_util.c, built by oracle/Makefile `ref`
behind the stubs and recording checksum wrappers of oracle/ref/glue_ipv4.c) did with each datagram,
recorded by tests/golden/make_ip_vectors.py. The recorder, the CPU tests (test_ip_reference_cpu.py) and
the GPU tests (test_gpu_ip_reference.py) all build their datagrams here, so a case means the same octets
to each of them. Nothing here computes an expected value, and nothing here uses the parse or verdict
rules of this project (netcsum_ipparse.h, oracle_packets.py): the checksums below are the plain RFC 1071
sum, used only to BUILD datagrams whose fields are right or wrong in a chosen way.

Datagrams start at the IP header. An explicit case is {"name", "n": octets received, "head": hex of its
first min(n, 96) octets}; octets 96 .. n-1 are hashlib.shake_256("ip/tail/" + name).digest(n - 96). The
generated set is `count` datagrams drawn by gen_dgram() from one ShakeRng(seed) stream, in order;
"sha256" is over every datagram's 2-octet little-endian length followed by its octets. No datagram
depends on the random module. Every datagram is handed to the reference as a frame from a remote host,
flagged as a link-layer broadcast exactly when rx_bcast() says so (its IP destination is a class D / E or
the subnet's broadcast address: what a sender's link layer would have done).

The interface the reference was given: one host address HOST / MASK, one joined group GROUP.

Outcomes. fixture["outcomes"] is the table of distinct records (error returned, stubs that ran, discards,
whether the buffer was queued as a fragment, the non-zero receive error counters by name, and per
checksum call its function, protocol type, offset and result); fixture["out"][lib]["outcome"] holds one
index into it per datagram (explicit cases first, then the generated set) and ["calls"] per datagram and
call the length and pseudo-header octets, see pack_calls(); the second library is stored as its
differences from "ipv4" ([datagram, index] pairs; calls null where they are the same).
"""
from __future__ import annotations

import base64
import hashlib
import json
import os
import struct
import zlib

import numpy as np

import refvec
from ethervec import ShakeRng

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_ip_vectors.json")
REF_DIR = os.path.join(os.path.dirname(HERE), "oracle", "_ref")
LIBS = ("ipv4", "udpdis")                   # recorded; "ipv4_O0" is the recorder's twin of "ipv4"
LIB_FILES = {"ipv4": "libipv4_ref.so", "ipv4_O0": "libipv4_ref_O0.so", "udpdis": "libipv4_ref_udpdis.so"}
HEAD = 96                                   # octets of an explicit case stored as hex

HOST = bytes([10, 1, 2, 3])
MASK = bytes([255, 255, 255, 0])
SUBNET_BCAST = bytes([10, 1, 2, 255])
GROUP = bytes([239, 1, 2, 3])
ALL_HOSTS = bytes([224, 0, 0, 1])
BCAST = b"\xff" * 4
SRC = bytes([10, 1, 2, 77])
SRC_FAR = bytes([192, 0, 2, 9])
FOREIGN = bytes([10, 1, 2, 4])
FN_NAMES = ("hdr_calc", "hdr_verify", "data_calc", "data_verify")
P_TCP, P_UDP, P_ICMP, P_IGMP = 6, 17, 1, 2


def libs_available() -> bool:
    return all(os.path.exists(os.path.join(REF_DIR, f)) for f in LIB_FILES.values())


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def rx_bcast(d: bytes) -> int:
    return int(len(d) >= 20 and (d[16] >= 224 or d[16:20] == SUBNET_BCAST))


# ------------------------------------------------------------------------------------- building datagrams
def csum16(b: bytes) -> int:
    """RFC 1071: the complement of the one's-complement sum of b's big-endian 16-bit words."""
    if len(b) & 1:
        b = b + b"\0"
    s = sum(struct.unpack("!%dH" % (len(b) // 2), b))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def ip_header(proto, src, dst, payload_len, ihl=5, opts=b"", flags_frag=0, ident=0x1234, ttl=64, tos=0, ver=4, tot=None):
    """An IPv4 header of ihl words (opts padded with EOL octets or cut to fit), checksum field zero."""
    opts = (opts + bytes(40))[:4 * (ihl - 5)] if ihl > 5 else b""
    tot = 4 * ihl + payload_len if tot is None else tot
    return struct.pack("!BBHHHBBH4s4s", (ver << 4) | (ihl & 0xF), tos, tot & 0xFFFF, ident, flags_frag, ttl, proto, 0, src, dst) + opts


def finalize(d: bytearray, udp_sum=True):
    """Store the right IPv4 header checksum and, for TCP / UDP / ICMP / IGMP behind a header of >= 20 octets
    that fits, the right transport checksum over [IHL * 4, len(d)) with the pseudo-header length len(d) -
    IHL * 4. (Builds inputs; judges nothing.)"""
    if len(d) < 20:
        return
    hl = (d[0] & 0xF) * 4
    if hl < 20 or hl > len(d):
        hl = 20
    d[10:12] = b"\0\0"
    d[10:12] = struct.pack("!H", csum16(bytes(d[:hl])))
    proto, l4 = d[9], len(d) - hl
    fld = {P_TCP: 16, P_UDP: 6, P_ICMP: 2, P_IGMP: 2}.get(proto)
    if fld is None or l4 < fld + 2:
        return
    d[hl + fld:hl + fld + 2] = b"\0\0"
    if proto == P_UDP and not udp_sum:
        return
    pseudo = bytes(d[12:20]) + struct.pack("!BBH", 0, proto, l4) if proto in (P_TCP, P_UDP) else b""
    c = csum16(pseudo + bytes(d[hl:]))
    if proto == P_UDP and c == 0:
        c = 0xFFFF
    d[hl + fld:hl + fld + 2] = struct.pack("!H", c)


def tcp_hdr(sport=40000, dport=80, doff=5, flags=0x10, seq=1, ack=2, win=512):
    return struct.pack("!HHIIBBHHH", sport, dport, seq, ack, (doff & 0xF) << 4, flags, win, 0, 0)


def udp_hdr(length, sport=40000, dport=5353):
    return struct.pack("!HHHH", sport, dport, length & 0xFFFF, 0)


def icmp_hdr(typ, code=0, rest=b"\x00\x07\x00\x01"):
    return struct.pack("!BBH", typ, code, 0) + rest


def icmp_err_body():
    """What an ICMPv4 error message quotes: an IP header and 8 octets of its payload."""
    inner = bytearray(ip_header(P_UDP, HOST, SRC_FAR, 8) + udp_hdr(8))
    inner[10:12] = struct.pack("!H", csum16(bytes(inner[:20])))
    return bytes(inner)


def igmp_msg(typ, group, max_resp=0):
    return struct.pack("!BBH4s", typ, max_resp, 0, group)


OPT_PAD = {5: b""}
for _ihl in range(6, 16):                   # options the reference accepts: NOP padding and an EOL, or ...
    OPT_PAD[_ihl] = b"\x01" * (4 * (_ihl - 5) - 1) + b"\x00"


def opt_record_route(ihl):
    """... a well-formed, empty record-route option filling the option area: type 7, pointer 4, and a length
    that is a multiple of 4 (the reference walks options in 4-octet words and accepts no other length)."""
    n = 4 * (ihl - 5)
    return bytes([7, n, 4]) + bytes(n - 3)


def opt_timestamp(ihl):
    n = 4 * (ihl - 5)
    ln = 4 + 4 * ((n - 4) // 4)
    return bytes([68, ln, 5, 0]) + bytes(ln - 4) + bytes(n - ln)


KINDS = ("tcp", "udp", "udp0", "echo_req", "echo_reply", "icmp_err", "igmp_query", "igmp_report", "other")


def transport(kind, payload: bytes):
    """-> (protocol number, transport octets with zero checksum, usual destination)."""
    if kind == "tcp":
        return P_TCP, tcp_hdr() + payload, HOST
    if kind in ("udp", "udp0"):
        return P_UDP, udp_hdr(8 + len(payload)) + payload, HOST
    if kind == "echo_req":
        return P_ICMP, icmp_hdr(8) + payload, HOST
    if kind == "echo_reply":
        return P_ICMP, icmp_hdr(0) + payload, HOST
    if kind == "icmp_err":
        return P_ICMP, icmp_hdr(3, 1, bytes(4)) + icmp_err_body() + payload, HOST
    if kind == "igmp_query":
        return P_IGMP, igmp_msg(0x11, bytes(4), 100) + payload, ALL_HOSTS
    if kind == "igmp_report":
        return P_IGMP, igmp_msg(0x12, GROUP) + payload, GROUP
    return 47, payload, HOST


def build(kind, payload, src=SRC, dst=None, ihl=5, opts=None, tail=b"", **ip_kw):
    """A well-formed datagram of that kind, checksums not yet stored; octets from HEAD on replaced by `tail`."""
    proto, l4, usual = transport(kind, payload)
    d = bytearray(ip_header(proto, src, usual if dst is None else dst, len(l4), ihl, OPT_PAD[ihl] if opts is None else opts, **ip_kw) + l4)
    if tail:
        assert len(d) == HEAD + len(tail)
        d[HEAD:] = tail
    return d


# ------------------------------------------------------------------------------------- explicit cases
def tail_bytes(name: str, n: int) -> bytes:
    return refvec.shake("ip/tail/" + name, n - HEAD) if n > HEAD else b""


def case_dgram(case) -> bytes:
    head = bytes.fromhex(case["head"])
    assert len(head) == min(case["n"], HEAD), case["name"]
    return head + tail_bytes(case["name"], case["n"])


# ------------------------------------------------------------------------------------- generated datagrams
def gen_dgram(rng: ShakeRng) -> bytes:
    """One datagram of a random kind, mostly short, then at most one fault of a random sort: a flipped bit
    (header, addresses, transport part), a wrong structural field, or a wrong received length."""
    kind = rng.choice(KINDS + ("tcp", "udp", "udp", "udp0", "udp0", "echo_req", "igmp_report", "igmp_query"))
    plen = (rng.randint(0, 3), rng.randint(0, 64), rng.randint(0, 64), rng.randint(0, 300))[rng.below(4)]
    ihl = 5 if rng.chance(700) else rng.randint(6, 15)
    opts = None
    if ihl > 5:
        opts = (OPT_PAD[ihl], OPT_PAD[ihl], opt_record_route(ihl), opt_timestamp(ihl) if ihl > 6 else OPT_PAD[ihl],
                rng.randbytes(4 * (ihl - 5)))[rng.below(5)]
    dst = None
    c = rng.below(100)
    if c < 6 and kind in ("udp", "udp0"):
        dst = rng.choice([BCAST, SUBNET_BCAST, GROUP])
    elif c < 9:
        dst = rng.choice([FOREIGN, bytes([224, 9, 9, 9]), bytes([10, 1, 3, 3])])
    src = rng.choice([SRC, SRC, SRC, SRC_FAR])
    if rng.chance(30):
        src = rng.choice([bytes(4), bytes([127, 0, 0, 1]), BCAST, GROUP, SUBNET_BCAST, bytes([240, 0, 0, 1])])
    d = build(kind, rng.randbytes(plen), src=src, dst=dst, ihl=ihl, opts=opts, ident=rng.below(65536))
    hl, n = 4 * ihl, len(d)
    fault = rng.below(100)
    udp_sum = kind != "udp0"
    received = n
    if fault < 30:                                              # none
        finalize(d, udp_sum)
    elif fault < 58:                                            # a transport bit (if there is a transport part)
        finalize(d, udp_sum)
        if n > hl:
            p = rng.choice([hl + rng.below(n - hl), n - 1, hl + rng.below(min(n - hl, 20))])
            d[p] ^= 1 << rng.below(8)
    elif fault < 66:                                            # an address, protocol or length bit: pseudo-header inputs
        finalize(d, udp_sum)
        p = rng.choice([12 + rng.below(8), 9, 3])
        d[p] ^= 1 << rng.below(8)
        if rng.chance(600):                                     # ... with the IP header checksum made right again
            d[10:12] = b"\0\0"
            d[10:12] = struct.pack("!H", csum16(bytes(d[:hl])))
    elif fault < 74:                                            # an IP header bit
        finalize(d, udp_sum)
        d[rng.below(hl)] ^= 1 << rng.below(8)
    elif fault < 90:                                            # a structural field, checksums right for the rest
        good_l4 = rng.chance(500)
        if not good_l4 and n > hl + 4:
            d[n - 1] ^= 0x10
        s = rng.below(16)
        if s == 0:
            d[0] = (rng.choice([0, 5, 6, 15]) << 4) | (d[0] & 0xF)
        elif s == 1:
            d[0] = 0x40 | rng.below(5)
        elif s == 2:
            d[2:4] = struct.pack("!H", rng.choice([hl - 1, 0, 19, n + 1, n + 100]))
        elif s == 3:
            d[6:8] = struct.pack("!H", rng.choice([0x8000, 0x2000, 0x2000 | 3, 5, 0x4000 | 5, 0x6000, 0x1FFF]))
        elif s == 4 and kind in ("udp", "udp0"):
            d[hl + 4:hl + 6] = struct.pack("!H", rng.choice([n - hl + 1, n - hl - 1, 7, 0, 0xFFFF]))
        elif s == 5 and kind == "tcp":
            d[hl + 12] = rng.choice([0, 4, 15, 6]) << 4
        elif s == 6 and kind in ("tcp", "udp", "udp0"):
            p = hl + 2 * rng.below(2)
            d[p:p + 2] = b"\0\0"
        elif s == 7 and kind == "tcp":
            d[hl + 13] = rng.choice([0, 0x03, 0x06, 0x3F, 0x05])
        elif s == 8 and d[9] == P_ICMP:
            d[hl] = rng.choice([1, 2, 7, 19, 40, 255, 3, 4, 5, 11, 12, 13, 14, 17, 18])
        elif s == 9 and d[9] == P_ICMP:
            d[hl + 1] = rng.choice([1, 16, 255])
        elif s == 10 and d[9] == P_IGMP:
            d[hl] = rng.choice([0x12, 0x17, 0x22, 0x01, 0x11, 0x16, 0x13])
        elif s == 11 and d[9] == P_IGMP:
            d[hl + 4:hl + 8] = rng.choice([ALL_HOSTS, bytes([239, 9, 9, 9]), bytes(4), HOST])
        elif s == 12:
            d[9] = rng.choice([P_TCP, P_UDP, P_ICMP, P_IGMP, 41, 50, 132])
        elif s == 13:
            d[6:8] = struct.pack("!H", rng.choice([0x2000, 0x2000 | 8, 16]))
        finalize(d, udp_sum)
        if not good_l4 and n > hl + 4:
            d[n - 1] ^= 0x10
    else:                                                       # the received length
        finalize(d, udp_sum)
        received = rng.choice([n + 1, n + 6, n + rng.randint(1, 40), n - 1, n - 1, max(n - rng.randint(2, 30), 0), 19, 0])
    out = bytes(d)
    if received > n:
        out += rng.randbytes(received - n)
    return out[:received]


def gen_dgrams(seed: str, count: int):
    rng = ShakeRng(seed, reserve=count * 400)
    return [gen_dgram(rng) for _ in range(count)]


def dgrams_sha256(dgrams) -> str:
    h = hashlib.sha256()
    for d in dgrams:
        h.update(struct.pack("<H", len(d)))
        h.update(d)
    return h.hexdigest()


def all_dgrams(fx):
    """-> (names, datagrams, link-layer broadcast flags) of the whole fixture: the explicit cases, then the
    generated set (checked against its recorded SHA-256)."""
    names = [c["name"] for c in fx["cases"]]
    dg = [case_dgram(c) for c in fx["cases"]]
    g = fx["generated"]
    gen = gen_dgrams(g["seed"], g["count"])
    if dgrams_sha256(gen) != g["sha256"]:
        raise AssertionError("the generated datagram set does not have the recorded SHA-256")
    dg += gen
    return names + [f"generated[{i}]" for i in range(g["count"])], dg, [rx_bcast(d) for d in dg]


# ------------------------------------------------------------------------------------- recorded outcomes
def pack_calls(per_dgram) -> str:
    """[[(len, pseudo octets), ...] per datagram] -> base64 of zlib of, per datagram and call, u16 len, u8
    pseudo length, the pseudo octets (the number of calls is the outcome record's)."""
    raw = bytearray()
    for calls in per_dgram:
        for ln, pseudo in calls:
            raw += struct.pack("<HB", ln, len(pseudo)) + pseudo
    return base64.b64encode(zlib.compress(bytes(raw), 9)).decode()


def compact(rec):
    """An outcome record as a row of fx["outcomes"]: no per-datagram call fields, counters (each moved by 1,
    none outside the named ones) as a list of names, a call as "function protocol-type offset result"."""
    return {"err": rec["err"], "stubs": rec["stubs"], "discards": rec["discards"], "frag_queued": rec["frag_queued"],
            "ctr": list(rec["ctr"]), "calls": [f"{c['fn']} {c['proto']} {c['off']} {c['result']}" for c in rec["calls"]]}


def outcomes_of(fx, lib):
    """-> per datagram the outcome record as RefIPv4.rx() gives it: its fx["outcomes"] row expanded, the calls
    with their "len" and "pseudo" (hex)."""
    n = len(fx["cases"]) + fx["generated"]["count"]
    ix = refvec.unpack(fx["out"]["ipv4"]["outcome"], np.uint16, n)
    if lib != "ipv4":                                           # stored as its differences from "ipv4"
        for i, v in fx["out"][lib]["outcome"]:
            ix[i] = v
    raw = zlib.decompress(base64.b64decode(fx["out"][lib]["calls"] or fx["out"]["ipv4"]["calls"]))
    pos, out = 0, []
    for i in ix:
        r = dict(fx["outcomes"][int(i)])
        calls = []
        for c in r["calls"]:
            fn, proto, off, result = c.split()
            ln, pl = struct.unpack_from("<HB", raw, pos)
            calls.append({"fn": fn, "proto": proto, "off": int(off), "result": int(result), "len": ln,
                          "pseudo": raw[pos + 3:pos + 3 + pl].hex()})
            pos += 3 + pl
        r.update(calls=calls, ctr={k: 1 for k in r["ctr"]}, ctr_other=0)
        out.append(r)
    assert pos == len(raw)
    return out


# ------------------------------------------------------------------------------------- the live libraries
class RefIPv4:
    """One build of the reference's IPv4 receive family behind oracle/ref/glue_ipv4.c."""
    MAX_CALLS, MAX_CTRS = 8, 128

    def __init__(self, lib: str):
        import ctypes
        u32 = ctypes.c_uint32

        class Call(ctypes.Structure):
            _fields_ = [("fn", u32), ("proto", u32), ("len", u32), ("off", u32), ("result", u32), ("pseudo_len", u32),
                        ("pseudo", ctypes.c_uint8 * 40)]

        class Out(ctypes.Structure):
            _fields_ = [("err", ctypes.c_int32), ("stubs", u32), ("discards", u32), ("frag_queued", u32), ("ctr_other", u32),
                        ("n_calls", u32), ("ctr", u32 * self.MAX_CTRS), ("calls", Call * self.MAX_CALLS)]

        self.ct, self.Out = ctypes, Out
        L = ctypes.CDLL(os.path.join(REF_DIR, LIB_FILES[lib]))
        L.RefIPv4_Rx.argtypes = [ctypes.c_char_p, ctypes.c_uint16, u32, u32, u32, u32, ctypes.POINTER(Out)]
        L.RefIPv4_Rx.restype = ctypes.c_int
        L.RefIPv4_Cfg.restype = u32
        for f in (L.RefIPv4_ErrNames, L.RefIPv4_CtrNames, L.RefIPv4_StubNames, L.RefIPv4_ProtoNames):
            f.restype = ctypes.c_char_p
        self.L = L
        self.cfg = int(L.RefIPv4_Cfg())
        self.err_name = {int(v): k for k, v in (ln.split() for ln in L.RefIPv4_ErrNames().decode().splitlines())}
        self.proto_name = {int(v): k for k, v in (ln.split() for ln in L.RefIPv4_ProtoNames().decode().splitlines())}
        self.ctr_names = L.RefIPv4_CtrNames().decode().split()
        self.stub_names = L.RefIPv4_StubNames().decode().split()

    def rx(self, dgram: bytes, bcast=None):
        """-> the outcome record, calls with "len" and "pseudo". Names, not numbers. Transmit-side counters
        (field names starting with Tx) are not part of the record."""
        o = self.Out()
        buf = self.ct.create_string_buffer(bytes(dgram), max(len(dgram), 1))
        be = lambda b: int.from_bytes(b, "big")
        rc = self.L.RefIPv4_Rx(buf, len(dgram), rx_bcast(dgram) if bcast is None else bcast, be(HOST), be(MASK), be(GROUP),
                               self.ct.byref(o))
        assert rc == 0, f"RefIPv4_Rx: start state step {rc} failed"
        assert o.n_calls <= self.MAX_CALLS
        calls = [{"fn": FN_NAMES[c.fn], "proto": self.proto_name[c.proto], "off": c.off, "result": c.result, "len": c.len,
                  "pseudo": bytes(c.pseudo[:c.pseudo_len]).hex()} for c in o.calls[:o.n_calls]]
        ctr = {k: int(v) for k, v in zip(self.ctr_names, o.ctr) if v and not k.split(".")[1].startswith("Tx")}
        return {"err": self.err_name[o.err], "stubs": [s for k, s in enumerate(self.stub_names) if o.stubs >> k & 1],
                "discards": o.discards, "frag_queued": o.frag_queued, "ctr": ctr, "ctr_other": o.ctr_other, "calls": calls}
