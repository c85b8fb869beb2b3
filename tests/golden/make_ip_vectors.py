#!/usr/bin/env python3
"""Record tests/golden/reference_ip_vectors.json from the reference's own IPv4 receive family.

`make -C oracle` builds the untouched IP/IPv4/net_ipv4.c, net_icmpv4.c, net_igmp.c, Source/net_udp.c and
net_tcp.c of a reference tree over its untouched Source/net_util.c, behind the stubs and the recording
checksum wrappers of oracle/ref/glue_ipv4.c, into oracle/_ref/: libipv4_ref.so (the template
configuration with error counters on), its -O0 twin, and libipv4_ref_udpdis.so (with
NET_UDP_CFG_RX_CHK_SUM_DISCARD_EN). This script hands NetIPv4_Rx one datagram at a time, always from the
same start state, and writes down what came back: the error returned, the stubs that ran, the receive
error counters that moved, and every call made to the four checksum functions (function, protocol type,
offset, length, pseudo-header octets, result). No rule of this project computes anything here: the only
expectations are the named rows below whose outcome can be stated without any code, which are asserted,
and the three shares the recorded reference alone must keep (printed; see check_shares). Every case must
give the same record at -O0 and -O2.

    python tests/golden/make_ip_vectors.py           # rewrites the fixture
    python tests/golden/make_ip_vectors.py --check   # regenerates in memory, compares with the file

The datagrams are described in tests/ipvec.py.
"""
import collections
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for sub in ("tests",):
    sys.path.insert(0, os.path.join(REPO, sub))

import ipvec as iv      # noqa: E402
import refvec           # noqa: E402

MAX_BYTES = 200000      # the fixture stays in the range of the other reference fixtures
GEN_SEED, GEN_COUNT = "ip/generated/0", 3000
CFG_WANT = {"ipv4": 0x1D, "ipv4_O0": 0x1D, "udpdis": 0x5D}   # IPv4, IGMP, TCP, error counters; + UDP discard
PAYLOADS = (0, 1, 2, 3, 8, 31, 64)
FULL_KINDS = ("tcp", "udp", "echo_req", "igmp_query")   # the kinds that get every sweep; the others a sample
BIG = (576, 1480, 8980)                      # payload octets of the three long datagrams per protocol
CHK_SUM_CTRS = ("IPv4.RxInvChkSumCtr", "TCP.RxHdrChkSumCtr", "UDP.RxHdrChkSumCtr", "ICMPv4.RxInvChkSumCtr", "IGMP.RxHdrChkSumCtr")
UPPER = ("NetSock_Rx", "NetConn_Srch", "NetICMP_RxEchoReply", "NetBuf_GetMaxSize")


def ones_add(a, b):
    s = a + b
    return (s & 0xFFFF) + (s >> 16)


def explicit_cases():
    cases, seen = [], set()

    def add(name, d: bytes):
        assert name not in seen, name
        seen.add(name)
        c = {"name": name, "n": len(d), "head": d[:iv.HEAD].hex()}
        assert iv.case_dgram(c) == d, name
        cases.append(c)

    def mk(name, kind, plen, *, pre=None, flip=None, fix_ip=False, post=None, received=None, zero_sum=False, **kw):
        """kind's datagram with plen payload octets. pre(d): before the checksums are stored. flip = (offset,
        mask): that bit is flipped after the checksums are stored, or, in the derived tail, the checksums
        stored are those of the datagram with that bit the other way (negative offsets count from the end); fix_ip: ... and the IP header checksum is made right again. zero_sum: a payload word is
        chosen so that the transport checksum computes to 0x0000. post(d): after everything. received: octets
        handed to the reference (more: padding; fewer: cut)."""
        udp_sum = kind != "udp0"
        d = iv.build(kind, refvec.shake("ip/payload/" + name, plen), **kw)
        n = len(d)
        rcv = n if received is None else received
        full = d + refvec.shake("ip/pad/" + name, max(rcv - n, 0))
        if rcv > iv.HEAD:                                       # octets from HEAD on are the derived tail
            full[iv.HEAD:rcv] = iv.tail_bytes(name, rcv)
        d, pad = full[:n], bytes(full[n:])
        if pre:
            pre(d)
        hl = (d[0] & 0xF) * 4
        if flip:
            pos = flip[0] if flip[0] >= 0 else n + flip[0]
            if pos >= iv.HEAD:                                  # the tail is fixed: make the checksums wrong instead
                d[pos] ^= flip[1]
                iv.finalize(d, udp_sum)
                d[pos] ^= flip[1]
            else:
                iv.finalize(d, udp_sum)
                d[pos] ^= flip[1]
            if fix_ip:
                d[10:12] = b"\0\0"
                d[10:12] = struct.pack("!H", iv.csum16(bytes(d[:hl])))
        else:
            iv.finalize(d, udp_sum)
        if zero_sum:
            fld = hl + {iv.P_TCP: 16, iv.P_UDP: 6}[d[9]]
            c = struct.unpack("!H", d[fld:fld + 2])[0]
            w = n - 2 - ((n - hl) & 1)                          # an aligned payload word inside the head
            assert hl + (8 if d[9] == iv.P_UDP else 20) <= w < iv.HEAD
            d[w:w + 2] = struct.pack("!H", ones_add(struct.unpack("!H", d[w:w + 2])[0], c))
            iv.finalize(d, udp_sum)
            assert d[fld:fld + 2] == (b"\xff\xff" if d[9] == iv.P_UDP else b"\0\0"), name
        if post:
            post(d)
        out = bytes(d) + pad
        add(name, out[:rcv])

    def setb(pos, b):
        def f(d):
            d[pos:pos + len(b)] = b
        return f

    def l4(pos, b):                                             # ... at an offset into the transport part
        def f(d):
            p = (d[0] & 0xF) * 4 + pos
            d[p:p + len(b)] = b
        return f

    for kind in iv.KINDS:
        # every protocol: good, and one bit flipped in turn in the transport header, the last octet, the
        # pseudo-header inputs (addresses, protocol, length) and the IP header
        for plen in PAYLOADS:
            mk(f"{kind} payload {plen}: good", kind, plen)
            mk(f"{kind} payload {plen}: last octet bit", kind, plen, flip=(-1, 0x01))
        for plen in BIG:
            mk(f"{kind} payload {plen}: good", kind, plen)
            mk(f"{kind} payload {plen}: last octet bit", kind, plen, flip=(-1, 0x80))
        for pos, what in ((20, "transport octet 0"), (21, "transport octet 1"), (8, "ttl")):
            mk(f"{kind}: {what} bit", kind, 12, flip=(pos, 0x04))
        for pos, what in ((12, "source address"), (19, "destination address"), (9, "protocol"), (3, "total length")):
            mk(f"{kind}: {what} bit, header checksum right", kind, 12, flip=(pos, 0x04), fix_ip=True)
        mk(f"{kind}: header checksum field bit", kind, 12, post=setb(10, b"\x00"))
        # IHL 5..15: NOP / EOL padding, a record-route or timestamp option, random option octets
        for ihl in range(5, 16) if kind in FULL_KINDS else (6, 15):
            mk(f"{kind} ihl {ihl}: padding, good", kind, 5, ihl=ihl)
            mk(f"{kind} ihl {ihl}: padding, last octet bit", kind, 5, ihl=ihl, flip=(-1, 0x02))
        for ihl in (6, 8, 11, 15) if kind in ("tcp", "udp") else ():
            for nm, opt in (("record route", iv.opt_record_route(ihl)), ("timestamp", iv.opt_timestamp(max(ihl, 7))[:4 * (ihl - 5)]),
                            ("random options", refvec.shake(f"ip/opts/{kind}/{ihl}", 4 * (ihl - 5)))):
                mk(f"{kind} ihl {ihl}: {nm}, good", kind, 6, ihl=ihl, opts=opt)
                mk(f"{kind} ihl {ihl}: {nm}, last octet bit", kind, 6, ihl=ihl, opts=opt, flip=(-1, 0x02))
        # received length against total length
        for good in (True, False) if kind in FULL_KINDS[:3] else ():
            g = "good" if good else "bad sum"
            fl = None if good else (-1, 0x08)
            for extra in (1, 6, 26):
                mk(f"{kind}: received total + {extra}, {g}", kind, 9, flip=fl, received=20 + len(iv.transport(kind, bytes(9))[1]) + extra)
            mk(f"{kind}: received total - 1, {g}", kind, 9, flip=fl, received=20 + len(iv.transport(kind, bytes(9))[1]) - 1)
            # the structural faults of the IP header, each with a right and a wrong transport checksum
            mk(f"{kind}: total length < header length, {g}", kind, 9, flip=fl, pre=setb(2, b"\x00\x13"))
            for v in (0, 5, 6, 15):
                mk(f"{kind}: version {v}, {g}", kind, 9, flip=fl, post=setb(0, bytes([(v << 4) | 5])))
            for i in (0, 4):
                mk(f"{kind}: ihl {i}, {g}", kind, 9, flip=fl, post=setb(0, bytes([0x40 | i])))
            for nm, ff, pl in (("first fragment", 0x2000, 16), ("middle fragment", 0x2000 | 2, 16), ("last fragment", 2, 9),
                               ("fragment, length no multiple of 8", 0x2000, 9), ("DF with an offset", 0x4000 | 3, 9),
                               ("DF with MF", 0x6000, 16), ("reserved flag", 0x8000, 9), ("DF alone", 0x4000, 9)):
                mk(f"{kind}: {nm}, {g}", kind, pl, flip=fl, flags_frag=ff)
            for nm, a in (("foreign destination", iv.FOREIGN), ("destination in another subnet", bytes([10, 1, 3, 3])),
                          ("destination this host 0.0.0.0", bytes(4)), ("unjoined group", bytes([239, 9, 9, 9])),
                          ("limited broadcast", iv.BCAST), ("subnet broadcast", iv.SUBNET_BCAST), ("joined group", iv.GROUP)):
                mk(f"{kind}: {nm}, {g}", kind, 9, flip=fl, dst=a)
            for nm, a in (("this host", bytes(4)), ("loopback", bytes([127, 0, 0, 1])), ("broadcast", iv.BCAST), ("multicast", iv.GROUP),
                          ("a far unicast", iv.SRC_FAR), ("class E", bytes([240, 0, 0, 1]))):
                mk(f"{kind}: source {nm}, {g}", kind, 9, flip=fl, src=a)
    for good in (True, False):
        g = "good" if good else "bad sum"
        fl = None if good else (-1, 0x08)
        # UDP length against the IP payload length
        for kind in ("udp", "udp0"):
            for nm, f in (("+ 1", lambda n: n + 1), ("- 1", lambda n: n - 1), ("7", lambda n: 7), ("0", lambda n: 0), ("8 of more", lambda n: 8)):
                mk(f"{kind}: length field {nm}, {g}", kind, 10, flip=fl, pre=l4(4, struct.pack("!H", f(18))))
            mk(f"{kind}: source port 0, {g}", kind, 10, flip=fl, pre=l4(0, b"\0\0"))
            mk(f"{kind}: destination port 0, {g}", kind, 10, flip=fl, pre=l4(2, b"\0\0"))
        for plen in range(0, 8):                                # UDP datagrams of fewer than 8 octets
            mk(f"udp of {plen} octets, {g}", "other", plen, flip=fl, pre=setb(9, bytes([iv.P_UDP])))
        # TCP shapes
        for off in (0, 4, 6, 8, 15):
            mk(f"tcp: data offset {off}, {g}", "tcp", 6, flip=fl, pre=l4(12, bytes([off << 4])))
        for plen in (0, 1, 4, 16, 19):
            mk(f"tcp segment of {plen} octets, {g}", "other", plen, flip=fl, pre=setb(9, bytes([iv.P_TCP])))
        mk(f"tcp: source port 0, {g}", "tcp", 6, flip=fl, pre=l4(0, b"\0\0"))
        mk(f"tcp: destination port 0, {g}", "tcp", 6, flip=fl, pre=l4(2, b"\0\0"))
        for fb in (0x00, 0x03, 0x06, 0x05, 0x3F, 0xC0 | 0x10):
            mk(f"tcp: flags {fb:#04x}, {g}", "tcp", 6, flip=fl, pre=l4(13, bytes([fb])))
        mk(f"tcp: options 8 octets of NOP, {g}", "tcp", 8, flip=fl, pre=lambda d: (l4(12, b"\x70")(d), l4(20, b"\x01" * 8)(d)))
        # ICMPv4 shapes
        for plen in range(0, 8):
            mk(f"icmp of {plen} octets, {g}", "other", plen, flip=fl, pre=setb(9, bytes([iv.P_ICMP])))
        for typ in (1, 2, 3, 4, 5, 11, 12, 13, 14, 17, 18, 19, 255):
            mk(f"icmp echo request retyped {typ}, {g}", "echo_req", 8, flip=fl, pre=l4(0, bytes([typ])))
        for code in (1, 16):
            mk(f"icmp echo request code {code}, {g}", "echo_req", 8, flip=fl, pre=l4(1, bytes([code])))
            mk(f"icmp dest unreachable code {code}, {g}", "icmp_err", 0, flip=fl, pre=l4(1, bytes([code])))
        for kind in ("echo_req", "echo_reply"):
            for a, nm in ((iv.BCAST, "limited broadcast"), (iv.GROUP, "joined group")):
                mk(f"{kind} to the {nm}, again, {g}", kind, 3, flip=fl, dst=a)
        # IGMP shapes
        for plen in range(0, 8):
            mk(f"igmp of {plen} octets, {g}", "other", plen, flip=fl, pre=setb(9, bytes([iv.P_IGMP])))
        for vt in (0x01, 0x13, 0x16, 0x17, 0x21, 0x22):
            mk(f"igmp type octet {vt:#04x}, {g}", "igmp_report", 0, flip=fl, pre=l4(0, bytes([vt])))
        mk(f"igmp report to all hosts, {g}", "igmp_report", 0, flip=fl, dst=iv.ALL_HOSTS)
        mk(f"igmp report of another group, {g}", "igmp_report", 0, flip=fl, pre=l4(4, bytes([239, 9, 9, 9])))
        mk(f"igmp query to this host, {g}", "igmp_query", 0, flip=fl, dst=iv.HOST)
        mk(f"igmp query to the joined group, {g}", "igmp_query", 0, flip=fl, dst=iv.GROUP)
    # a sum that comes out 0x0000 against 0xFFFF
    for plen in (4, 7):
        mk(f"udp payload {plen}: checksum computes to 0, sent as 0xffff", "udp", plen, zero_sum=True)
        mk(f"udp payload {plen}: checksum computes to 0, field 0x0000", "udp", plen, zero_sum=True, post=l4(6, b"\0\0"))
        mk(f"tcp payload {plen}: checksum computes to 0, field 0x0000", "tcp", plen, zero_sum=True)
        mk(f"tcp payload {plen}: checksum computes to 0, field 0xffff", "tcp", plen, zero_sum=True, post=l4(16, b"\xff\xff"))
    mk("udp payload 4: field 0xffff over a sum that is not 0", "udp", 4, post=l4(6, b"\xff\xff"))
    mk("empty", "other", 0, received=0)
    mk("one octet", "other", 0, received=1)
    mk("19 octets", "udp", 4, received=19)
    mk("header only, protocol udp", "other", 0, pre=setb(9, bytes([iv.P_UDP])))
    return cases


# rows whose outcome can be stated without any code: name -> (stub that ran or counter that moved)
NAMED = {
    "udp payload 8: good": "NetSock_Rx", "udp0 payload 8: good": "NetSock_Rx", "tcp payload 8: good": "NetConn_Srch",
    "echo_reply payload 8: good": "NetICMP_RxEchoReply", "echo_req payload 8: good": "NetBuf_GetMaxSize",
    "udp payload 8: last octet bit": "UDP.RxHdrChkSumCtr", "tcp payload 8: last octet bit": "TCP.RxHdrChkSumCtr",
    "echo_req payload 8: last octet bit": "ICMPv4.RxInvChkSumCtr", "igmp_query payload 0: last octet bit": "IGMP.RxHdrChkSumCtr",
    "udp: ttl bit": "IPv4.RxInvChkSumCtr", "tcp: source address bit, header checksum right": "TCP.RxHdrChkSumCtr",
    "udp: source address bit, header checksum right": "UDP.RxHdrChkSumCtr", "udp: version 6, good": "IPv4.RxInvVerCtr", "udp: ihl 4, good": "IPv4.RxInvLenCtr",
    "udp: total length < header length, good": "IPv4.RxInvTotLenCtr", "udp: received total - 1, good": "IPv4.RxInvTotLenCtr",
    "udp: received total + 6, good": "NetSock_Rx", "udp: reserved flag, good": "IPv4.RxInvFlagsCtr",
    "udp: foreign destination, good": "IPv4.RxDestCtr", "udp: source loopback, good": "IPv4.RxInvAddrSrcCtr",
    "udp: limited broadcast, good": "NetSock_Rx", "udp: joined group, good": "NetSock_Rx", "udp ihl 15: padding, good": "NetSock_Rx",
    "tcp ihl 8: record route, good": "NetConn_Srch", "udp: length field + 1, good": "UDP.RxHdrDatagramLenCtr",
    "udp payload 4: checksum computes to 0, sent as 0xffff": "NetSock_Rx", "tcp payload 4: checksum computes to 0, field 0xffff": "NetConn_Srch",
    "tcp payload 4: checksum computes to 0, field 0x0000": "NetConn_Srch", "other payload 8: good": "IPv4.RxInvProtocolCtr",
}
NAMED_UDPDIS = {"udp0 payload 8: good": "UDP.RxHdrChkSumCtr", "udp payload 8: good": "NetSock_Rx"}


def what_of(rec):
    """The upper stub that ran, else the receive counters that moved besides the discard counters: a reading
    of the record for the named rows (the tests have their own table)."""
    up = [s for s in rec["stubs"] if s in UPPER]
    if up:
        return up
    return [k for k in rec["ctr"] if not k.endswith(("RxPktDisCtr", "RxPktDiscardedCtr"))]


def check_named(lib, names, recs):
    by_name = dict(zip(names, recs))
    for name, what in {**NAMED, **(NAMED_UDPDIS if lib == "udpdis" else {})}.items():
        assert what in what_of(by_name[name]), (lib, name, by_name[name])


def check_shares(lib, recs):
    """What the recorded reference alone must keep, so that the tests' caps can hold: every checksum counter
    moved for at least 20 datagrams (UDP's for 20 datagrams without a checksum under the discard build), and
    at most a third of the datagrams made no checksum call."""
    count = collections.Counter(k for r in recs for k in r["ctr"] if k in CHK_SUM_CTRS)
    assert all(count[k] >= 20 for k in CHK_SUM_CTRS), (lib, count)
    no_call = sum(not r["calls"] for r in recs)
    assert 3 * no_call <= len(recs), (lib, no_call, len(recs))
    assert all(r["ctr_other"] == 0 and len(r["calls"]) <= 3 for r in recs)
    return {"no_checksum_call": no_call, "datagrams": len(recs), **{k: count[k] for k in CHK_SUM_CTRS}}


def generate():
    libs = {k: iv.RefIPv4(k) for k in iv.LIB_FILES}
    for k, L in libs.items():
        assert L.cfg == CFG_WANT[k], (k, hex(L.cfg))
        assert L.ctr_names == libs["ipv4"].ctr_names and L.stub_names == libs["ipv4"].stub_names
    cases = explicit_cases()
    names = [c["name"] for c in cases]
    dgrams = [iv.case_dgram(c) for c in cases]
    gen = iv.gen_dgrams(GEN_SEED, GEN_COUNT)
    names += [f"generated[{i}]" for i in range(GEN_COUNT)]
    dgrams += gen

    table, out, calls_made, shares = [], {}, 0, {}
    key_of = {}
    for lib in iv.LIBS:
        ix, per_calls, recs = [], [], []
        for nm, d in zip(names, dgrams):
            rec = libs[lib].rx(d)
            calls_made += 1
            if lib == "ipv4":
                calls_made += 1
                twin = libs["ipv4_O0"].rx(d)
                if twin != rec:
                    raise AssertionError(f"{nm}: -O2 gives {rec}, -O0 gives {twin}")
            recs.append(rec)
            per_calls.append([(c["len"], bytes.fromhex(c["pseudo"])) for c in rec["calls"]])
            assert rec["ctr_other"] == 0 and all(v == 1 for v in rec["ctr"].values()), (nm, rec)
            row = iv.compact(rec)
            key = json.dumps(row, sort_keys=True)
            if key not in key_of:
                key_of[key] = len(table)
                table.append(row)
            ix.append(key_of[key])
        check_named(lib, names, recs)
        shares[lib] = check_shares(lib, recs)
        out[lib] = {"cfg": libs[lib].cfg, "outcome": refvec.pack(np.array(ix, np.uint16)), "calls": iv.pack_calls(per_calls)}
        if lib != "ipv4":                                       # ... stored as its differences from "ipv4"
            base = refvec.unpack(out["ipv4"]["outcome"], np.uint16, len(ix))
            out[lib]["outcome"] = [[i, v] for i, (v, b) in enumerate(zip(ix, base)) if v != b]
            if out[lib]["calls"] == out["ipv4"]["calls"]:
                out[lib]["calls"] = None
    assert len(table) < 65536
    doc = {
        "generator": "tests/golden/make_ip_vectors.py",
        "source": "what NetIPv4_Rx of the reference's IP/IPv4/net_ipv4.c (V3.06.01), with net_icmpv4.c, net_igmp.c, net_udp.c and "
                  "net_tcp.c over net_util.c, did with each datagram behind the stubs and recording checksum wrappers of "
                  "oracle/ref/glue_ipv4.c, built by oracle/Makefile `ref`: LP64 little-endian; libraries ipv4 (template "
                  "configuration, error counters on) and udpdis (NET_UDP_CFG_RX_CHK_SUM_DISCARD_EN on); -O0 and -O2 builds of ipv4 "
                  "agree on every case. Every datagram met the same start state: interface 1 up with `host` / `mask` configured "
                  "and `group` joined, no fragment lists, no connections, no transmit buffers",
        "host": iv.HOST.hex(), "mask": iv.MASK.hex(), "group": iv.GROUP.hex(),
        "ctr_names": libs["ipv4"].ctr_names, "stubs": libs["ipv4"].stub_names, "cases": cases,
        "generated": {"seed": GEN_SEED, "count": GEN_COUNT, "sha256": iv.dgrams_sha256(gen)},
        "outcomes": table, "out": out, "shares": shares, "reference_calls": calls_made,
    }
    return json.dumps(doc, separators=(",", ":")) + "\n"


def main():
    if not iv.libs_available():
        sys.exit("oracle/_ref/libipv4_ref*.so are missing: `make -C oracle` with a reference tree builds them")
    check = "--check" in sys.argv[1:]
    text = generate()
    assert len(text.encode()) <= MAX_BYTES, len(text.encode())
    if check:
        with open(iv.FIXTURE) as f:
            have = f.read()
        if have != text:
            sys.exit("tests/golden/reference_ip_vectors.json differs from what the reference libraries give now")
        print(f"check ok: {len(text.encode())} bytes reproduce")
        return
    with open(iv.FIXTURE, "w") as f:
        f.write(text)
    doc = json.loads(text)
    print(f"wrote {iv.FIXTURE}: {len(text.encode())} bytes, {len(doc['cases'])} explicit cases, {GEN_COUNT} generated, "
          f"{len(doc['outcomes'])} distinct outcomes, {doc['reference_calls']} reference calls")
    for lib, c in doc["shares"].items():
        print(" ", lib, c)


if __name__ == "__main__":
    main()
