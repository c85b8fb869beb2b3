"""The Rx burst's IPv4 and transport verdicts against the reference's own receive path (CPU; no kernel
launches).

tests/golden/reference_ip_vectors.json holds what the untouched NetIPv4_Rx, with the reference's ICMPv4,
IGMP, UDP and TCP receive functions above it and its net_util.c below, did with each datagram
(tests/golden/make_ip_vectors.py recorded it through oracle/ref/glue_ipv4.c; tests/ipvec.py reads it):
two builds — "ipv4", the template configuration, and "udpdis", with NET_UDP_CFG_RX_CHK_SUM_DISCARD_EN —
and per datagram the error returned, the stubs above the transport layer that were reached, the receive
error counters that moved, and every call made to the four checksum functions.

Held against it, per datagram, under rx_cfg 0 ("ipv4") and NETCSUM_RXCFG_UDP_DISCARD_NO_CHK_SUM ("udpdis"):
oracle_packets.rx_validate_ip (flags, and the checksum calls it makes), netcsum.rx_action
(NetUtil_MI355X_RxAction) of those flags, and the verdict of netcsum_ipparse.h through
tests/c_ipparse/ipparse_caller.cpp at window limits 81, 1024 and the datagram's own length, which must
equal the oracle's flags. The rules are the tables below, read off the reference's counter names and the
header's DROP list (include/netcsum_mi355x.h names the counter of each DROP code), not off our rules:

1. the reference moved a checksum counter -> the action is that counter's DROP code, and the flags say so
   (IP_OK clear; L4_CHECKED set and L4_OK clear; UDP_NO_CSUM for the discard build's datagram without one);
2. the reference reached a stub above the transport layer, or took the datagram without an error ->
   DELIVER; a fragment it queued -> DELIVER_L4_UNVERIFIED;
3. an action of DROP -> the reference reached no such stub, and counted either that DROP's counter or one
   of a check that precedes that checksum in its own order (PRECEDING: the exception include/
   netcsum_mi355x.h documents: both sides drop, the counter differs);
4. every checksum call the reference made, the oracle made too, at the same place in the same order:
   function, protocol type, offset, length, pseudo-header octets, result;
5. a datagram the reference rejected for version, header length or total length is MALFORMED here, or is
   one whose version nibble is 6, which this project judges as an IPv6 datagram (mixed bursts); a UDP
   datagram it rejected for its length field is L4_MALFORMED here, and left to the stack.

Caps, so that the exception cannot hide a failure: every DROP code 1-6 is witnessed by >= 20 datagrams
under rule 1 (code 4 under the discard build), the DROP rows resting on the exception are <= 1/4 of all
DROP rows, and the datagrams that give rule 4 nothing to compare are <= 1/3 of the corpus. The shares of
the committed fixture (printed by test_shares): exception rows 274 of 1 428 DROP rows (19.2 %) under
rx_cfg 0 and 328 of 1 828 (17.9 %) under the discard build; datagrams without a reference checksum call
392 of 3 789 (10.3 %); fewest rule-1 witnesses of a DROP code: 165 (TCP).

Where oracle/_ref/ holds the libraries the recorder's --check runs too; it skips, saying so, where it
does not. Everything else reads the fixture only.
"""
import os
import re
import sys

import pytest

import ipvec as iv
import netcsum
import oracle_packets as op
from test_ipparse_cpu import exe, run  # noqa: F401  (the stand-alone caller, built with the sanitizers)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN_DIR)
import make_ip_vectors as rec  # noqa: E402  (the recorder: no rule of this project in it)

needs_ref = pytest.mark.skipif(not iv.libs_available(),
                               reason="oracle/_ref/libipv4_ref*.so are absent (no reference tree at build time)")
RX_CFG = {"ipv4": 0, "udpdis": netcsum.RXCFG_UDP_DISCARD_NO_CHK_SUM}
LIMITS = (81, 1024, None)                   # the smallest and largest kernel windows, and the datagram's own length
DELIVER, UNVERIFIED = netcsum.RX_DELIVER, netcsum.RX_DELIVER_L4_UNVERIFIED


def _header_drops():
    """{counter name: [DROP codes]} from the header's text: '#define NETCSUM_RX_DROP_x  nu  /* Counter ...'."""
    text = open(os.path.join(netcsum.REPO, "include", "netcsum_mi355x.h")).read()
    out = {}
    for m in re.finditer(r"#define NETCSUM_RX_DROP_\w+\s+(\d+)u\s+/\*\s*([\w.]+)", text):
        out.setdefault(m.group(2), []).append(int(m.group(1)))
    return out


DROPS = _header_drops()
CHK_SUM_CTR = {"IPv4.RxInvChkSumCtr": 1, "TCP.RxHdrChkSumCtr": 2, "UDP.RxHdrChkSumCtr": 3, "ICMPv4.RxInvChkSumCtr": 5,
               "IGMP.RxHdrChkSumCtr": 6}
UDP_NO_CHK_SUM = 4                          # UDP.RxHdrChkSumCtr moved without a checksum call: the discard build
# the checks NetIPv4_RxPktValidate makes after the header checksum and before it hands the datagram up, as far as
# a transport DROP can meet them (its fragment-field and protocol checks cannot: a datagram with fragment
# fields is L4_UNVERIFIED here, one of another protocol carries no transport verdict)
IP_AFTER_CHK_SUM = {"IPv4.RxInvFlagsCtr", "IPv4.RxDestCtr", "IPv4.RxDestBcastCtr", "IPv4.RxInvAddrSrcCtr", "IPv4.RxInvOptsCtr"}
# per DROP code, the counters of the checks that come before that checksum in the reference's own order
# (NetTCP_RxPktValidate, NetUDP_RxPktValidate, NetICMPv4_RxPktValidate, NetIGMP_RxPktValidate)
PRECEDING = {
    1: set(),
    2: IP_AFTER_CHK_SUM | {"TCP.RxHdrPortSrcCtr", "TCP.RxHdrPortDestCtr", "TCP.RxHdrLenCtr", "TCP.RxHdrSegLenCtr", "TCP.RxHdrFlagsCtr"},
    3: IP_AFTER_CHK_SUM | {"UDP.RxHdrPortSrcCtr", "UDP.RxHdrPortDestCtr", "UDP.RxHdrDatagramLenCtr"},
    5: IP_AFTER_CHK_SUM | {"ICMPv4.RxBcastCtr", "ICMPv4.RxMcastCtr", "ICMPv4.RxInvTypeCtr", "ICMPv4.RxInvCodeCtr",
                           "ICMPv4.RxInvMsgLenCtr", "ICMPv4.RxInvPtrCtr"},
    6: IP_AFTER_CHK_SUM | {"IGMP.RxHdrMsgLenCtr", "IGMP.RxHdrVerCtr", "IGMP.RxPktInvalidAddrDestCtr", "IGMP.RxHdrTypeCtr"},
}
PRECEDING[4] = PRECEDING[3]
STRUCTURAL = {"IPv4.RxInvVerCtr", "IPv4.RxInvLenCtr", "IPv4.RxInvTotLenCtr"}
# stubs above the transport layer: the socket layer (UDP), the TCP connection search, the echo reply's taker,
# and the echo request's reply asking for its buffer size (NetICMPv4_TxReqReply; no other path here gets
# that far: TCP's callers of it sit behind a connection, and there are none)
UPPER = {"NetSock_Rx", "NetConn_Srch", "NetICMP_RxEchoReply", "NetBuf_GetMaxSize"}
PROTO_TYPE = {"NET_PROTOCOL_TYPE_NONE": 0, "NET_PROTOCOL_TYPE_ICMP_V4": netcsum.NET_PROTOCOL_TYPE_ICMP_V4,
              "NET_PROTOCOL_TYPE_IGMP": netcsum.NET_PROTOCOL_TYPE_IGMP, "NET_PROTOCOL_TYPE_UDP_V4": netcsum.NET_PROTOCOL_TYPE_UDP_V4,
              "NET_PROTOCOL_TYPE_TCP_V4": netcsum.NET_PROTOCOL_TYPE_TCP_V4}


def test_the_tables_are_the_headers():
    assert {k: DROPS[k] for k in CHK_SUM_CTR} == {"IPv4.RxInvChkSumCtr": [1], "TCP.RxHdrChkSumCtr": [2], "UDP.RxHdrChkSumCtr": [3, 4],
                                                   "ICMPv4.RxInvChkSumCtr": [5], "IGMP.RxHdrChkSumCtr": [6]}
    assert (DELIVER, UNVERIFIED) == (0, 8) and netcsum.RX_DROP_UDP_NO_CHK_SUM == UDP_NO_CHK_SUM


# ------------------------------------------------------------------ reading one record
def taken(r) -> bool:
    """The reference reached a stub above the transport layer, or took the datagram without an error (an
    IGMP message, which ends in no stub) and did not merely queue it as a fragment."""
    return bool(UPPER & set(r["stubs"])) or (r["err"] == "NET_IPv4_ERR_NONE" and not r["frag_queued"])


def queued(r) -> bool:
    return bool(r["frag_queued"]) and r["err"] == "NET_IPv4_ERR_NONE"


def recorded_drop(r):
    """The DROP code of the checksum counter the reference moved, or None."""
    moved = [k for k in r["ctr"] if k in CHK_SUM_CTR]
    assert len(moved) <= 1, r
    if not moved:
        return None
    code = CHK_SUM_CTR[moved[0]]
    if code == 3 and not any(c["fn"] == "data_verify" for c in r["calls"]):
        code = UDP_NO_CHK_SUM
    return code


def check_rules(name, d, r, flags, action, oracle_calls):
    """Rules 1-5 for one datagram under one configuration -> 'exception' | 'drop' | None, or raises.
    oracle_calls None: without rule 4 (the device reports no calls)."""
    ctx = (name, d[:40].hex(), len(d), f"flags {flags:#x} action {action}", r)
    want = recorded_drop(r)
    if want is not None:                                        # rule 1
        assert action == want, ("rule 1: the reference dropped it at a checksum check", ) + ctx
        if want == 1:
            assert not flags & op.IP_OK, ("rule 1: flags", ) + ctx
        elif want == UDP_NO_CHK_SUM:
            assert flags & op.UDP_NO_CSUM, ("rule 1: flags", ) + ctx
        else:
            assert flags & op.L4_CHECKED and not flags & op.L4_OK, ("rule 1: flags", ) + ctx
    if taken(r):                                                # rule 2
        assert action == (UNVERIFIED if r["frag_queued"] else DELIVER), ("rule 2: the reference took it", ) + ctx
    elif queued(r):
        assert action == UNVERIFIED, ("rule 2: the reference queued it as a fragment", ) + ctx
    for i, c in enumerate(r["calls"] if oracle_calls is not None else ()):   # rule 4
        assert c["fn"] in ("hdr_verify", "data_verify"), ("a transmit-side checksum call in the record", ) + ctx
        ref_call = (c["fn"], PROTO_TYPE[c["proto"]], c["off"], c["len"], bytes.fromhex(c["pseudo"]), c["result"])
        assert i < len(oracle_calls) and oracle_calls[i] == ref_call, \
            ("rule 4: checksum call", i, "reference", ref_call, "oracle", oracle_calls[i] if i < len(oracle_calls) else None) + ctx
    if STRUCTURAL & set(r["ctr"]):                              # rule 5
        assert flags & op.MALFORMED or (len(d) and d[0] >> 4 == 6), ("rule 5", ) + ctx
    if "UDP.RxHdrDatagramLenCtr" in r["ctr"]:
        assert flags & op.L4_MALFORMED and action == DELIVER, ("rule 5: a UDP length the reference rejected", ) + ctx
    if action in (DELIVER, UNVERIFIED):
        return None
    assert 1 <= action <= 6 or (d[0] >> 4 == 6 and action == netcsum.RX_DROP_ICMPV6_CHK_SUM), ("an unknown action", ) + ctx
    assert not taken(r), ("rule 3: dropped what the reference delivers", ) + ctx      # rule 3
    if want == action:
        return "drop"
    if d[0] >> 4 == 6:                                          # judged as IPv6; the reference counted the version
        assert "IPv4.RxInvVerCtr" in r["ctr"], ("rule 3", ) + ctx
        return "exception"
    assert want is None and PRECEDING[action] & set(r["ctr"]), \
        ("rule 3: a DROP the reference neither counted nor preceded by an earlier check", ) + ctx
    return "exception"


# ------------------------------------------------------------------ the fixture and our side of it
@pytest.fixture(scope="module")
def fx():
    return iv.load()


@pytest.fixture(scope="module")
def dgrams(fx):
    return iv.all_dgrams(fx)                                    # (names, datagrams, broadcast flags); checks the SHA-256


@pytest.fixture(scope="module")
def ours(dgrams):
    """Per datagram (flags, protocol, the oracle's checksum calls)."""
    out = []
    for d in dgrams[1]:
        calls = []
        flags = op.rx_validate(d, calls) if not (len(d) and d[0] >> 4 == 6) else op.rx_validate_ip(d)
        out.append((flags, d[9] if len(d) > 9 else 0, calls))
    return out


def test_fixture_is_small_and_covers_what_it_should(fx, dgrams):
    assert os.path.getsize(iv.FIXTURE) <= rec.MAX_BYTES
    names = set(dgrams[0])
    assert len(names) == len(dgrams[0]) and fx["generated"]["count"] >= 2000
    assert (bytes.fromhex(fx["host"]), bytes.fromhex(fx["mask"]), bytes.fromhex(fx["group"])) == (iv.HOST, iv.MASK, iv.GROUP)
    assert {k: fx["out"][k]["cfg"] for k in iv.LIBS} == {k: rec.CFG_WANT[k] for k in iv.LIBS}
    for kind in iv.KINDS:
        for plen in rec.PAYLOADS + rec.BIG:
            assert {f"{kind} payload {plen}: good", f"{kind} payload {plen}: last octet bit"} <= names
        for what in ("transport octet 0 bit", "source address bit, header checksum right", "protocol bit, header checksum right",
                     "total length bit, header checksum right", "header checksum field bit"):
            assert f"{kind}: {what}" in names
    for kind in rec.FULL_KINDS:
        for ihl in range(5, 16):
            assert {f"{kind} ihl {ihl}: padding, good", f"{kind} ihl {ihl}: padding, last octet bit"} <= names
    for g in ("good", "bad sum"):
        for what in ("received total + 6", "received total - 1", "total length < header length", "version 0", "version 5", "version 6",
                     "version 15", "ihl 4", "first fragment", "middle fragment", "last fragment", "fragment, length no multiple of 8",
                     "DF with an offset", "reserved flag", "foreign destination", "source this host", "source loopback",
                     "source broadcast", "source multicast"):
            assert f"udp: {what}, {g}" in names and f"tcp: {what}, {g}" in names
        for what in ("udp: length field + 1", "udp: length field - 1", "udp: length field 7", "udp of 7 octets", "tcp: data offset 4",
                     "tcp: data offset 15", "tcp segment of 19 octets", "tcp: source port 0", "udp: destination port 0",
                     "icmp of 3 octets", "icmp of 7 octets", "igmp of 7 octets"):
            assert f"{what}, {g}" in names
    assert "udp payload 4: checksum computes to 0, sent as 0xffff" in names and "tcp payload 4: checksum computes to 0, field 0xffff" in names
    lens = [len(d) for d in dgrams[1]]
    assert min(lens) == 0 and max(lens) == 20 + 36 + 8980 and sum(n <= 100 for n in lens) > len(lens) // 2
    for c, d in zip(fx["cases"], dgrams[1]):
        assert len(d) == c["n"] and d[:iv.HEAD].hex() == c["head"], c["name"]


@pytest.mark.parametrize("lib", iv.LIBS)
def test_flags_actions_and_checksum_calls_follow_the_recorded_reference(fx, dgrams, ours, lib):
    names, dg, _ = dgrams
    recs = iv.outcomes_of(fx, lib)
    kinds = [check_rules(nm, d, r, flags, netcsum.rx_action(flags, proto, len(d) > 0 and d[0] >> 4 == 6, RX_CFG[lib]), calls)
             for nm, d, r, (flags, proto, calls) in zip(names, dg, recs, ours)]
    assert kinds.count("drop") and kinds.count("exception")


def shares_of(fx, dgrams, ours, lib):
    names, dg, _ = dgrams
    recs = iv.outcomes_of(fx, lib)
    witnesses, drops, exceptions, exc_ctrs = dict.fromkeys(range(1, 7), 0), 0, 0, {}
    for nm, d, r, (flags, proto, calls) in zip(names, dg, recs, ours):
        action = netcsum.rx_action(flags, proto, len(d) > 0 and d[0] >> 4 == 6, RX_CFG[lib])
        kind = check_rules(nm, d, r, flags, action, calls)
        if kind:
            drops += 1
        if kind == "drop":
            witnesses[action] += 1
        elif kind == "exception":
            exceptions += 1
            for k in (PRECEDING.get(action, set()) | {"IPv4.RxInvVerCtr"}) & set(r["ctr"]):
                exc_ctrs[k] = exc_ctrs.get(k, 0) + 1
    no_call = sum(not r["calls"] for r in recs)
    return witnesses, drops, exceptions, exc_ctrs, no_call, len(recs)


def test_shares(fx, dgrams, ours):
    """The three shares, printed, within their caps."""
    for lib in iv.LIBS:
        witnesses, drops, exceptions, exc_ctrs, no_call, n = shares_of(fx, dgrams, ours, lib)
        print(f"{lib}: rule-1 witnesses per DROP code {witnesses}; exception rows {exceptions} of {drops} DROP rows "
              f"({100 * exceptions / drops:.1f} %): {dict(sorted(exc_ctrs.items()))}; no reference checksum call: {no_call} of {n} "
              f"({100 * no_call / n:.1f} %)")
        for code, w in witnesses.items():
            if code != UDP_NO_CHK_SUM or lib == "udpdis":
                assert w >= 20, (lib, code, w)
        assert witnesses[UDP_NO_CHK_SUM] == 0 or lib == "udpdis"
        assert 4 * exceptions <= drops, (lib, exceptions, drops)
        assert 3 * no_call <= n, (lib, no_call, n)


def test_ipparse_rules_equal_the_oracle_on_every_datagram(dgrams, ours, exe):  # noqa: F811
    """netcsum_ipparse.h, the rules the kernels share, at the smallest and largest window limits and at the
    datagram's own length: the flags the rules above were checked on."""
    names, dg, _ = dgrams
    lines, want = [], []
    for nm, d, (flags, _, _) in zip(names, dg, ours):
        for limit in LIMITS:
            lines.append(f"{d.hex() or '-'} {len(d)} {len(d) if limit is None else limit} 0 1 0\n")
            want.append((nm, limit, flags))
    out = run(exe, lines)
    for (nm, limit, flags), line in zip(want, out):
        assert line.split()[0] != "DEFER" and int(line.split()[0], 16) == flags, (nm, limit, line, hex(flags))


# ------------------------------------------------------------------ with the reference libraries
@needs_ref
def test_recorder_check_reproduces_the_committed_fixture():
    with open(iv.FIXTURE) as f:
        assert f.read() == rec.generate()
