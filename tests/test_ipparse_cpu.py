"""The packet kernels' IP parse and verdict rules on the CPU (uc-tcp-ip_amd/csrc/netcsum_ipparse.h, the
one statement of them that the run-stream kernels, the lane-group kernels and the extension-header
walk include): tests/c_ipparse/ipparse_caller.cpp, a stand-alone program, includes the same header as
plain C++ with an accessor over a byte array, built here with -fsanitize=address,undefined -Wall
-Wextra -Werror and run as a subprocess (nothing is loaded into Python).

Corpus: every kind of make_packet / make_packet_v6 with payloads of 0, 1 and up to 64 octets; IPv4
with every IHL 5..15; Routing-header chains of 1..5 headers of 1..3 units (the chains the window rules
walk themselves); the long-chain outcomes of test_gpu_packets_v6.py; truncations of one datagram of every kind, IHL and chain
(avail 0, 19, 20, 39, 40, total length - 1). Every datagram is judged at every window limit the kernels have — 81..96 (run
stream, 96 - lead), 113..128, 241..256, 497..512, 1009..1024 (lane groups of 8 / 16 / 32 / 64,
16 G - lead) — and at limit = len(datagram), as Rx, as Rx with fragment sums, and as Tx under the three UDP
checksum settings (none, all, per datagram):

1. a datagram that is not DEFER equals oracle_packets.rx_validate_ip (Rx) / tx_finalize_ip (Tx: flags
   and written bytes); with sums, its fragment record equals test_fragsum_cpu.piece_record of the
   oracle's payload;
2. DEFER is never given to an IPv4 datagram;
3. nor to an IPv6 datagram whose next header at offset 6 is 6 / 17 / 58 / 44 or no extension value;
4. / 5. DEFER goes exactly to the datagrams `defers` names: a chain that holds something other than up
   to four accepted Routing headers, a Routing header whose first 8 octets (off + 8) or transport fields
   behind Routing headers (off + 24) pass the limit, and, with sums, a fragment whose Fragment header
   (off + 8) passes it. A condition, not a sample: at limit = len(datagram) only the first applies,
   unless the datagram itself ends inside those octets.
The program's accessor exits with an error on any read outside [16 MinOff, limit) or past `avail`, so
the run also shows that the rules stay inside the window they are given.
For IPv4 it also takes the run-stream lane's route — the header step alone, then the transport step
called by itself — and exits with an error if that classification differs from the whole one.

The datagrams the window rules defer are also judged the way the walk judges them (the chain walked by
the oracle, then the shared transport and verdict steps with the whole datagram as window).

Deferred share of this corpus, counted on the CPU (Rx, each datagram once per limit): of 178 IPv6
datagrams, 81 (46 %) are deferred at limit 81 and 73 (41 %) at limit 96; 54 % are judged at limit 81. Over
all rows (datagrams x 81 limits x 5 modes, truncations included) 544 925 are judged and 27 340 deferred.
"""
import os
import random
import struct
import subprocess

import pytest

import netcsum
import oracle_packets as op
import test_fragsum_cpu as fs
from packets import KINDS, KINDS6, LONG_TAILS, _ext_chain, long_chain_pkts, long_prefix_pkt, make_packet, make_packet_v6

REPO = netcsum.REPO
LIMITS = [*range(81, 97), *range(113, 129), *range(241, 257), *range(497, 513), *range(1009, 1025)]
MODES = [(0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 0, 0), (1, 2, 0)]  # (tx, udp_tx_csum, sums)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ipparse") / "ipparse_caller_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-I" + os.path.join(REPO, "include"),
           "-I" + os.path.join(REPO, "uc-tcp-ip_amd", "csrc"), os.path.join(REPO, "tests", "c_ipparse", "ipparse_caller.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(exe, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def with_ihl(rng, pkt, ihl, udp_tx_csum):
    """The IPv4 datagram `pkt` (IHL 5) with 4 * (ihl - 5) option octets, finalized again."""
    opts = rng.randbytes(4 * (ihl - 5))
    b = bytearray(pkt[:20] + opts + pkt[20:])
    b[0] = 0x40 | ihl
    b[2:4] = struct.pack("!H", len(b))
    return op.tx_finalize(bytes(b), udp_tx_csum)[0]


def routing_chain_pkt(rng, n_hdrs, units, inner_kind):
    inner = make_packet_v6(rng, inner_kind, payload=rng.choice([0, 1, rng.randint(2, 40)]))
    nh, ext = _ext_chain(rng, [(43, units)] * n_hdrs, inner[6])
    body = ext + inner[40:]
    p = inner[:4] + struct.pack("!HB", len(body), nh) + inner[7:40] + body
    return op.tx_finalize_v6(p, udp_tx_csum=(inner_kind != "udp0"))[0]


@pytest.fixture(scope="module")
def corpus():
    """[(name, datagram octets, avail)]"""
    rng = random.Random(20)
    rows = []
    for kind in dict.fromkeys(KINDS):
        for payload in (0, 1, rng.randint(2, 64)):
            rows.append((f"v4 {kind} {payload}", make_packet(rng, kind, payload)))
    for kind in ("tcp", "udp", "udp0", "icmp", "igmp", "frag", "other", "udp_badlen"):
        for ihl in range(5, 16):
            p = make_packet(rng, kind, rng.choice([0, 1, 9]))
            while p[0] & 0xF != 5:
                p = make_packet(rng, kind, rng.choice([0, 1, 9]))
            q = with_ihl(rng, p, ihl, kind != "udp0")
            if kind == "udp_badlen":                             # (finalizing leaves a bad length alone)
                assert op.rx_validate(q) & op.L4_MALFORMED
            rows.append((f"v4 {kind} ihl {ihl}", q))
    for kind in dict.fromkeys(KINDS6):
        for payload in (0, 1, rng.randint(2, 64)) if kind.startswith("ext") else (0, 1, 8, 9, rng.randint(2, 64), rng.randint(2, 64)):
            rows.append((f"v6 {kind} {payload}", make_packet_v6(rng, kind, payload)))
    for n_hdrs in range(1, 6):                                   # 8..120 octets of Routing headers
        for units in (1, 2, 3):
            inside = n_hdrs * units <= 2                         # transport fields inside every window
            for inner in ("tcp", "udp", "udp0", "icmp_echo", "icmp_err", "tcp_short") if inside else ("tcp", "udp"):
                rows.append((f"v6 rt x{n_hdrs} u{units} {inner}", routing_chain_pkt(rng, n_hdrs, units, inner)))
    for tail in LONG_TAILS:
        for big in (17, 129):
            rows.append((f"v6 long {tail} {big}", long_prefix_pkt(rng, tail, big)))
    for k, p in enumerate(long_chain_pkts(rng, 3, n_hdrs=(1, 4, 5), reps=1)):
        rows.append((f"v6 chain {k}", p))
    out = [(n, p, len(p)) for n, p in rows]
    first = {}                                                   # truncations: one datagram of every kind / chain / IHL
    for n, p in rows:
        first.setdefault(n.rsplit(" ", 1)[0] if n.startswith(("v4", "v6 ")) and " ihl " not in n and " rt " not in n
                         and " long " not in n else n, (n, p))
    for n, p in first.values():
        tot = (40 + struct.unpack("!H", p[4:6])[0]) if p[0] >> 4 == 6 else struct.unpack("!H", p[2:4])[0]
        for avail in sorted({0, 19, 20, 39, 40, max(tot - 1, 0)}):
            if avail < len(p):
                out.append((f"{n} avail {avail}", p, avail))
    return out


def defers(p, limit, sums):
    """Is the IPv6 datagram p (all octets present) left to the walk pass by a window of `limit` octets?"""
    if len(p) < 40 or p[0] >> 4 != 6:
        return False
    tot = 40 + struct.unpack("!H", p[4:6])[0]
    if tot > len(p):
        return False
    nh, off = p[6], 40
    for _ in range(4):
        if nh != 43:
            break
        if off + 8 > limit or (p[off + 2] > 2 and p[off + 3] != 0):
            return True
        nh, off = p[off], off + (p[off + 1] + 1) * 8
        if off > tot:
            return False                                          # MALFORMED
    if nh == 44:
        return bool(sums) and off + 8 < tot and off + 8 > limit
    if nh in op.IPV6_EXT:
        return True
    return off != 40 and off + 24 > limit


def frag_record(p):
    """The fragment record the oracle's view of datagram p gives (0, 0 unless it is a fragment with payload)."""
    if not p:
        return (0, 0)
    if p[0] >> 4 == 6:
        q = op._parse6(p)
        if q is None or q[0] != op.FRAGMENT:
            return (0, 0)
        return fs.piece_record(p[q[1] + 8:40 + struct.unpack("!H", p[4:6])[0]])
    q = op._parse(p)
    if q is None or not q[2]:
        return (0, 0)
    return fs.piece_record(p[q[0]:q[1]])


def udp_field(p):
    """The UDP checksum field of datagram p as the oracle finds it (None: not a UDP datagram it would finalize)."""
    if p and p[0] >> 4 == 6:
        q = op._parse6(p)
        off = q[1] if q is not None and q[0] == 0 and q[3] == 17 else None
    else:
        q = op._parse(p)
        off = q[0] if q is not None and not q[2] and q[3] == 17 else None
    return None if off is None or off + 8 > len(p) else struct.unpack("!H", p[off + 6:off + 8])[0]


def expected(p, tx, udp, sums):
    """The program's output line for datagram p (the octets present) when it is judged."""
    if not tx:
        rec = frag_record(p) if sums else (0, 0)
        return (op.rx_validate_ip(p), None, rec)
    if udp == 2:                                                 # per datagram: a UDP field of 0 is left 0, any other computed
        udp = udp_field(p) not in (None, 0)
    done, flags = op.tx_finalize_ip(p, bool(udp))
    return (flags, done, (0, 0))


def check_line(name, p, tx, got, want):
    flags, cip, cl4, l4off, fsum, flen = got.split()
    assert int(flags, 16) == want[0], (name, got, want[0])
    assert (int(fsum, 16), int(flen)) == want[2], (name, got, want[2])
    if not tx:
        assert cip == "-" and cl4 == "-", (name, got)
        return
    b = bytearray(p)
    if cip != "-":
        b[10:12] = int(cip, 16).to_bytes(2, "little")            # the host-order value, memcpy'd
    if cl4 != "-":
        b[int(l4off):int(l4off) + 2] = int(cl4, 16).to_bytes(2, "little")
    assert bytes(b) == want[1], (name, got)


def test_window_rules_equal_the_oracle_at_every_limit(exe, corpus):
    lines, meta = [], []
    for name, p, avail in corpus:
        for k, limit in enumerate(LIMITS + [len(p)]):
            for tx, udp, sums in MODES:
                lines.append(f"{p[:avail].hex() or '-'} {avail} {limit} {tx} {udp} {sums}\n")
                meta.append((name, p[:avail], limit, tx, udp, sums, k < len(LIMITS) and avail == len(p)))
    out = run(exe, lines)
    cache, judged, deferred = {}, 0, 0
    v6_at = {81: [0, 0], 96: [0, 0]}                              # limit: [deferred, all] (Rx, no sums)
    for got, (name, p, limit, tx, udp, sums, count) in zip(out, meta):
        v6 = len(p) > 0 and p[0] >> 4 == 6
        want_defer = defers(p, limit, sums)
        assert (got == "DEFER") == want_defer, (name, limit, tx, sums, got)
        if got == "DEFER":
            deferred += 1
            assert v6, name                                       # (2)
            assert p[6] in op.IPV6_EXT and p[6] != 44, name       # (3)
        else:
            judged += 1
            key = (p, tx, udp, sums)
            if key not in cache:
                cache[key] = expected(p, tx, udp, sums)
            check_line(f"{name} limit {limit}", p, tx, got, cache[key])
        if v6 and count and limit in v6_at and (tx, sums) == (0, 0):
            v6_at[limit][0] += got == "DEFER"
            v6_at[limit][1] += 1
    print(f"judged {judged}, deferred {deferred}; IPv6 datagrams deferred at limit 81: {v6_at[81]}, at 96: {v6_at[96]}")
    assert judged > deferred > 0
    assert 2 * v6_at[81][0] < v6_at[81][1]                        # more than half judged at the smallest window


def test_walked_datagrams_get_the_oracle_s_verdict(exe, corpus):
    """The walk's use of the shared steps: the oracle walks the chain (any length), the program judges the
    transport header it ends at with the datagram as the window."""
    lines, meta = [], []
    for name, p, avail in corpus:
        q = op._parse6(p[:avail]) if avail and p[0] >> 4 == 6 else None
        if q is None or q[0] != 0:                                # malformed, or decided by the chain alone
            continue
        tot = 40 + struct.unpack("!H", p[4:6])[0]
        for tx, udp, sums in MODES:
            lines.append(f"{p.hex()} {avail} {tot} {tx} {udp} {sums} {q[3]} {q[1]}\n")
            meta.append((name, p[:avail], tx, udp, sums))
    out = run(exe, lines)
    assert len({m[0] for m in meta if m[0].startswith("v6 long")}) >= 20
    for got, (name, p, tx, udp, sums) in zip(out, meta):
        assert got != "DEFER", name
        check_line(name + " (walk)", p, tx, got, expected(p, tx, udp, sums))
