"""Fragment payload sums, host side (include/netcsum_mi355x.h (2b''')), no kernel launches:

* NetUtil_MI355X_FragSumCalc / FragSumVerify over per-fragment records equal the oracle's DataCalc /
  DataVerify over the chain of the fragments' NET_BUFs (oracle/net_util_oracle.c, the reference's
  own walk), for random TCP / UDP / ICMP datagrams cut the way the stack accepts fragments
  (multiples of 8, a last piece of any length) and for any other cut (odd and empty middle pieces),
  with the 12-B IPv4 and 40-B IPv6 pseudo-headers, one corrupted bit, all-zero payloads, 0 / 1 / 2 /
  45 fragments and the 65 535-octet bound. Each record's sum is the oracle's one-buffer DataCalc of
  that piece, complemented: what NetUtil_MI355X_RxBurstSums reports.
* the new burst entry points reject bad arguments before any device work;
* tests/c_frag/frag_caller.c (its own main, its own expectations) builds with
  -fsanitize=address,undefined from host code alone and exits 0.
"""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import netcsum
import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_NULL, E_ARG = netcsum.NET_UTIL_ERR_NONE, netcsum.NET_ERR_FAULT_NULL_PTR, netcsum.NET_UTIL_ERR_MI355X_INVALID_ARG
TCP4 = netcsum.NET_PROTOCOL_TYPE_TCP_V4


def piece_record(piece: bytes):
    """The record RxBurstSums defines for a fragment whose IP payload is `piece`."""
    if not piece:
        return (0, 0)
    ch = netcsum.Chain([{"data": piece, "proto": TCP4, "offset": 2}])
    v, err = oracle.data_calc(ch.ptr, None, 0)
    assert err == OK
    return ((~v) & 0xFFFF, len(piece))


def oracle_chain(pieces, pseudo):
    """(DataCalc, DataVerify) of the reference over the chain of the pieces' buffers."""
    ch = netcsum.Chain([{"data": p, "proto": TCP4, "offset": 2 + (i & 1)} for i, p in enumerate(pieces)])
    ph = netcsum.HostBytes(pseudo, 1) if pseudo is not None else None
    args = (ch.ptr, ph.ptr if ph else None, len(pseudo) if pseudo is not None else 0)
    c, e1 = oracle.data_calc(*args)
    v, e2 = oracle.data_verify(*args)
    assert e1 == OK and e2 == OK
    return c, v


def check(pieces, pseudo):
    recs = [piece_record(p) for p in pieces]
    want_c, want_v = oracle_chain(pieces, pseudo)
    assert netcsum.frag_sum_calc(recs, pseudo) == (want_c, OK)
    assert netcsum.frag_sum_verify(recs, pseudo) == (want_v, OK)
    return want_v


def datagram(rng, kind, n, v6):
    """A finalized transport datagram of n octets and its pseudo-header (None for ICMPv4)."""
    src, dst = rng.randbytes(16 if v6 else 4), rng.randbytes(16 if v6 else 4)
    proto = {"tcp": 6, "udp": 17, "icmp": 58 if v6 else 1}[kind]
    pseudo = (src + dst + struct.pack("!IHBB", n, 0, 0, proto)) if v6 else (src + dst + struct.pack("!BBH", 0, proto, n))
    if kind == "icmp" and not v6:
        pseudo = None
    field = {"tcp": 16, "udp": 6, "icmp": 2}[kind]
    body = bytearray(rng.randbytes(n))
    if n >= field + 2:
        body[field:field + 2] = b"\0\0"
        c, _ = oracle_chain([bytes(body)], pseudo)
        body[field:field + 2] = struct.pack("=H", c)            # the host-order value, memcpy'd
    return bytes(body), pseudo


def cut_mf(rng, data, n_frag):
    """n_frag pieces: multiples of 8, then a last piece of any length (net_ipv4.c:5320-5334)."""
    units = (len(data) - 1) // 8
    n_frag = max(1, min(n_frag, units + 1))
    marks = sorted(rng.sample(range(1, units + 1), n_frag - 1)) if n_frag > 1 else []
    edges = [0] + [8 * m for m in marks] + [len(data)]
    return [data[a:b] for a, b in zip(edges, edges[1:])]


@pytest.mark.parametrize("v6", [False, True])
@pytest.mark.parametrize("kind", ["tcp", "udp", "icmp"])
def test_fragment_records_add_up_to_the_reference(kind, v6):
    rng = random.Random(f"{kind}{v6}")
    sizes = [8, 9, 24, 1480, 1481, 2960, 65515] + [rng.randint(8, 65515) for _ in range(8)]
    for n in sizes:
        data, pseudo = datagram(rng, kind, n, v6)
        for n_frag in (1, 2, rng.randint(3, 44), 45):
            pieces = cut_mf(rng, data, n_frag)
            if n >= 24:
                assert check(pieces, pseudo) == 1                # finalized: the reference accepts it
            bad = bytearray(data)
            bad[rng.randrange(n)] ^= 1 << rng.randrange(8)
            cuts = np.cumsum([0] + [len(p) for p in pieces])
            assert check([bytes(bad[a:b]) for a, b in zip(cuts, cuts[1:])], pseudo) == 0


def test_any_lengths_odd_and_empty_middle_pieces():
    rng = random.Random(7)
    for t in range(300):
        pieces = [rng.randbytes(0 if rng.random() < 0.2 else rng.randint(1, 301)) for _ in range(rng.randint(2, 7))]
        if sum(map(len, pieces)) == 0:
            pieces[0] = b"\x01"
        pseudo = [None, rng.randbytes(12), rng.randbytes(40), rng.randbytes(11)][t % 4]
        check(pieces, pseudo)
    data, pseudo = datagram(rng, "udp", 1013, False)
    assert check([data[:8], data[8:15], data[15:16], data[16:]], pseudo) == 1     # odd-length middle pieces


def test_all_zero_payloads_and_the_null_chain():
    z12 = bytes(12)
    for pieces in ([bytes(1480), bytes(333)], [bytes(8)], [bytes(7), bytes(9)]):
        assert [piece_record(p)[0] for p in pieces] == [0] * len(pieces)
        check(pieces, z12)
        check(pieces, None)
        assert netcsum.frag_sum_calc([piece_record(p) for p in pieces], z12) == (0xFFFF, OK)
    # n_frag == 0: the reference's NULL chain (an odd pseudo-header's last octet is never summed)
    for pseudo in (None, b"\x12\x34\x56", bytes(range(12)), bytes(range(40)), bytes(range(11))):
        ph = netcsum.HostBytes(pseudo) if pseudo is not None else None
        args = (None, ph.ptr if ph else None, len(pseudo) if pseudo else 0)
        assert netcsum.frag_sum_calc([], pseudo) == (oracle.data_calc(*args)[0], OK)
        assert netcsum.frag_sum_verify([], pseudo) == (oracle.data_verify(*args)[0], OK)


def test_total_length_bound_and_null_arguments():
    rng = random.Random(11)
    data, pseudo = datagram(rng, "tcp", 65535, False)
    assert check([data[:65528], data[65528:]], pseudo) == 1                         # 65 535 octets: inside
    assert check([data[:1], data[1:]], pseudo) == 1
    over = [(1, 65528), (2, 8)]                                                     # 65 536: refused
    assert netcsum.frag_sum_calc(over, pseudo)[1] == E_ARG
    assert netcsum.frag_sum_verify(over, pseudo)[1] == E_ARG
    assert netcsum.frag_sum_verify([(1, 65535)] * 70000, None)[1] == E_ARG          # (no 32-bit wrap of the total)
    L = netcsum.lib()
    rec = np.array([[1, 8]], np.uint16)
    out16, out8 = np.zeros(1, np.uint16), np.zeros(1, np.uint8)
    assert L.NetUtil_MI355X_FragSumCalc(None, 1, None, 0, out16.ctypes.data_as(L.NetUtil_MI355X_FragSumCalc.argtypes[4])) == E_NULL
    assert L.NetUtil_MI355X_FragSumCalc(rec.ctypes.data, 1, None, 0, None) == E_NULL
    assert L.NetUtil_MI355X_FragSumCalc(rec.ctypes.data, 1, None, 12, out16.ctypes.data_as(L.NetUtil_MI355X_FragSumCalc.argtypes[4])) == E_NULL
    assert L.NetUtil_MI355X_FragSumVerify(None, 1, None, 0, out8.ctypes.data_as(L.NetUtil_MI355X_FragSumVerify.argtypes[4])) == E_NULL
    assert L.NetUtil_MI355X_FragSumVerify(rec.ctypes.data, 1, None, 0, None) == E_NULL


def test_burst_sums_check_arguments_before_device_work():
    """RxBurst's / RxBurstHost's checks, then the sums array: all before any device work (so on a
    host without a GPU too); n_pkt == 0 succeeds."""
    L = netcsum.lib()
    assert L.NetUtil_MI355X_RxBurstSums(None, None, None, 64, 64, 0, 0, None, None, None, None) == OK
    assert L.NetUtil_MI355X_RxBurstSums(16, None, None, 64, 64, 3, 0, None, None, 16, None) == E_NULL     # actions
    assert L.NetUtil_MI355X_RxBurstSums(16, None, None, 64, 64, 3, 4, 16, None, 16, None) == E_ARG        # rx_cfg
    assert L.NetUtil_MI355X_RxBurstSums(16, None, None, 64, 64, 3, 2, 16, None, 16, None) == E_ARG
    assert L.NetUtil_MI355X_RxBurstSums(16, None, None, 64, 64, 3, 0, 16, None, None, None) == E_NULL     # sums
    assert L.NetUtil_MI355X_RxBurstSums(16, None, None, 64, 64, 3, 0, 16, None, 18, None) == E_ARG        # alignment
    assert L.NetUtil_MI355X_RxBurstSums(None, None, None, 64, 64, 3, 0, 16, None, 16, None) == E_NULL     # base
    assert L.NetUtil_MI355X_RxBurstSums(16, 16, None, 64, 64, 3, 0, 16, None, 16, None) == E_NULL         # off w/o len
    assert L.NetUtil_MI355X_RxBurstSumsHost(None, None, None, 64, 64, 0, 0, None, None, None, 4) == OK
    assert L.NetUtil_MI355X_RxBurstSumsHost(8, None, None, 64, 64, 3, 0, None, None, 8, 4) == E_NULL      # actions
    assert L.NetUtil_MI355X_RxBurstSumsHost(8, None, None, 64, 64, 3, 4, 8, None, 8, 4) == E_ARG          # rx_cfg
    assert L.NetUtil_MI355X_RxBurstSumsHost(8, None, None, 64, 64, 3, 0, 8, None, None, 4) == E_NULL      # sums
    assert L.NetUtil_MI355X_RxBurstSumsHost(None, None, None, 64, 64, 3, 0, 8, None, 8, 4) == E_NULL      # base
    assert L.NetUtil_MI355X_RxBurstSumsHost(8, 8, None, 64, 64, 3, 0, 8, None, 8, 4) == E_NULL            # off w/o len
    buf, act, sums = np.zeros(64 * 4, np.uint8), np.zeros(4, np.uint8), np.zeros(3, np.uint32)
    with pytest.raises(ValueError):                                                 # 4 records needed, 3 held
        netcsum.rx_burst_sums_host(buf, 4, act, sums, stride=64, pkt_len=64)
    with pytest.raises(ValueError):
        netcsum.rx_burst_sums(buf, 4, act, sums, stride=64, pkt_len=64, stream=0)
    with pytest.raises(ValueError):
        netcsum.rx_burst_sums(buf, 5, act, np.zeros(5, np.uint32), stride=64, pkt_len=64, stream=0)   # packets


def test_c_caller_under_sanitizers(tmp_path):
    exe = str(tmp_path / "frag_caller_asan")
    cmd = ["gcc", "-std=c99", "-D_DEFAULT_SOURCE", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pedantic",
           "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c_frag", "frag_caller.c"),
           os.path.join(REPO, "uc-tcp-ip_amd", "host", "netcsum_fragsum.c"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert r.stdout.startswith("frag_caller ok")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
