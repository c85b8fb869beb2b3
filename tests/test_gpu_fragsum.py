"""GPU parity of NetUtil_MI355X_RxBurstSums (include/netcsum_mi355x.h (2b''')).

Bursts of 1, 63, 64, 65 and 200 frames (a wave's run is 64 packets) in the layouts a driver hands
over — packed offset/length batches with odd starts, 1520-B pool slots with the frame at +14, 2-KiB
slots — with a raised share of fragments: IPv4 with IHL 5 .. 15, More Fragments only / offset only /
both, payloads of 0, 1, 7, 8, 9, 1479 and 1480 octets, some with a bad header checksum; IPv6 with the
Fragment header right after the fixed header, behind a Destination Options header (the walk), behind
routing headers inside and past the lane's window, and behind a chain of > 1 KiB (the walk).

* action / flags: what rx_burst writes on the same batch, and the oracle's
  (oracle_packets.rx_validate_ip, netcsum.rx_action);
* sums[i] of a fragment: its payload length and (uint16_t)~DataCalc of one NET_BUF holding exactly
  its payload octets (the oracle's DataCalc); {0, 0} for every other frame;
* end to end: finalized TCP / UDP datagrams over IPv4 and IPv6 cut into fragment frames, scattered
  through a burst, half of them with one corrupted bit: FragSumVerify over the GPU's records equals
  the oracle's DataVerify of the reassembled chain;
* the lane-group kernel and its walk pass (TUNE_KERNEL 2), and the host-memory form.
"""
import functools
import random
import struct

import numpy as np
import pytest

import netcsum
import oracle
import oracle_offload as oo
import oracle_packets as op
from packets import KINDS, KINDS6, _ext_chain, make_packet, make_packet_v6, packed_batch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
TCP4 = netcsum.NET_PROTOCOL_TYPE_TCP_V4
PAYLOADS = [0, 1, 7, 8, 9, 1479, 1480]
MAX_FRAME = 1500


def v4_fragment(rng, payload: bytes, ihl=5, frag=0x2000, proto=17, ident=None, src=None, dst=None, bad_ip=False):
    hdr = struct.pack("!BBHHHBBH4s4s", (4 << 4) | ihl, 0, ihl * 4 + len(payload), rng.getrandbits(16) if ident is None else ident,
                      frag, 64, proto, 0, src or rng.randbytes(4), dst or rng.randbytes(4))
    pkt, _ = op.tx_finalize(hdr + rng.randbytes(ihl * 4 - 20) + payload)     # (a fragment: the IP checksum only)
    if bad_ip:
        b = bytearray(pkt)
        b[8] ^= 0x10
        pkt = bytes(b)
    return pkt


def v6_fragment(rng, payload: bytes, chain=(), nh=17, offset_mf=1, ident=None, src=None, dst=None):
    """Fixed header, the extension headers `chain` ((type, units of 8 B) each), the Fragment header."""
    first, ext = _ext_chain(rng, list(chain) + [(44, 1)], nh)
    ext = bytearray(ext)
    ext[-6:] = struct.pack("!HI", offset_mf, rng.getrandbits(32) if ident is None else ident)   # after nh, reserved
    body = bytes(ext) + payload
    return struct.pack("!IHBB16s16s", (6 << 28) | rng.getrandbits(20), len(body), first, 64, src or rng.randbytes(16),
                       dst or rng.randbytes(16)) + body


V6_CHAINS = [(), ((60, 1),), ((43, 1),), ((43, 2), (43, 1)), ((43, 6),), ((0, 1), (43, 1)), ((60, 130),)]


def fragment_mix(rng, n):
    """n frames <= MAX_FRAME octets: about half fragments, the rest the packet generators' kinds."""
    out = []
    for ihl in (5, 6, 15):
        for pay in PAYLOADS:
            if ihl * 4 + pay <= MAX_FRAME:
                frag = rng.choice([0x2000, rng.randint(1, 0x1FFF), 0x2000 | rng.randint(1, 0x1FFF)])
                out.append(v4_fragment(rng, rng.randbytes(pay), ihl, frag, rng.choice([6, 17, 1]), bad_ip=rng.random() < 0.15))
    for chain in V6_CHAINS:
        room = MAX_FRAME - 48 - 8 * sum(u for _, u in chain)
        for pay in [p for p in PAYLOADS if p <= room] + [room]:
            out.append(v6_fragment(rng, rng.randbytes(pay), chain, rng.choice([6, 17, 58]), rng.choice([1, 8, 0x5B9])))
    out.append(v4_fragment(rng, bytes(1480)))                       # all-zero payloads: sum 0
    out.append(v6_fragment(rng, bytes(64)))
    rng.shuffle(out)
    out = out[:max(1, n // 2)]
    kinds4 = KINDS + ["frag"] * 4
    kinds6 = KINDS6 + ["ext_frag"] * 4
    while len(out) < n:
        mk, kinds = (make_packet, kinds4) if rng.random() < 0.5 else (make_packet_v6, kinds6)
        p = mk(rng, rng.choice(kinds), payload=rng.randint(0, 1300))
        if len(p) <= MAX_FRAME:
            out.append(p)
    rng.shuffle(out)
    return out


def frag_payload(pkt: bytes):
    """The IP payload of a frame the oracle flags FRAGMENT (and not MALFORMED), else None."""
    f = op.rx_validate_ip(pkt)
    if not f & op.FRAGMENT or f & op.MALFORMED:
        return None
    if pkt[0] >> 4 == 4:
        hlen, tot = (pkt[0] & 0xF) * 4, struct.unpack("!H", pkt[2:4])[0]
        return pkt[hlen:tot]
    _, off, _, nh, _ = op._parse6(pkt)
    assert nh == 44
    return pkt[off + 8:40 + struct.unpack("!H", pkt[4:6])[0]]


def want_record(pkt: bytes):
    pay = frag_payload(pkt)
    if not pay:
        return 0
    ch = netcsum.Chain([{"data": pay, "proto": TCP4, "offset": 2}])
    v, err = oracle.data_calc(ch.ptr, None, 0)
    assert err == netcsum.NET_UTIL_ERR_NONE
    return ((~v) & 0xFFFF) | (len(pay) << 16)


def want_all(frames):
    f = np.array([op.rx_validate_ip(p) for p in frames], np.uint8)
    a = np.array([netcsum.rx_action(int(x), oo.transport_proto(p), len(p) and p[0] >> 4 == 6, 0) for x, p in zip(f, frames)],
                 np.uint8)
    return f, a, np.array([want_record(p) for p in frames], np.uint32)


@functools.lru_cache(maxsize=None)
def burst(n):
    """The n-frame burst and, per layout, its buffer and the oracle's verdicts (computed once)."""
    rng = random.Random(1000 + n)
    frames = fragment_mix(rng, n)
    out = {}
    buf, offs, lens = packed_batch(frames, rng, lead=1)
    out["packed"] = (buf, offs, lens, 0, 0, 0, want_all([bytes(buf[x:x + y]) for x, y in zip(offs, lens)]))
    for name, stride, lead, pkt_len in (("pool1520", 1520, 14, 1506), ("slot2k", 2048, 64, 1536)):
        buf = np.frombuffer(rng.randbytes(lead + n * stride + 128), np.uint8).copy()
        for i, p in enumerate(frames):
            buf[lead + i * stride:lead + i * stride + len(p)] = np.frombuffer(p, np.uint8)
        present = [bytes(buf[lead + i * stride:lead + i * stride + pkt_len]) for i in range(n)]
        out[name] = (buf, None, None, stride, lead, pkt_len, want_all(present))
    return out


def run_sums(layout, n, sums_fn=True):
    buf, offs, lens, stride, lead, pkt_len, want = burst(n)[layout]
    b = torch.from_numpy(buf).to(DEV)
    act = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    fl = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    sums = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    kw = dict(flags=fl)
    if offs is not None:
        kw.update(off=torch.from_numpy(offs.astype(np.int64)).to(DEV), lens=torch.from_numpy(lens.view(np.int16)).to(DEV))
        base = b
    else:
        kw.update(stride=stride, pkt_len=pkt_len)
        base = b[lead:]
    if sums_fn:
        netcsum.rx_burst_sums(base, n, act, sums, **kw)
        assert ",sums>" in netcsum.last_launch()                         # the SUMS instantiations
    else:
        netcsum.rx_burst(base, n, act, **kw)
    torch.cuda.synchronize()
    return act.cpu().numpy(), fl.cpu().numpy(), sums.cpu().numpy().view(np.uint32), want


def check_records(got, want):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("layout", ["packed", "pool1520", "slot2k"])
def test_rx_burst_sums_layouts(layout, n):
    act, fl, sums, (want_f, want_a, want_s) = run_sums(layout, n)
    act0, fl0, _, _ = run_sums(layout, n, sums_fn=False)
    assert np.array_equal(fl, fl0) and np.array_equal(act, act0)         # byte for byte rx_burst's
    assert np.array_equal(fl, want_f), np.nonzero(fl != want_f)[0][:10]
    assert np.array_equal(act, want_a), np.nonzero(act != want_a)[0][:10]
    check_records(sums, want_s)
    if n >= 63:                                                          # the mix holds what it should
        frag = (want_f & op.FRAGMENT) != 0
        assert frag.sum() >= n // 4 and (want_s[frag] != 0).sum() >= n // 5 and not want_s[~frag].any()


def test_rx_burst_sums_lane_group_kernel_and_walk_pass():
    netcsum.tune(netcsum.TUNE_KERNEL, 2)
    try:
        for layout in ("packed", "pool1520"):
            act, fl, sums, (want_f, want_a, want_s) = run_sums(layout, 200)
            assert netcsum.last_launch().startswith("pkt_batch_kernel") and "sums" in netcsum.last_launch()
            assert np.array_equal(fl, want_f) and np.array_equal(act, want_a)
            check_records(sums, want_s)
    finally:
        netcsum.tune(netcsum.TUNE_KERNEL, 0)


@pytest.mark.parametrize("n_chunks", [0, 3, 7])
def test_rx_burst_sums_host_form(n_chunks):
    """7 chunks (6 of 29 frames and one of 26): every pipeline slot is reused, and the last chunk is short."""
    n = 200
    for layout in ("packed", "pool1520"):
        buf, offs, lens, stride, lead, pkt_len, (want_f, want_a, want_s) = burst(n)[layout]
        act, fl, sums = np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8), np.full(n, 0x5A5A5A5A, np.uint32)
        if offs is not None:
            netcsum.rx_burst_sums_host(buf, n, act, sums, flags=fl, off=offs, lens=lens, n_chunks=n_chunks)
        else:
            netcsum.rx_burst_sums_host(buf[lead:], n, act, sums, flags=fl, stride=stride, pkt_len=pkt_len, n_chunks=n_chunks)
        assert np.array_equal(fl, want_f) and np.array_equal(act, want_a)
        check_records(sums, want_s)


def _datagram(rng, proto, n, v6):
    src, dst = rng.randbytes(16 if v6 else 4), rng.randbytes(16 if v6 else 4)
    pseudo = op.pseudo6(src + dst, n, proto) if v6 else src + dst + struct.pack("!BBH", 0, proto, n)
    field = 16 if proto == 6 else 6
    body = bytearray(rng.randbytes(n))
    if proto == 17:
        body[4:6] = struct.pack("!H", n)
    body[field:field + 2] = b"\0\0"
    ch = netcsum.Chain([{"data": bytes(body), "proto": TCP4}])
    ph = netcsum.HostBytes(pseudo)
    body[field:field + 2] = struct.pack("=H", oracle.data_calc(ch.ptr, ph.ptr, len(pseudo))[0])
    return bytes(body), pseudo, src, dst


def test_reassembled_datagrams_end_to_end():
    rng = random.Random(77)
    frames, owners = [], []                                  # owners[i] = (datagram, piece index) or None
    dgrams = []
    for d in range(24):
        v6, proto = d % 2 == 1, rng.choice([6, 17])
        data, pseudo, src, dst = _datagram(rng, proto, rng.choice([1481, 2960, 2961, 4000, rng.randint(1500, 5800)]), v6)
        if d % 4 >= 2:                                       # half of them: one corrupted bit
            b = bytearray(data)
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            data = bytes(b)
        mtu_pay = rng.choice([1480, 1448, 576 - 24]) & ~7
        pieces = [data[k:k + mtu_pay] for k in range(0, len(data), mtu_pay)]
        dgrams.append((pieces, pseudo))
        ident = rng.getrandbits(16)
        for k, piece in enumerate(pieces):
            mf = k + 1 < len(pieces)
            if v6:
                chain = rng.choice([(), (), ((60, 1),), ((43, 1),)])
                p = v6_fragment(rng, piece, chain, proto, (k * mtu_pay) | (1 if mf else 0), ident, src, dst)
            else:
                p = v4_fragment(rng, piece, rng.choice([5, 5, 7]), (0x2000 if mf else 0) | (k * mtu_pay // 8), proto, ident, src, dst)
            frames.append(p)
            owners.append((d, k))
    for _ in range(len(frames)):                             # other traffic in between
        mk, kinds = (make_packet, KINDS) if rng.random() < 0.5 else (make_packet_v6, KINDS6)
        frames.append(mk(rng, rng.choice(kinds), payload=rng.randint(0, 1300)))
        owners.append(None)
    order = list(range(len(frames)))
    rng.shuffle(order)                                       # fragments arrive in any order, anywhere
    frames, owners = [frames[i] for i in order], [owners[i] for i in order]
    n = len(frames)
    buf, offs, lens = packed_batch(frames, rng, lead=1)
    b = torch.from_numpy(buf).to(DEV)
    act = torch.zeros(n, dtype=torch.uint8, device=DEV)
    sums = torch.zeros(n, dtype=torch.int32, device=DEV)
    netcsum.rx_burst_sums(b, n, act, sums, off=torch.from_numpy(offs.astype(np.int64)).to(DEV),
                          lens=torch.from_numpy(lens.view(np.int16)).to(DEV))
    torch.cuda.synchronize()
    rec = sums.cpu().numpy().view(np.uint16).reshape(n, 2)
    got_act = act.cpu().numpy()
    by_dgram = {}
    for i, o in enumerate(owners):
        if o is not None:
            assert got_act[i] == netcsum.RX_DELIVER_L4_UNVERIFIED
            by_dgram.setdefault(o[0], {})[o[1]] = (int(rec[i, 0]), int(rec[i, 1]))
    verdicts = []
    for d, (pieces, pseudo) in enumerate(dgrams):
        recs = [by_dgram[d][k] for k in range(len(pieces))]              # reassembly order
        assert [r[1] for r in recs] == [len(p) for p in pieces]
        ch = netcsum.Chain([{"data": p, "proto": TCP4, "offset": 2} for p in pieces])
        ph = netcsum.HostBytes(pseudo)
        want, err = oracle.data_verify(ch.ptr, ph.ptr, len(pseudo))
        assert err == netcsum.NET_UTIL_ERR_NONE
        assert netcsum.frag_sum_verify(recs, pseudo) == (want, netcsum.NET_UTIL_ERR_NONE), d
        verdicts.append(want)
    assert verdicts == [1, 1, 0, 0] * 6
