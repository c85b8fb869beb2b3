"""Fragment payload sums from pinned rings through the resident burst server: NetUtil_MI355X_
RxBurstEtherSumsHost and RxBurstSumsHost served in place (include/netcsum_mi355x.h (2b'''), (2b'''')).

A thread's first sums burst stops its server and relaunches it as the SUMS instantiation
(csrc/netcsum_pktstream.hip burst_server_kernel<true>), which from then on serves the thread's bursts of
every kind; the records arrive in coherent pinned memory behind a 0xFFFFFFFF sentinel. Which path ran is
read from last_launch(): "…burst_server_kernel rx,sums form=… zero-copy". Frames and expectations are
those of tests/ether_frag_frames.py; the copy pipeline (TUNE_BURST_ZERO_COPY 0) gives the same bytes.
"""
import random
import threading
import time

import numpy as np
import pytest

import ether_frag_frames as eff
import ether_frames as ef
import netcsum
import oracle
import oracle_offload as oo
import oracle_packets as op
from packets import KINDS, KINDS6, make_packet, make_packet_v6
from test_gpu_ether import call_args
from test_gpu_ether_server import pinned
from test_gpu_ether_server import served as served_plain
from test_gpu_ether_sums import FILL, check, run_host
from test_gpu_fragsum import TCP4, _datagram, v4_fragment, v6_fragment

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
MCAST = netcsum.ETHCFG_MCAST_RX
SENTINEL = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def _release_the_threads_server_afterwards():
    """These tests turn the main thread's server into the SUMS instantiation for good; the thread's context
    is released at the end, so the modules that follow start their server as they did before."""
    yield
    netcsum.thread_release()


def served(n):
    return (f"ether_demux b=16 | burst_server_kernel rx,sums form=ether "
            f"pkts_per_wave={min(16, -(-n // 64))} zero-copy")


def written(got):
    """No result is the caller's fill or the server's sentinel."""
    return (not any(np.isin(x, (0xEE, 0xFF)).any() for x in got[:3])) and not np.isin(got[3], (FILL, SENTINEL)).any()


@pytest.mark.parametrize("layout,n", [(la, n) for la in ("packed1", "slot1520") for n in (1, 63, 64, 65, 257, 1031)]
                         + [("slot1520", 4096)])
def test_served_in_place_and_equal_to_the_copy_pipeline(layout, n):
    b = eff.burst(layout, n)
    ring = pinned(b.buf)
    got = run_host(b, ring)
    assert got[4] == served(n) and "zero-copy" in got[4] and "sums" in got[4], got[4]
    check(b, layout, got)
    assert written(got)
    copy = run_host(b, ring, zero_copy=0)
    assert "zero-copy" not in copy[4] and copy[4].startswith("ether_demux b=") and ",sums" in copy[4], copy[4]
    for k in range(4):
        assert np.array_equal(got[k], copy[k]), k
    assert np.array_equal(ring, b.buf)                                   # the ring is only read


def _ip_level(b, form):
    """The IP datagrams of slot-layout burst b as an IP-level burst: (call kwargs, datagrams as present)."""
    lead = 14
    if form == "strided":
        kw = dict(stride=b.stride, pkt_len=b.stride - lead)
        present = [bytes(b.buf[i * b.stride + lead:(i + 1) * b.stride]) for i in range(b.n - 1)]
        return lead, b.n - 1, kw, present                                # (the last slot ends with its frame)
    lens = np.array([max(len(f) - lead, 0) for f in b.present], np.uint16)
    kw = dict(off=np.arange(b.n, dtype=np.int64) * b.stride + lead, lens=lens.view(np.int16))
    return 0, b.n, kw, [f[lead:] for f in b.present]


def _ip_want(present):
    none = (netcsum.PKT_MALFORMED, netcsum.RX_DELIVER)                   # (a slot with no octets present)
    fl, act = (np.array(x, np.uint8) for x in zip(*(ef.ip_verdict(d) if d else none for d in present)))
    return fl, act, np.array([eff._record(d) for d in present], np.uint32)


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("form", ["strided", "offlen"])
def test_rx_burst_sums_host_is_served_in_place(form, n):
    b = eff.burst("slot1520", n + 1 if form == "strided" else n)
    ring = pinned(b.buf)
    lead, m, kw, present = _ip_level(b, form)
    want_fl, want_act, want_rec = _ip_want(present)
    assert (want_rec != 0).sum() >= m // 8                               # (the fragments behind Ethernet II)
    out = []
    for zc in (3, 0):
        act, fl, rec = np.full(m, 0xEE, np.uint8), np.full(m, 0xEE, np.uint8), np.full(m, FILL, np.uint32)
        netcsum.tune(netcsum.TUNE_BURST_ZERO_COPY, zc)
        try:
            netcsum.rx_burst_sums_host(ring[lead:], m, act, rec, flags=fl, **kw)
            launch = netcsum.last_launch()
        finally:
            netcsum.tune(netcsum.TUNE_BURST_ZERO_COPY, 3)
        if zc == 3:
            assert launch.startswith("burst_server_kernel rx") and "sums" in launch and "zero-copy" in launch, launch
        else:
            assert "zero-copy" not in launch and "sums" in launch, launch
        assert np.array_equal(fl, want_fl) and np.array_equal(act, want_act)
        assert np.array_equal(rec, want_rec), np.nonzero(rec != want_rec)[0][:8]
        out.append((act, fl, rec))
    assert all(np.array_equal(x, y) for x, y in zip(*out))
    assert np.array_equal(ring, b.buf)


def _ether_plain(b, ring, eth_cfg=MCAST, hw=ef.HW):
    act, fl, l2 = (np.full(b.n, 0xEE, np.uint8) for _ in range(3))
    netcsum.rx_burst_ether_host(ring[b.lead:], b.n, act, l2, flags=fl, eth_cfg=eth_cfg, hw_addr=hw, **call_args(b, lambda a: a))
    return act, fl, l2, netcsum.last_launch()


def test_mixed_sequence_on_one_thread():
    """Ether, Ether with sums, IP-level Rx, Tx, Ether with sums without address or multicast, Ether — three
    times round on one thread. Every result is right, and after the first sums burst every burst is still
    served in place (the SUMS server takes the other kinds too)."""
    b = eff.burst("slot1520", 65)
    ring = pinned(b.buf)
    stride, lead, m = 1520, 14, 64
    ip_present = [bytes(ring[i * stride + lead:(i + 1) * stride]) for i in range(m)]
    ip_fl, ip_act, _ = _ip_want(ip_present)
    rng = random.Random(5)
    k = 16
    tx = np.frombuffer(rng.randbytes(k * stride), np.uint8).copy()
    tx_want = tx.copy()
    for i in range(k):
        pkt = (make_packet(rng, rng.choice(["tcp", "udp"]), payload=rng.randint(0, 1400)) if i % 2 else
               make_packet_v6(rng, rng.choice(["tcp", "udp"]), payload=rng.randint(0, 1400)))
        o = i * stride + lead
        tx[o:o + len(pkt)] = np.frombuffer(oo.tx_stack_offload(pkt, True), np.uint8)
        tx_want[o:o + len(pkt)] = np.frombuffer(op.tx_finalize_ip(pkt, True)[0], np.uint8)
    want = {cfg: eff.expect("slot1520", 65, *cfg) for cfg in ((MCAST, ef.HW), (0, None))}

    def plain(cfg):
        act, fl, l2, launch = _ether_plain(b, ring, *cfg)
        assert launch == served_plain(65), launch
        w = want[cfg]
        assert np.array_equal(l2, w[0]) and np.array_equal(fl, w[2]) and np.array_equal(act, w[3])

    def with_sums(cfg):
        got = run_host(b, ring, eth_cfg=cfg[0], hw=cfg[1])
        assert got[4] == served(65), got[4]
        check(b, "slot1520", got, *cfg)
        assert written(got)

    for _ in range(3):
        plain((MCAST, ef.HW))
        with_sums((MCAST, ef.HW))
        act, fl = np.full(m, 0xEE, np.uint8), np.full(m, 0xEE, np.uint8)
        netcsum.rx_burst_host(ring[lead:], m, act, flags=fl, stride=stride, pkt_len=stride - lead)
        assert netcsum.last_launch().startswith("burst_server_kernel rx form=") and "zero-copy" in netcsum.last_launch()
        assert np.array_equal(act, ip_act) and np.array_equal(fl, ip_fl)
        tx_ring = pinned(tx)
        netcsum.tx_burst_host(tx_ring[lead:], k, None, stride=stride, pkt_len=stride - lead)
        assert netcsum.last_launch().startswith("burst_server_kernel tx") and "zero-copy" in netcsum.last_launch()
        assert np.array_equal(tx_ring, tx_want)
        with_sums((0, None))
        plain((MCAST, ef.HW))
    assert np.array_equal(ring, b.buf)


def _shuffled(seed, n):
    rng = random.Random(seed)
    ess, frags, others = eff.pools()
    pool = [f for _, f in list(ess) + list(frags) + list(others)]
    rng.shuffle(pool)
    frames = [pool[i % len(pool)] for i in range(n)]
    return frames, np.array([len(f) for f in frames], np.uint16)


def _write_slots(ring, frames, stride=1520):
    for i, f in enumerate(frames):
        ring[i * stride:i * stride + len(f)] = np.frombuffer(f, np.uint8)


def _slot_call(ring, frames, lens, hw=ef.HW, sums=True):
    n = len(frames)
    act, fl, l2 = (np.full(n, 0xEE, np.uint8) for _ in range(3))
    rec = np.full(n, FILL, np.uint32)
    if sums:
        netcsum.rx_burst_ether_sums_host(ring, n, act, l2, rec, flags=fl, eth_cfg=MCAST, hw_addr=hw, stride=1520,
                                         lens=lens.view(np.int16))
    else:
        netcsum.rx_burst_ether_host(ring, n, act, l2, flags=fl, eth_cfg=MCAST, hw_addr=hw, stride=1520, lens=lens.view(np.int16))
    return act, fl, l2, rec


def _ok(want, got, sums=True):
    return (np.array_equal(got[2], want[0]) and np.array_equal(got[1], want[2]) and np.array_equal(got[0], want[3])
            and (not sums or np.array_equal(got[3], want[4])))


def test_ring_rewritten_in_place_between_bursts():
    """Two orders of the mix written alternately into one pinned ring: the records follow the frames —
    nothing stale from a cache, nothing of the staged sentinel."""
    n = 257
    ring = pinned(np.zeros(n * 1520, np.uint8))
    orders = [_shuffled(21, n), _shuffled(22, n)]
    wants = [eff.expect_frames(fr, MCAST) for fr, _ in orders]
    assert not np.array_equal(wants[0][4], wants[1][4]) and all((w[4] != 0).sum() >= n // 4 for w in wants)
    for k in range(6):
        frames, lens = orders[k % 2]
        _write_slots(ring, frames)
        got = _slot_call(ring, frames, lens)
        assert netcsum.last_launch() == served(n)
        assert _ok(wants[k % 2], got), k
        assert not np.isin(got[3], (FILL, SENTINEL)).any()


@pytest.mark.parametrize("order", ["reversed", "duplicates"])
def test_unordered_and_overlapping_descriptors(order):
    """Runs whose descriptors are not in address order, or overlap: one datagram per run, records included."""
    b = eff.burst("packed1", 65)
    idx = list(range(64, -1, -1)) if order == "reversed" else [j for i in range(65) for j in ([i, i] if i % 3 == 0 else [i])]
    n = len(idx)
    act, fl, l2 = (np.full(n, 0xEE, np.uint8) for _ in range(3))
    rec = np.full(n, FILL, np.uint32)
    netcsum.rx_burst_ether_sums_host(pinned(b.buf), n, act, l2, rec, flags=fl, eth_cfg=MCAST, hw_addr=ef.HW,
                                     off=b.off[idx].astype(np.int64), lens=b.lens[idx].view(np.int16))
    assert netcsum.last_launch() == served(n)
    want = eff.expect("packed1", 65, MCAST)
    assert _ok([w[idx] for w in want], (act, fl, l2, rec))
    assert (rec != 0).sum() >= n // 4


def test_server_life_cycle():
    """50 sums bursts of 64 frames with a server that is relaunched about every burst (1 us of life). Only
    the test as a whole is bounded."""
    n = 64
    frames, lens = _shuffled(31, n)
    want = eff.expect_frames(frames, MCAST)
    ring = pinned(np.zeros(n * 1520, np.uint8))
    _write_slots(ring, frames)
    t0 = time.perf_counter()
    netcsum.tune(netcsum.TUNE_BURST_SERVER_LIFE_US, 1)
    try:
        for k in range(50):
            got = _slot_call(ring, frames, lens)
            assert netcsum.last_launch() == served(n)
            assert _ok(want, got), k
    finally:
        netcsum.tune(netcsum.TUNE_BURST_SERVER_LIFE_US, 1000)
        netcsum.tune(netcsum.TUNE_BURST_SERVER_IDLE_US, 500)
    assert time.perf_counter() - t0 < 60.0


def test_two_threads_one_with_sums_and_one_without():
    errs = []

    def worker(seed, sums):
        try:
            torch.cuda.set_device(0)
            n = 65
            frames, lens = _shuffled(seed, n)
            want = eff.expect_frames(frames, MCAST)
            ring = pinned(np.zeros(n * 1520, np.uint8))
            _write_slots(ring, frames)
            name = served(n) if sums else served_plain(n)
            for k in range(50):
                got = _slot_call(ring, frames, lens, sums=sums)
                if netcsum.last_launch() != name or not _ok(want, got, sums):
                    errs.append((seed, k, netcsum.last_launch()))
                    break
        except Exception as e:                                        # noqa: BLE001
            errs.append(repr(e))
        finally:
            netcsum.thread_release()

    th = [threading.Thread(target=worker, args=a) for a in ((41, True), (42, False))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs


def test_reassembled_datagrams_end_to_end():
    """test_gpu_fragsum's datagrams — half with one corrupted bit, fragments shuffled among other traffic —
    each fragment framed alternately as Ethernet II and SNAP, the bursts served from a pinned ring:
    FragSumVerify over the returned records equals the oracle's DataVerify of the reassembled chain."""
    rng = random.Random(77)
    frames, owners, dgrams = [], [], []
    for d in range(24):
        v6, proto = d % 2 == 1, rng.choice([6, 17])
        data, pseudo, src, dst = _datagram(rng, proto, rng.choice([1481, 2960, 2961, 4000, rng.randint(1500, 5800)]), v6)
        if d % 4 >= 2:
            x = bytearray(data)
            x[rng.randrange(len(x))] ^= 1 << rng.randrange(8)
            data = bytes(x)
        mtu_pay = rng.choice([1424, 1400, 576 - 24]) & ~7                 # (room for LLC/SNAP and the FCS)
        pieces = [data[k:k + mtu_pay] for k in range(0, len(data), mtu_pay)]
        dgrams.append((pieces, pseudo))
        ident = rng.getrandbits(16)
        for k, piece in enumerate(pieces):
            mf = k + 1 < len(pieces)
            if v6:
                p = v6_fragment(rng, piece, rng.choice([(), (), ((60, 1),), ((43, 1),)]), proto, (k * mtu_pay) | (1 if mf else 0),
                                ident, src, dst)
            else:
                p = v4_fragment(rng, piece, rng.choice([5, 5, 7]), (0x2000 if mf else 0) | (k * mtu_pay // 8), proto, ident, src, dst)
            frames.append((eff.frame_snap if len(frames) % 2 else eff.frame_e2)(rng, p))
            owners.append((d, k))
    n_frag = len(frames)
    while len(frames) < 2 * n_frag:                                      # other traffic in between
        mk, kinds = (make_packet, KINDS) if rng.random() < 0.5 else (make_packet_v6, KINDS6)
        p = mk(rng, rng.choice(kinds), payload=rng.randint(0, 1300))
        if len(p) <= 1500:                                               # (the long-chain kinds may exceed a frame)
            frames.append(eff.frame_e2(rng, p))
            owners.append(None)
    order = list(range(len(frames)))
    rng.shuffle(order)
    frames, owners = [frames[i] for i in order], [owners[i] for i in order]
    assert max(len(f) for f in frames) <= 1514
    by_dgram = {}
    per = 64                                                             # the ring: 64 slots, burst after burst
    ring = pinned(np.zeros(per * 1520, np.uint8))
    for s0 in range(0, len(frames), per):
        part = frames[s0:s0 + per]
        lens = np.array([len(f) for f in part], np.uint16)
        _write_slots(ring, part)
        act, fl, l2, rec = _slot_call(ring, part, lens)
        assert netcsum.last_launch() == served(len(part))
        for i, o in enumerate(owners[s0:s0 + per]):
            if o is not None:
                assert act[i] == netcsum.RX_DELIVER_L4_UNVERIFIED and l2[i] in ef.IP_CLASSES
                by_dgram.setdefault(o[0], {})[o[1]] = (int(rec[i]) & 0xFFFF, int(rec[i]) >> 16)
    verdicts = []
    for d, (pieces, pseudo) in enumerate(dgrams):
        recs = [by_dgram[d][k] for k in range(len(pieces))]
        assert [r[1] for r in recs] == [len(p) for p in pieces]
        ch = netcsum.Chain([{"data": p, "proto": TCP4, "offset": 2} for p in pieces])
        ph = netcsum.HostBytes(pseudo)
        want, err = oracle.data_verify(ch.ptr, ph.ptr, len(pseudo))
        assert err == netcsum.NET_UTIL_ERR_NONE
        assert netcsum.frag_sum_verify(recs, pseudo) == (want, netcsum.NET_UTIL_ERR_NONE), d
        verdicts.append(want)
    assert verdicts == [1, 1, 0, 0] * 6
