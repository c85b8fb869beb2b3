"""NetUtil_MI355X_RxBurstEtherHost on a pinned receive ring: the resident burst server's Ether form.

A burst of at most 4096 whole Ethernet frames in one pinned allocation, with n_chunks 0 and
TUNE_BURST_ZERO_COPY 3, is served in place: the wave of burst_server_kernel that owns a run classifies
its frames (csrc/netcsum_etherhead.h) and streams their datagrams from descriptors it keeps in registers
(csrc/netcsum_pktstream.hip pkt_ether_run). Every other call takes the copy pipeline. Both give the same
bytes; which one ran is read from last_launch() (a library without the Ether form has no "zero-copy" in
it after any RxBurstEtherHost call, so every `== served(n)` below fails there).

Frames, layouts and expectations are those of test_gpu_ether.py (the mix of ether_frames.py in the
packed / slot / fixed layouts, the last frame ending the allocation); the rings here are pinned host
memory. Burst sizes: 1 (one frame, one wave), 63 / 64 (one frame per wave), 65 (two per wave: the run
length is min(16, ceil(n / 64)) on the server's 64 waves), 257 and 1031 (runs of 5 and 16 + 1), 4096 (16
frames per run, 4 runs per wave), and 4097 (past the server's limit).
"""
import random
import threading
import time

import numpy as np
import pytest

import ether_frames as ef
import netcsum
import oracle_offload as oo
import oracle_packets as op
from packets import make_packet, make_packet_v6
from test_gpu_ether import LAYOUTS, MCAST, burst, call_args, check

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SERVER_BLOCKS = 16                      # csrc/netcsum_host.h kServerBlocks: 16 blocks x 4 waves
SIZES = [1, 63, 64, 65, 257, 1031]
CONFIGS = [(0, ef.HW, 0, True), (MCAST, ef.HW, 0, True), (0, None, 0, True), (MCAST, None, 0, True),
           (0, ef.OTHER, 0, True), (MCAST, ef.HW, netcsum.RXCFG_UDP_DISCARD_NO_CHK_SUM, True), (0, ef.HW, 0, False)]


def served(n):
    return (f"ether_demux b={SERVER_BLOCKS} | burst_server_kernel rx form=ether "
            f"pkts_per_wave={min(16, -(-n // 64))} zero-copy")


def pinned(buf):
    """A pinned copy of buf as a numpy array (the tensor that owns the memory stays its base)."""
    return torch.from_numpy(buf).pin_memory().numpy()


def run_host(b, ring, eth_cfg=MCAST, hw=ef.HW, rx_cfg=0, with_flags=True, n_chunks=0, zero_copy=3):
    """-> (actions, flags or None, classes, last_launch) of one RxBurstEtherHost call on `ring`."""
    act, l2 = np.full(b.n, 0xEE, np.uint8), np.full(b.n, 0xEE, np.uint8)
    fl = np.full(b.n, 0xEE, np.uint8) if with_flags else None
    netcsum.tune(netcsum.TUNE_BURST_ZERO_COPY, zero_copy)
    try:
        netcsum.rx_burst_ether_host(ring[b.lead:], b.n, act, l2, flags=fl, rx_cfg=rx_cfg, eth_cfg=eth_cfg, hw_addr=hw,
                                    n_chunks=n_chunks, **call_args(b, lambda a: a))
        launch = netcsum.last_launch()
    finally:
        netcsum.tune(netcsum.TUNE_BURST_ZERO_COPY, 3)
    return act, fl, l2, launch


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def written(got):
    """No result byte is the caller's 0xEE fill or the server's 0xFF sentinel."""
    return all(x is None or not np.isin(x, (0xEE, 0xFF)).any() for x in got[:3])


@pytest.mark.parametrize("layout,n", [(la, n) for la in LAYOUTS for n in SIZES] + [("packed1", 4096), ("slot1520", 4096)])
def test_served_in_place_and_equal_to_the_copy_pipeline(layout, n):
    b = burst(layout, n)
    ring = pinned(b.buf)
    got = run_host(b, ring)
    assert got[3] == served(n), got[3]
    check(b, got)
    assert written(got)
    copy = run_host(b, ring, zero_copy=0)
    assert "zero-copy" not in copy[3] and copy[3].startswith("ether_demux b="), copy[3]
    assert same(got, copy)
    assert np.array_equal(ring, b.buf)                                   # the ring is only read


@pytest.mark.parametrize("case", ["n4097", "pageable", "chunks3", "zc0", "zc1", "zc2"])
def test_every_other_call_takes_the_copy_pipeline(case):
    b = burst("slot1520", 4097 if case == "n4097" else 257)
    ring = b.buf.copy() if case == "pageable" else pinned(b.buf)
    got = run_host(b, ring, n_chunks=3 if case == "chunks3" else 0, zero_copy=int(case[2]) if case.startswith("zc") else 3)
    assert "zero-copy" not in got[3] and got[3].startswith("ether_demux b="), got[3]
    check(b, got)
    assert written(got)
    if b.n <= 4096:
        ref = run_host(b, pinned(b.buf))
        assert ref[3] == served(b.n) and same(got, ref)


@pytest.mark.parametrize("eth_cfg,hw,rx_cfg,with_flags", CONFIGS)
def test_configurations(eth_cfg, hw, rx_cfg, with_flags):
    for layout in ("packed1", "slot1520"):
        b = burst(layout, 257)
        got = run_host(b, pinned(b.buf), eth_cfg, hw, rx_cfg, with_flags)
        assert got[3] == served(257), got[3]
        check(b, got, eth_cfg, hw, rx_cfg)
        assert written(got)
        if rx_cfg:
            assert (got[0] == netcsum.RX_DROP_UDP_NO_CHK_SUM).any()


def _shuffled(seed, n):
    """n frames of the mix in an order of their own: (frames, received lengths)."""
    rng = random.Random(seed)
    mix = [f for _, f in ef.frame_mix(random.Random(11))]
    rng.shuffle(mix)
    frames = [mix[i % len(mix)] for i in range(n)]
    rng.shuffle(frames)
    return frames, np.array([len(f) for f in frames], np.uint16)


def _write_slots(ring, frames, stride=1520):
    for i, f in enumerate(frames):
        ring[i * stride:i * stride + len(f)] = np.frombuffer(f, np.uint8)


def _expect_ok(frames, act, fl, l2, eth_cfg=MCAST, hw=ef.HW):
    want_l2, _, want_fl, want_act = ef.expect(frames, eth_cfg, hw, 0)
    return np.array_equal(l2, want_l2) and np.array_equal(act, want_act) and (fl is None or np.array_equal(fl, want_fl))


def _slot_call(ring, frames, lens, hw=ef.HW, eth_cfg=MCAST):
    n = len(frames)
    act, fl, l2 = (np.full(n, 0xEE, np.uint8) for _ in range(3))
    netcsum.rx_burst_ether_host(ring, n, act, l2, flags=fl, eth_cfg=eth_cfg, hw_addr=hw, stride=1520, lens=lens.view(np.int16))
    return act, fl, l2


def test_ring_rewritten_in_place_between_bursts():
    """Two orders of the mix written alternately into one pinned ring: each burst sees its own frames and
    lengths (nothing of the previous burst's heads or staged lengths is read from a cache)."""
    n = 257
    ring = pinned(np.zeros(n * 1520, np.uint8))
    orders = [_shuffled(21, n), _shuffled(22, n)]
    assert any(a != b for a, b in zip(orders[0][0], orders[1][0]))
    for k in range(6):
        frames, lens = orders[k % 2]
        _write_slots(ring, frames)
        act, fl, l2 = _slot_call(ring, frames, lens)
        assert netcsum.last_launch() == served(n)
        assert _expect_ok(frames, act, fl, l2), k


def test_post_fields_of_one_burst_do_not_leak_into_the_next():
    """On one thread, one server: an Ether burst with an address and multicast, a strided Rx burst, a Tx
    burst, an Ether burst without address or multicast, an offset/length Rx burst."""
    b = burst("slot1520", 65)
    ring = pinned(b.buf)
    got = run_host(b, ring, MCAST, ef.HW)
    assert got[3] == served(65)
    check(b, got, MCAST, ef.HW)

    m, stride, lead = 64, 1520, 14                                       # the ring's 64 whole slots, datagrams at +14
    want = [ef.ip_verdict(bytes(ring[i * stride + lead:(i + 1) * stride])) for i in range(m)]
    want_fl, want_act = (np.array(x, np.uint8) for x in zip(*want))
    act, fl = np.full(m, 0xEE, np.uint8), np.full(m, 0xEE, np.uint8)
    netcsum.rx_burst_host(ring[lead:], m, act, flags=fl, stride=stride, pkt_len=stride - lead)
    assert netcsum.last_launch().startswith("burst_server_kernel rx form=")
    assert np.array_equal(act, want_act) and np.array_equal(fl, want_fl)

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
    tx_ring = pinned(tx)
    netcsum.tx_burst_host(tx_ring[lead:], k, None, stride=stride, pkt_len=stride - lead)
    assert netcsum.last_launch().startswith("burst_server_kernel tx")
    assert np.array_equal(tx_ring, tx_want)

    got = run_host(b, ring, 0, None)
    assert got[3] == served(65)
    check(b, got, 0, None)

    act, fl = np.full(m, 0xEE, np.uint8), np.full(m, 0xEE, np.uint8)
    netcsum.rx_burst_host(ring, m, act, flags=fl, off=np.arange(m, dtype=np.int64) * stride + lead,
                          lens=np.full(m, stride - lead, np.uint16).view(np.int16))
    assert netcsum.last_launch().startswith("burst_server_kernel rx form=offlen")
    assert np.array_equal(act, want_act) and np.array_equal(fl, want_fl)


@pytest.mark.parametrize("order", ["reversed", "duplicates"])
def test_unordered_and_overlapping_descriptors(order):
    """Runs whose descriptors are not in address order, or overlap, are done one datagram at a time."""
    b = burst("packed2", 65)
    idx = list(range(64, -1, -1)) if order == "reversed" else [j for i in range(65) for j in ([i, i] if i % 3 == 0 else [i])]
    n = len(idx)
    frames = [b.present[j] for j in idx]
    act, fl, l2 = (np.full(n, 0xEE, np.uint8) for _ in range(3))
    netcsum.rx_burst_ether_host(pinned(b.buf), n, act, l2, flags=fl, eth_cfg=MCAST, hw_addr=ef.HW,
                                off=b.off[idx].astype(np.int64), lens=b.lens[idx].view(np.int16))
    assert netcsum.last_launch() == served(n)
    assert _expect_ok(frames, act, fl, l2)


@pytest.mark.parametrize("key,value", [(netcsum.TUNE_BURST_SERVER_LIFE_US, 1), (netcsum.TUNE_BURST_SERVER_IDLE_US, 50)])
def test_server_life_cycle(key, value):
    """200 bursts of 64 frames with a server that is relaunched about every burst (1 us of life), and with
    one that idles out (50 us) in a 1-ms pause every 20 bursts. Only the test as a whole is bounded."""
    n = 64
    frames, lens = _shuffled(31, n)
    ring = pinned(np.zeros(n * 1520, np.uint8))
    _write_slots(ring, frames)
    t0 = time.perf_counter()
    netcsum.tune(key, value)
    try:
        for k in range(200):
            act, fl, l2 = _slot_call(ring, frames, lens)
            assert netcsum.last_launch() == served(n)
            assert _expect_ok(frames, act, fl, l2), k
            if key == netcsum.TUNE_BURST_SERVER_IDLE_US and k % 20 == 19:
                time.sleep(0.001)
    finally:
        netcsum.tune(netcsum.TUNE_BURST_SERVER_LIFE_US, 1000)
        netcsum.tune(netcsum.TUNE_BURST_SERVER_IDLE_US, 500)
    assert time.perf_counter() - t0 < 60.0


def test_two_threads_each_with_its_own_ring_and_address():
    errs = []

    def worker(seed, hw):
        try:
            torch.cuda.set_device(0)
            n = 65
            frames, lens = _shuffled(seed, n)
            ring = pinned(np.zeros(n * 1520, np.uint8))
            _write_slots(ring, frames)
            for k in range(100):
                act, fl, l2 = _slot_call(ring, frames, lens, hw=hw)
                if netcsum.last_launch() != served(n) or not _expect_ok(frames, act, fl, l2, hw=hw):
                    errs.append((seed, k, netcsum.last_launch()))
                    break
        except Exception as e:                                        # noqa: BLE001
            errs.append(repr(e))
        finally:
            netcsum.thread_release()

    th = [threading.Thread(target=worker, args=a) for a in ((41, ef.HW), (42, ef.OTHER))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
