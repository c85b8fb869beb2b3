"""GPU parity of NetUtil_MI355X_TxBurstEther / TxBurstEtherHost (include/netcsum_mi355x.h (2b''''')).

Bursts of 1, 63, 64, 65, 257 and 1031 frames (around the wave, the demux block of 256 and the packet
kernels' runs) of the mix of tests/ether_tx_frames.py — the stack's offload-form datagrams of every kind
behind an Ethernet II header, padded to 60 octets, with ARP, unknown types, 802.3/SNAP frames, a runt, a
60-octet frame, type / version mismatches, UDP with the checksum off, IPv6 chains past the header window
and 1514-octet frames among them — in the layouts a driver's Tx queue has:

  packed  offset/length frames at random leads (every start residue mod 4, 64-B sectors straddled);
  slot0   1520-B slots, frame at +0, per-frame lengths and no offsets;
  slot2   1520-B slots, frame at +2, per-frame lengths and no offsets;
  fixed   2048-B slots of 1514 octets, neither offsets nor lengths.

Checked: the WHOLE ring afterwards (gaps, padding, Ethernet headers, ARP / INV_* frames and a guard tail
keep every byte; the IP frames are the header + the Tx adapter's rule on the datagram), the classes and
the flags against the helpers, with and without a flags array; the ring against tx_burst over host-built
descriptors of the IP frames; both Tx pass settings; the finalized ring through rx_burst_ether; argument
errors, last_launch(), an empty burst under stream capture; the host-memory form's copy pipeline.
"""
import random

import numpy as np
import pytest

import ether_frames as ef
import ether_tx_frames as etx
import netcsum

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 63, 64, 65, 257, 1031]
LAYOUTS = ["packed", "slot0", "slot2", "fixed"]
to_dev = lambda a: torch.from_numpy(a).to(DEV)


def run_device(b, with_flags=True, stream=None):
    t = torch.from_numpy(b.buf).to(DEV)
    l2 = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=DEV)
    fl = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=DEV) if with_flags else None
    netcsum.tx_burst_ether(t[b.lead:], b.n, l2, flags=fl, **etx.call_args(b, to_dev))
    launch = netcsum.last_launch()
    torch.cuda.synchronize()
    return t.cpu().numpy(), l2.cpu().numpy(), fl.cpu().numpy() if with_flags else None, launch


def check(b, ring, l2, fl):
    bad = np.nonzero(l2 != b.want_l2)[0]
    assert bad.size == 0, [(int(i), b.names[i], int(l2[i]), int(b.want_l2[i])) for i in bad[:8]]
    if fl is not None:
        bad = np.nonzero(fl != b.want_fl)[0]
        assert bad.size == 0, [(int(i), b.names[i], hex(int(fl[i])), hex(int(b.want_fl[i]))) for i in bad[:8]]
    bad = np.nonzero(ring != b.want)[0]
    if bad.size:
        starts = np.array(b.start) + b.lead
        k = int(np.searchsorted(starts, bad[0], side="right")) - 1
        raise AssertionError((bad[:8].tolist(), k, b.names[k], int(bad[0] - starts[k])))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_tx_burst_ether_layouts(layout, n):
    b = etx.ring(layout, n)
    ring, l2, fl, launch = run_device(b)
    assert launch.startswith(f"ether_tx_demux b={(n + 255) // 256} | pkt_"), launch
    check(b, ring, l2, fl)
    ring2, l22, _, _ = run_device(b, with_flags=False)
    check(b, ring2, l22, None)
    if n >= 257:                                                         # the burst holds what it should
        assert {ef.ETHER_IPV4, ef.ETHER_IPV6, ef.ETHER_ARP, ef.INV_ETHER_TYPE} <= set(b.want_l2.tolist())
        assert layout == "fixed" or ef.INV_FRAME_SIZE in b.want_l2
        assert (b.want != b.buf).sum() > n                               # ... and the burst had fields to fill
        assert any(nm == "v6 ext_long" for nm in b.names)


@pytest.mark.parametrize("layout", ["packed", "slot2"])
def test_ring_equals_tx_burst_over_host_built_descriptors(layout):
    b = etx.ring(layout, 1031)
    ring, l2, fl, _ = run_device(b)
    ip = [i for i, f in enumerate(b.frames) if etx.datagram(f)[1]]
    off = np.array([b.start[i] + 14 for i in ip], np.int64)
    lens = np.array([len(b.frames[i]) - 14 for i in ip], np.uint16)
    t = torch.from_numpy(b.buf).to(DEV)
    fl2 = torch.full((len(ip),), 0xEE, dtype=torch.uint8, device=DEV)
    netcsum.tx_burst(t[b.lead:], len(ip), flags=fl2, off=to_dev(off), lens=to_dev(lens.view(np.int16)))
    torch.cuda.synchronize()
    assert np.array_equal(ring, t.cpu().numpy())
    assert np.array_equal(fl[ip], fl2.cpu().numpy())


@pytest.mark.parametrize("passes", [1, 2])
def test_tx_pass_tuning(passes):
    netcsum.tune(netcsum.TUNE_TX_PASSES, passes)
    try:
        for layout in ("packed", "slot0"):
            b = etx.ring(layout, 257)
            ring, l2, fl, _ = run_device(b)
            check(b, ring, l2, fl)
    finally:
        netcsum.tune(netcsum.TUNE_TX_PASSES, 0)


def test_loopback_through_rx_burst_ether():
    """The finalized ring, received by a station whose address is the destination used: every class,
    flag and action is what the Rx helpers expect of the expected frames, and none of these kinds (the
    ones on which the Tx and Rx oracles agree) is dropped."""
    b = etx.ring("slot0", 1031, loopback_only=True)
    t = torch.from_numpy(b.buf).to(DEV)
    l2 = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=DEV)
    kw = etx.call_args(b, to_dev)
    netcsum.tx_burst_ether(t[b.lead:], b.n, l2, **kw)
    act, rfl, rl2 = (torch.full((b.n,), 0xEE, dtype=torch.uint8, device=DEV) for _ in range(3))
    netcsum.rx_burst_ether(t[b.lead:], b.n, act, rl2, flags=rfl, eth_cfg=netcsum.ETHCFG_MCAST_RX, hw_addr=etx.DST, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), b.want)
    want_l2, _, want_fl, want_act = ef.expect(b.want_frames, netcsum.ETHCFG_MCAST_RX, etx.DST)
    act, rfl, rl2 = act.cpu().numpy(), rfl.cpu().numpy(), rl2.cpu().numpy()
    assert np.array_equal(rl2, want_l2) and np.array_equal(rfl, want_fl) and np.array_equal(act, want_act)
    assert np.array_equal(rl2, l2.cpu().numpy())                         # both rules name these frames alike
    ok = (act == netcsum.RX_DELIVER) | (act == netcsum.RX_DELIVER_L4_UNVERIFIED)
    assert ok.all(), [(int(i), b.names[i], int(act[i])) for i in np.nonzero(~ok)[0][:8]]
    assert (act == netcsum.RX_DELIVER_L4_UNVERIFIED).any()               # (the fragments)


def test_argument_errors_and_last_launch():
    b = etx.ring("slot0", 65)
    t = torch.from_numpy(b.buf).to(DEV)
    l2 = torch.zeros(b.n, dtype=torch.uint8, device=DEV)
    L = netcsum.lib()
    ln = to_dev(b.lens.view(np.int16))
    assert L.NetUtil_MI355X_TxBurstEther(t.data_ptr(), None, ln.data_ptr(), 1520, 0, b.n, None, None, None) == \
        netcsum.NET_ERR_FAULT_NULL_PTR
    assert L.NetUtil_MI355X_TxBurstEther(None, None, ln.data_ptr(), 1520, 0, b.n, None, l2.data_ptr(), None) == \
        netcsum.NET_ERR_FAULT_NULL_PTR
    assert L.NetUtil_MI355X_TxBurstEther(t.data_ptr(), None, ln.data_ptr(), 1520, 0, 0x80000000, None, l2.data_ptr(), None) == \
        netcsum.NET_UTIL_ERR_MI355X_INVALID_ARG
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), b.buf)                        # nothing ran
    netcsum.tx_burst(t[14:], 1, stride=1520, pkt_len=60)
    before = netcsum.last_launch()
    assert L.NetUtil_MI355X_TxBurstEther(t.data_ptr(), None, None, 1520, 1514, 0, None, None, None) == netcsum.NET_UTIL_ERR_NONE
    assert netcsum.last_launch() == before                               # an empty burst launches nothing
    netcsum.tx_burst_ether(t, b.n, l2, lens=ln, stride=1520)
    s = netcsum.last_launch()
    head, _, rest = s.partition(" | ")
    assert head == "ether_tx_demux b=1" and rest.startswith("pkt_") and "tx" in rest, s
    torch.cuda.synchronize()


def test_empty_burst_under_stream_capture_is_a_no_op():
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(64, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        assert netcsum.tx_burst_ether(x, 0, None, stride=64, frame_len=64, stream=s) == netcsum.NET_UTIL_ERR_NONE
        x.add_(1)
    g.replay()
    torch.cuda.synchronize()
    assert int(x[0]) == 1


@pytest.mark.parametrize("layout,n,n_chunks", [("packed", 1031, 0), ("packed", 1031, 3), ("slot0", 257, 1), ("slot2", 1031, 4),
                                               ("fixed", 65, 0), ("fixed", 257, 5), ("slot0", 1, 0),
                                               ("packed", 29, 7)])       # 6 chunks of 5, 5, 5, 5, 5, 4: slots reused
def test_tx_burst_ether_host_form(layout, n, n_chunks):
    b = etx.ring(layout, n)
    for pinned in (True, False):
        ring = torch.from_numpy(b.buf.copy())
        ring = (ring.pin_memory() if pinned else ring).numpy()
        l2, fl = np.full(b.n, 0xEE, np.uint8), np.full(b.n, 0xEE, np.uint8)
        netcsum.tx_burst_ether_host(ring[b.lead:], b.n, l2, flags=fl, n_chunks=n_chunks, **etx.call_args(b, lambda a: a))
        launch = netcsum.last_launch()
        assert launch.startswith("ether_tx_demux b="), launch
        if n_chunks or not pinned:                                       # (else a pinned ring may be served in place)
            assert " | pkt_" in launch, launch
        check(b, ring, l2, fl)
    ring = torch.from_numpy(b.buf.copy()).pin_memory().numpy()           # no flags array
    l2 = np.full(b.n, 0xEE, np.uint8)
    netcsum.tx_burst_ether_host(ring[b.lead:], b.n, l2, n_chunks=n_chunks, **etx.call_args(b, lambda a: a))
    check(b, ring, l2, None)
    assert netcsum.rx_burst_ether_tally(l2) == [int((b.want_l2 == c).sum()) for c in range(netcsum.L2_NBR_CLASSES)]


def test_host_ring_rewritten_in_place_between_bursts():
    b1, b2 = etx.ring("slot0", 257), etx.ring("slot0", 257, seed=1)
    ring = torch.from_numpy(b1.buf.copy()).pin_memory().numpy()
    for b in (b1, b2, b1):
        ring[:] = b.buf
        l2, fl = np.full(b.n, 0xEE, np.uint8), np.full(b.n, 0xEE, np.uint8)
        netcsum.tx_burst_ether_host(ring, b.n, l2, flags=fl, **etx.call_args(b, lambda a: a))
        check(b, ring, l2, fl)
