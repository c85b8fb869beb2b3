"""GPU parity of NetUtil_MI355X_RxBurstEtherSums and the copy pipeline of RxBurstEtherSumsHost
(include/netcsum_mi355x.h (2b'''')): RxBurstEther with the fragment payload sums of (2b''').

Bursts of 1, 63, 64, 65 and 257 frames of the mix of tests/ether_frag_frames.py (fragments behind both
layer-2 headers, padded with non-zero octets, behind long IPv6 chains; every non-IP class; type / version
mismatches that carry fragments) in the packed (odd starts), 1520-B slot and fixed-length layouts, the last
frame ending the allocation. Checked: actions, flags and classes equal rx_burst_ether's on the same burst
and the Python rules; the records equal the expectation (the oracle's DataCalc over the fragment's payload,
found through the Python 802.x rules) and rx_burst_sums run directly on the datagrams' own descriptors;
last_launch(); three configurations; the host form from pageable rings, in chunks, and past the server's
limit; a burst captured into a HIP graph.
"""
import numpy as np
import pytest

import ether_frag_frames as eff
import ether_frames as ef
import netcsum
from test_gpu_ether import call_args

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
MCAST = netcsum.ETHCFG_MCAST_RX
SIZES = [1, 63, 64, 65, 257]
FILL = 0x5A5A5A5A


def check_equal(b, what, got, want, fmt=int):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, [(int(i), b.names[i], fmt(int(got[i])), fmt(int(want[i]))) for i in bad[:8]])


def check(b, layout, got, eth_cfg=MCAST, hw=ef.HW, rx_cfg=0):
    """got = (actions, flags, classes, records) against the Python rules and the oracle."""
    want_l2, hdr, want_fl, want_act, want_rec = eff.expect(layout, b.n, eth_cfg, hw, rx_cfg)
    check_equal(b, "class", got[2], want_l2)
    check_equal(b, "action", got[0], want_act)
    if got[1] is not None:
        check_equal(b, "flags", got[1], want_fl, hex)
    check_equal(b, "record", got[3], want_rec, hex)
    assert not (got[3][hdr == 0]).any()                                  # no datagram to check: {0, 0}
    return hdr, want_rec


def run_device(b, sums=True, eth_cfg=MCAST, hw=ef.HW, rx_cfg=0, stream=None, keep=None):
    t = torch.from_numpy(b.buf).to(DEV)
    to = lambda a: torch.from_numpy(a).to(DEV)
    act, fl, l2 = (torch.full((b.n,), 0xEE, dtype=torch.uint8, device=DEV) for _ in range(3))
    rec = torch.full((b.n,), FILL, dtype=torch.int32, device=DEV)
    kw = dict(flags=fl, rx_cfg=rx_cfg, eth_cfg=eth_cfg, hw_addr=hw, **call_args(b, to))
    if sums:
        netcsum.rx_burst_ether_sums(t[b.lead:], b.n, act, l2, rec, **kw)
    else:
        netcsum.rx_burst_ether(t[b.lead:], b.n, act, l2, **kw)
    launch = netcsum.last_launch()
    torch.cuda.synchronize()
    return act.cpu().numpy(), fl.cpu().numpy(), l2.cpu().numpy(), rec.cpu().numpy().view(np.uint32), launch, t


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", eff.LAYOUTS)
def test_rx_burst_ether_sums_layouts(layout, n):
    b = eff.burst(layout, n)
    got = run_device(b)
    assert got[4].startswith(f"ether_demux b={(n + 255) // 256} | pkt_") and ",sums" in got[4], got[4]
    plain = run_device(b, sums=False)
    assert ",sums" not in plain[4]
    for k in range(3):                                                   # byte for byte rx_burst_ether's
        assert np.array_equal(got[k], plain[k]), k
    assert (plain[3] == FILL).all()
    hdr, want_rec = check(b, layout, got)
    # the datagrams' own descriptors through rx_burst_sums: the same records
    ip = np.nonzero(hdr)[0]
    if ip.size:
        off = np.array([b.start[i] + hdr[i] for i in ip], np.int64)
        lens = np.array([len(b.present[i]) - hdr[i] for i in ip], np.uint16)
        act2, fl2 = (torch.full((ip.size,), 0xEE, dtype=torch.uint8, device=DEV) for _ in range(2))
        rec2 = torch.full((ip.size,), FILL, dtype=torch.int32, device=DEV)
        netcsum.rx_burst_sums(got[5][b.lead:], int(ip.size), act2, rec2, flags=fl2, off=torch.from_numpy(off).to(DEV),
                              lens=torch.from_numpy(lens.view(np.int16)).to(DEV))
        torch.cuda.synchronize()
        assert np.array_equal(got[3][ip], rec2.cpu().numpy().view(np.uint32))
        assert np.array_equal(got[0][ip], act2.cpu().numpy()) and np.array_equal(got[1][ip], fl2.cpu().numpy())
    if n >= 63:
        assert (want_rec != 0).sum() >= n // 4
    # the mismatch frames: RxBurstSums at frame + 14 would report a sum, this call must not
    for i, nm in enumerate(b.names):
        if nm.startswith("mismatch"):
            assert got[3][i] == 0 and got[1][i] == netcsum.PKT_MALFORMED and got[0][i] == netcsum.RX_DELIVER, nm


@pytest.mark.parametrize("eth_cfg,hw,rx_cfg", [(0, None, 0), (MCAST, ef.OTHER, 0),
                                               (MCAST, ef.HW, netcsum.RXCFG_UDP_DISCARD_NO_CHK_SUM)])
def test_rx_burst_ether_sums_configurations(eth_cfg, hw, rx_cfg):
    for layout in ("packed1", "slot1520"):
        b = eff.burst(layout, 257)
        got = run_device(b, True, eth_cfg, hw, rx_cfg)
        check(b, layout, got, eth_cfg, hw, rx_cfg)
        # a fragment whose destination the interface rejects has no record; promiscuous, it has one
        other = [i for i, nm in enumerate(b.names) if nm.startswith("other station")]
        assert other
        for i in other:
            if hw is None or hw == ef.OTHER:
                assert got[2][i] == ef.ETHER_IPV4 and got[3][i] >> 16 == 100
            else:
                assert got[2][i] == ef.INV_ADDR_DEST and got[3][i] == 0
        if hw == ef.OTHER:                                               # every unicast frame of the mix is for HW
            dest = got[2] == ef.INV_ADDR_DEST
            assert dest.sum() > b.n // 2 and not got[3][dest].any()
        if rx_cfg:
            assert (got[0] == netcsum.RX_DROP_UDP_NO_CHK_SUM).any()


def run_host(b, ring, n_chunks=0, zero_copy=3, eth_cfg=MCAST, hw=ef.HW):
    act, fl, l2 = (np.full(b.n, 0xEE, np.uint8) for _ in range(3))
    rec = np.full(b.n, FILL, np.uint32)
    netcsum.tune(netcsum.TUNE_BURST_ZERO_COPY, zero_copy)
    try:
        netcsum.rx_burst_ether_sums_host(ring[b.lead:], b.n, act, l2, rec, flags=fl, eth_cfg=eth_cfg, hw_addr=hw,
                                         n_chunks=n_chunks, **call_args(b, lambda a: a))
        launch = netcsum.last_launch()
    finally:
        netcsum.tune(netcsum.TUNE_BURST_ZERO_COPY, 3)
    return act, fl, l2, rec, launch


@pytest.mark.parametrize("layout,n_chunks", [("packed1", 0), ("packed1", 3), ("slot1520", 0), ("slot1520", 3), ("fixed", 3),
                                             ("packed1", 7), ("slot1520", 7)])
def test_host_form_copy_pipeline_from_a_pageable_ring(layout, n_chunks):
    """257 frames in 3 chunks: a chunk boundary lies inside the records; in 7 chunks (6 of 37 and one of 35)
    every pipeline slot is reused, by a form that stages offsets and lengths and by one that stages lengths."""
    b = eff.burst(layout, 257)
    dev = run_device(b)
    got = run_host(b, b.buf.copy(), n_chunks)
    assert got[4].startswith("ether_demux b=") and ",sums" in got[4] and "zero-copy" not in got[4], got[4]
    for k in range(4):
        assert np.array_equal(got[k], dev[k]), k
    check(b, layout, got)


def test_host_form_past_the_servers_limit_takes_the_copy_pipeline():
    n = 4097
    b = eff.burst("slot1520", n)
    ring = torch.from_numpy(b.buf).pin_memory().numpy()
    got = run_host(b, ring)
    assert got[4].startswith("ether_demux b=") and ",sums" in got[4] and "zero-copy" not in got[4], got[4]
    l2, hdr, fl, act, rec = eff.expect_frames(b.present, MCAST)
    assert np.array_equal(got[0], act) and np.array_equal(got[1], fl) and np.array_equal(got[2], l2)
    assert np.array_equal(got[3], rec)


def test_graph_capture_follows_the_tx_scratch_rule():
    """As RxBurstEther's: after one uncaptured call on the stream the burst is captured into a HIP graph; a
    later uncaptured burst on the stream takes a slot of its own; the graph, replayed afterwards, still
    gives its own burst's results, records included."""
    s = torch.cuda.Stream()
    b1, b2 = eff.burst("slot1520", 257), eff.burst("packed1", 65)
    to = lambda a: torch.from_numpy(a).to(DEV)
    with torch.cuda.stream(s):
        t1, t2 = to(b1.buf), to(b2.buf)
        kw1, kw2 = call_args(b1, to), call_args(b2, to)
        r1 = [torch.full((b1.n,), 0xEE, dtype=torch.uint8, device=DEV) for _ in range(3)]
        r2 = [torch.full((b2.n,), 0xEE, dtype=torch.uint8, device=DEV) for _ in range(3)]
        s1 = torch.full((b1.n,), FILL, dtype=torch.int32, device=DEV)
        s2 = torch.full((b2.n,), FILL, dtype=torch.int32, device=DEV)
        call1 = lambda: netcsum.rx_burst_ether_sums(t1[b1.lead:], b1.n, r1[0], r1[2], s1, flags=r1[1], eth_cfg=MCAST,
                                                    hw_addr=ef.HW, stream=s, **kw1)
        call1()
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call1()
    with torch.cuda.stream(s):
        netcsum.rx_burst_ether_sums(t2[b2.lead:], b2.n, r2[0], r2[2], s2, flags=r2[1], eth_cfg=MCAST, hw_addr=ef.HW,
                                    stream=s, **kw2)
    s.synchronize()
    host = lambda r, sm: (r[0].cpu().numpy(), r[1].cpu().numpy(), r[2].cpu().numpy(), sm.cpu().numpy().view(np.uint32))
    check(b2, "packed1", host(r2, s2))
    for x in r1:
        x.fill_(0xEE)
    s1.fill_(FILL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    check(b1, "slot1520", host(r1, s1))
