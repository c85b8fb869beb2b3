"""CPU-only checks of NetUtil_MI355X_RxBurstEtherSums / RxBurstEtherSumsHost (include/netcsum_mi355x.h
(2b'''')): the condition on the shared frame mix of ether_frag_frames.py, and the argument checks, which
come before any device work (the library loads and answers them without a GPU).
"""
import ctypes

import numpy as np
import pytest

import ether_frag_frames as eff
import ether_frames as ef
import netcsum

E_NULL, E_ARG, OK = netcsum.NET_ERR_FAULT_NULL_PTR, netcsum.NET_UTIL_ERR_MI355X_INVALID_ARG, netcsum.NET_UTIL_ERR_NONE
SIZES = [63, 64, 65, 257, 1031, 4096]


@pytest.mark.parametrize("layout", eff.LAYOUTS)
def test_the_mix_holds_what_the_gpu_tests_rely_on(layout):
    """For every burst of n >= 63 frames: at least n // 4 fragments with a non-zero expected record, one of
    them behind LLC/SNAP, one that takes the extension-header walk, a non-IP frame, and both type / version
    mismatch frames (which carry well-formed fragments and expect {0, 0})."""
    for n in SIZES:
        if layout != "slot1520" and n == 4096:
            continue
        b = eff.burst(layout, n)
        c = eff.mix_counts(b, eth_cfg=netcsum.ETHCFG_MCAST_RX)
        assert c["fragments"] >= n // 4, (n, c)
        assert c["behind_snap"] >= 1 and c["walk"] >= 1 and c["non_ip"] >= 1, (n, c)
        assert c["mismatch"] >= 2 and len(c["mismatch_names"]) == 2, (n, c)
        assert all(len(f) <= eff.MAX_FRAME for f, r in zip(b.present, eff.expect(layout, n, netcsum.ETHCFG_MCAST_RX)[4]) if r)


def test_the_pools_cover_the_listed_cases():
    ess, frags, others = eff.pools()
    l2, hdr, fl, _, rec = eff.expect_frames([f for _, f in frags], netcsum.ETHCFG_MCAST_RX)
    assert (rec != 0).all(), [frags[i][0] for i in np.nonzero(rec == 0)[0]]
    assert {14, 22} <= set(hdr.tolist())
    names = " ".join(nm for nm, _ in frags)
    for ihl in (5, 6, 15):
        for pay in (1, 7, 8, 9):
            assert f"v4 ihl{ihl} pay{pay}" in names
        assert f"v4 ihl{ihl} bad ip csum" in names
    assert "v4 ihl5 pay1479" in names and "v4 ihl5 pay1480" in names
    for chain in eff.V6_CHAINS:
        assert f"v6 chain{chain} " in names
    # a bad IPv4 header checksum keeps its record
    bad = [i for i, (nm, _) in enumerate(frags) if "bad ip csum" in nm]
    assert bad and all(fl[i] & netcsum.PKT_FRAGMENT and not fl[i] & netcsum.PKT_IP_OK and rec[i] >> 16 for i in bad)
    # the padded fragments: 60 octets received, non-zero padding behind the datagram, len from the IP header
    padded = [(nm, f) for nm, f in frags + ess if "pay7" in nm and len(f) == 60]
    assert len(padded) >= 2 and {nm.split()[0] for nm, _ in padded} == {"e2", "snap"}
    for nm, f in padded:
        _, h, d = ef.ip_datagram(f, netcsum.ETHCFG_MCAST_RX)
        tot = int.from_bytes(d[2:4], "big")
        assert tot < len(d) and all(d[tot:]), nm
        assert eff.expect_frames([f], netcsum.ETHCFG_MCAST_RX)[4][0] >> 16 == 7
    # empty and all-zero payloads, every class of the Ethernet mix
    o_l2, _, _, _, o_rec = eff.expect_frames([f for _, f in others], netcsum.ETHCFG_MCAST_RX)
    assert set(range(16)) <= set(o_l2.tolist())
    zero = [i for i, (nm, _) in enumerate(others) if "all-zero" in nm]
    assert len(zero) >= 3 and all(o_rec[i] & 0xFFFF == 0 and o_rec[i] >> 16 for i in zero)
    assert all(o_rec[i] == 0 for i, (nm, _) in enumerate(others) if "pay0" in nm)


def _ptr(a):
    return a.ctypes.data


def test_argument_checks_come_before_device_work():
    L = netcsum.lib()
    buf = np.zeros(4096, np.uint8)
    out = np.zeros(64, np.uint8)
    sums = np.zeros(16, np.uint32)
    b, a, f, l, s = _ptr(buf), _ptr(out), _ptr(out) + 16, _ptr(out) + 32, _ptr(sums)
    for fn, tail in ((L.NetUtil_MI355X_RxBurstEtherSums, None), (L.NetUtil_MI355X_RxBurstEtherSumsHost, 0)):
        call = lambda n=3, rx=0, eth=0, base=b, act=a, l2=l, sm=s: fn(base, None, None, 1024, 1024, n, rx, eth, None, act, f, l2, sm, tail)
        assert call(sm=None) == E_NULL                                   # NULL sums
        assert call(act=None) == E_NULL and call(l2=None) == E_NULL and call(base=None) == E_NULL
        assert call(sm=s + 2) == E_ARG and call(sm=s + 1) == E_ARG       # one record is one 4-B store
        assert call(n=1 << 30) == E_ARG                                  # 2^30 - 1 frames at most
        assert call(rx=2) == E_ARG and call(rx=1 << 31) == E_ARG         # unknown rx_cfg bits
        assert call(eth=2) == E_ARG and call(eth=0x100) == E_ARG         # unknown eth_cfg bits
        assert call(n=0) == OK                                           # nothing to do, no launch
        assert call(n=0, sm=None, act=None, l2=None, base=None) == OK
        assert call(rx=2, sm=None) == E_ARG                              # RxBurstEther's checks first
        assert call(act=None, rx=2) == E_NULL


def test_the_binding_rejects_undersized_buffers():
    n = 8
    ring = np.zeros(n * 1520, np.uint8)
    act, l2, sums = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    for fn in (netcsum.rx_burst_ether_sums, netcsum.rx_burst_ether_sums_host):
        with pytest.raises(ValueError, match="fragment sums"):
            fn(ring, n, act, l2, sums[:n - 1], stride=1520, frame_len=1514)
        with pytest.raises(ValueError, match="actions"):
            fn(ring, n, act[:n - 1], l2, sums, stride=1520, frame_len=1514)
        with pytest.raises(ValueError, match="layer-2 classes"):
            fn(ring, n, act, l2[:n - 1], sums, stride=1520, frame_len=1514)
        with pytest.raises(ValueError, match="frames"):
            fn(ring[:-7], n, act, l2, sums, stride=1520, frame_len=1520)
    assert netcsum.rx_burst_ether_sums_host(ring, 0, act, l2, sums, stride=1520, frame_len=1514) == OK


def test_the_entry_points_are_declared_and_exported():
    names = netcsum.exported_symbols_from_headers()
    for nm in ("NetUtil_MI355X_RxBurstEtherSums", "NetUtil_MI355X_RxBurstEtherSumsHost"):
        assert nm in names and isinstance(getattr(netcsum.lib(), nm), ctypes._CFuncPtr)
