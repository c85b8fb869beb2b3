"""NetUtil_MI355X_TxBurstEtherHost from a pinned ring through the resident burst server's Tx Ether form
(include/netcsum_mi355x.h (2e)): in place against the copy pipeline.

Bursts of 1, 63, 64, 65, 257, 1031 and 4096 frames of the mix of tests/ether_tx_frames.py in a pinned ring
of 1520-B slots and a packed one: the in-place result (n_chunks 0: the wave that owns a run classifies its
frames and streams their datagrams into records, the host applies them at frame + 14) equals the copy
pipeline's (n_chunks 1) byte for byte — the whole ring, the classes, the flags — and both equal the
helpers; last_launch() names the server on the first and not on the second. Calls outside the in-place
conditions (4097 frames, a pageable ring, n_chunks 3, BURST_ZERO_COPY 0 / 1 / 2) take the copy pipeline
with the same bytes; IPv6 chains past the header window go to the copy path from the served burst; Rx and
Tx Ether bursts share one server in either order; a ring rewritten in place is served right each time.
"""
import numpy as np
import pytest

import ether_frames as ef
import ether_tx_frames as etx
import netcsum

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257, 1031, 4096]
SERVED = "burst_server_kernel tx form=ether pkts_per_wave="
host = lambda a: a


def pinned(buf):
    return torch.from_numpy(buf.copy()).pin_memory().numpy()


def run_host(b, ring, n_chunks=0, with_flags=True):
    l2 = np.full(b.n, 0xEE, np.uint8)
    fl = np.full(b.n, 0xEE, np.uint8) if with_flags else None
    netcsum.tx_burst_ether_host(ring[b.lead:], b.n, l2, flags=fl, n_chunks=n_chunks, **etx.call_args(b, host))
    return l2, fl, netcsum.last_launch()


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


def has_long_chain(b):
    return any(nm == "v6 ext_long" for nm in b.names)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", ["slot0", "slot2", "packed"])
def test_in_place_equals_the_copy_pipeline(layout, n):
    b = etx.ring(layout, n)
    r0, r1 = pinned(b.buf), pinned(b.buf)
    l2, fl, launch = run_host(b, r0)
    assert launch.startswith("ether_tx_demux b=") and SERVED in launch and "zero-copy" in launch, launch
    assert "+copy path for" in launch or not has_long_chain(b), launch
    l2c, flc, launch_c = run_host(b, r1, n_chunks=1)
    assert launch_c.startswith("ether_tx_demux b=") and "burst_server_kernel" not in launch_c, launch_c
    assert np.array_equal(r0, r1) and np.array_equal(l2, l2c) and np.array_equal(fl, flc)
    check(b, r0, l2, fl)
    r2 = pinned(b.buf)                                                   # no flags array
    l22, _, launch2 = run_host(b, r2, with_flags=False)
    assert SERVED in launch2
    check(b, r2, l22, None)


def test_calls_outside_the_conditions_take_the_copy_pipeline():
    b = etx.ring("slot0", 257)
    big = etx.ring("slot0", 4097)
    cases = [(big, pinned(big.buf), 0, 3), (b, b.buf.copy(), 0, 3), (b, pinned(b.buf), 3, 3)]
    cases += [(b, pinned(b.buf), 0, zc) for zc in (0, 1, 2)]
    for bb, ring, n_chunks, zc in cases:
        netcsum.tune(netcsum.TUNE_BURST_ZERO_COPY, zc)
        try:
            l2, fl, launch = run_host(bb, ring, n_chunks)
        finally:
            netcsum.tune(netcsum.TUNE_BURST_ZERO_COPY, 3)
        assert launch.startswith("ether_tx_demux b=") and "burst_server_kernel" not in launch, (launch, n_chunks, zc)
        check(bb, ring, l2, fl)


def test_long_chains_take_the_mixed_path():
    b = etx.ring("slot0", 257)
    assert has_long_chain(b)
    ring = pinned(b.buf)
    l2, fl, launch = run_host(b, ring)
    # every chain past the header window goes there, and nothing but IPv6 datagrams with extension headers
    # (a short chain that ends past the lane's own window is finished there too)
    k = sum(nm == "v6 ext_long" for nm in b.names)
    k_max = sum(nm.startswith("v6 ext_") for nm in b.names)
    head, _, tail = launch.partition(" zero-copy +copy path for ")
    assert SERVED in head and tail.endswith(" EXT_HDR datagrams"), launch
    assert k <= int(tail.split()[0]) <= k_max, (launch, k, k_max)
    check(b, ring, l2, fl)


@pytest.mark.parametrize("tx_first", [True, False])
def test_rx_and_tx_ether_bursts_share_one_server(tx_first):
    """No field of one burst's post may leak into the next: the Rx burst has an interface address, a
    multicast setting and an rx_cfg, the Tx burst a UDP mode."""
    bt = etx.ring("slot0", 257)
    import test_gpu_ether as tge
    br = tge.burst("slot1520", 257)

    def tx():
        ring = pinned(bt.buf)
        l2, fl, launch = run_host(bt, ring)
        assert SERVED in launch
        check(bt, ring, l2, fl)

    def rx():
        ring = pinned(br.buf)
        act, fl, l2 = (np.full(br.n, 0xEE, np.uint8) for _ in range(3))
        netcsum.rx_burst_ether_host(ring[br.lead:], br.n, act, l2, flags=fl, eth_cfg=netcsum.ETHCFG_MCAST_RX, hw_addr=ef.HW,
                                    rx_cfg=netcsum.RXCFG_UDP_DISCARD_NO_CHK_SUM, **tge.call_args(br, host))
        assert "burst_server_kernel rx form=ether" in netcsum.last_launch()
        tge.check(br, (act, fl, l2), netcsum.ETHCFG_MCAST_RX, ef.HW, netcsum.RXCFG_UDP_DISCARD_NO_CHK_SUM)
        assert np.array_equal(ring, br.buf)                              # Rx writes nothing

    for step in ((tx, rx, tx, rx) if tx_first else (rx, tx, rx, tx)):
        step()


def test_ring_rewritten_in_place_between_bursts():
    b1, b2 = etx.ring("slot0", 257), etx.ring("slot0", 257, seed=1)
    ring = pinned(b1.buf)
    for b in (b1, b2, b1):
        ring[:] = b.buf
        l2, fl, launch = run_host(b, ring)
        assert SERVED in launch
        check(b, ring, l2, fl)
