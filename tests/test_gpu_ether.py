"""GPU parity of NetUtil_MI355X_RxBurstEther / RxBurstEtherHost (include/netcsum_mi355x.h (2b'''')).

Bursts of 1, 63, 64, 65, 255, 256, 257 and 1031 frames (around the wave, the demux block of 256 and the
packet kernels' runs) of the mix of tests/ether_frames.py — every layer-2 class, every single wrong
field, runts, address cases, type / version mismatches, good and corrupted datagrams behind both
headers — repeated or cut to n and shuffled by seed, in the layouts a driver hands over:

  packed    offset/length frames back to back at their odd lengths, the first at +0 / +1 / +2 / +3;
  slot1520  1520-B slots, frame at +0, received lengths and no offsets;
  slot1536  1536-B slots, frame at +2, received lengths and no offsets;
  fixed     1536-B slots, frame at +2, neither offsets nor lengths: 1514 octets per slot (the mix with
            the slots' stale octets behind each frame, and 802.3 frames whose length field is 1496).

In every layout the last frame ends exactly where the allocation does. Checked: the classes against the
Python rules; actions and flags against the packet oracle on frame[hdr:] (MALFORMED / DELIVER for a
frame without a datagram to check), and against rx_burst called directly on those datagrams;
last_launch(); both multicast settings, with and without the interface's address, the UDP discard
policy, no flags array; the host-memory form and the tally; bursts back to back on one stream; a burst
captured into a HIP graph and replayed.
"""
import functools
import random

import numpy as np
import pytest

import ether_frames as ef
import netcsum

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 63, 64, 65, 255, 256, 257, 1031]
LAYOUTS = ["packed0", "packed1", "packed2", "packed3", "slot1520", "slot1536", "fixed"]
MCAST = netcsum.ETHCFG_MCAST_RX


class Burst:
    """buf: the allocation; lead: the base pointer's offset in it; off / lens / stride / frame_len: the
    call's arguments; start[i], present[i]: frame i's offset from the base and its octets received."""


@functools.lru_cache(maxsize=None)
def _mix(fixed):
    rng = random.Random(11)
    return ef.fixed_len_mix(rng) if fixed else ef.frame_mix(rng)


@functools.lru_cache(maxsize=None)
def burst(layout, n):
    rng = random.Random(100 * n + len(layout))
    mix = list(_mix(layout == "fixed"))
    rng.shuffle(mix)
    if n == 1:                                                           # (not the frame of no octets alone)
        mix = [m for m in mix if len(m[1]) >= 60]
    picked = [mix[i % len(mix)] for i in range(n)]
    if n > len(mix):
        rng.shuffle(picked)
    b = Burst()
    b.names = [nm for nm, _ in picked]
    b.present = [f for _, f in picked]
    b.n = n
    b.off = b.lens = None
    b.stride = b.frame_len = 0
    if layout.startswith("packed"):
        b.lead = 0
        pos = int(layout[-1])
        b.start = []
        for f in b.present:
            b.start.append(pos)
            pos += len(f)
        b.off = np.array(b.start, np.uint64)
        b.lens = np.array([len(f) for f in b.present], np.uint16)
        size = pos
    else:
        b.stride, b.lead = (1520, 0) if layout == "slot1520" else (1536, 2)
        b.start = [i * b.stride for i in range(n)]
        if layout == "fixed":
            b.frame_len = 1514
        else:
            b.lens = np.array([len(f) for f in b.present], np.uint16)
        size = b.lead + b.start[-1] + len(b.present[-1])
    b.buf = np.frombuffer(rng.randbytes(size), np.uint8).copy()          # (stale octets between the frames)
    for s, f in zip(b.start, b.present):
        b.buf[b.lead + s:b.lead + s + len(f)] = np.frombuffer(f, np.uint8)
    assert b.lead + b.start[-1] + len(b.present[-1]) == b.buf.size       # the last frame ends the allocation
    return b


def call_args(b, to):
    kw = dict(stride=b.stride, frame_len=b.frame_len)
    if b.off is not None:
        kw["off"] = to(b.off.astype(np.int64))
    if b.lens is not None:
        kw["lens"] = to(b.lens.view(np.int16))
    return kw


def run_device(b, eth_cfg=MCAST, hw=ef.HW, rx_cfg=0, with_flags=True):
    t = torch.from_numpy(b.buf).to(DEV)
    to = lambda a: torch.from_numpy(a).to(DEV)
    act = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=DEV)
    l2 = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=DEV)
    fl = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=DEV) if with_flags else None
    netcsum.rx_burst_ether(t[b.lead:], b.n, act, l2, flags=fl, rx_cfg=rx_cfg, eth_cfg=eth_cfg, hw_addr=hw, **call_args(b, to))
    launch = netcsum.last_launch()
    torch.cuda.synchronize()
    return act.cpu().numpy(), fl.cpu().numpy() if with_flags else None, l2.cpu().numpy(), launch, t


def check(b, got, eth_cfg=MCAST, hw=ef.HW, rx_cfg=0):
    act, fl, l2 = got[:3]
    want_l2, hdr, want_fl, want_act = ef.expect(b.present, eth_cfg, hw, rx_cfg)
    bad = np.nonzero(l2 != want_l2)[0]
    assert bad.size == 0, [(int(i), b.names[i], int(l2[i]), int(want_l2[i])) for i in bad[:8]]
    bad = np.nonzero(act != want_act)[0]
    assert bad.size == 0, [(int(i), b.names[i], int(act[i]), int(want_act[i])) for i in bad[:8]]
    if fl is not None:
        bad = np.nonzero(fl != want_fl)[0]
        assert bad.size == 0, [(int(i), b.names[i], hex(int(fl[i])), hex(int(want_fl[i]))) for i in bad[:8]]
    for i, nm in enumerate(b.names):                                     # the hole this entry point closes
        if "snap" in nm and "tcp bad l4" in nm and want_l2[i] in (ef.SNAP_IPV4, ef.SNAP_IPV6):
            assert act[i] == netcsum.RX_DROP_TCP_CHK_SUM, nm
        if hdr[i] == 0:                                                  # no datagram to check
            assert act[i] == netcsum.RX_DELIVER and (fl is None or fl[i] == netcsum.PKT_MALFORMED), nm
    return want_l2, hdr


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rx_burst_ether_layouts(layout, n):
    b = burst(layout, n)
    act, fl, l2, launch, t = run_device(b)
    assert launch.startswith(f"ether_demux b={(n + 255) // 256} | pkt_"), launch
    want_l2, hdr = check(b, (act, fl, l2))
    if n >= 255:                                                         # the burst holds what it should
        assert set(range(16)) - set(want_l2.tolist()) <= ({ef.INV_FRAME_SIZE} if layout == "fixed" else set())
        assert (act == netcsum.RX_DROP_TCP_CHK_SUM).sum() >= 4 and (act == netcsum.RX_DELIVER_L4_UNVERIFIED).any()
    # the IP frames: byte for byte what rx_burst gives the datagrams at frame + hdr, len - hdr
    ip = np.nonzero(hdr)[0]
    if ip.size:
        off = np.array([b.start[i] + hdr[i] for i in ip], np.int64)
        lens = np.array([len(b.present[i]) - hdr[i] for i in ip], np.uint16)
        act2 = torch.full((ip.size,), 0xEE, dtype=torch.uint8, device=DEV)
        fl2 = torch.full((ip.size,), 0xEE, dtype=torch.uint8, device=DEV)
        netcsum.rx_burst(t[b.lead:], int(ip.size), act2, flags=fl2, off=torch.from_numpy(off).to(DEV),
                         lens=torch.from_numpy(lens.view(np.int16)).to(DEV))
        torch.cuda.synchronize()
        assert np.array_equal(act[ip], act2.cpu().numpy()) and np.array_equal(fl[ip], fl2.cpu().numpy())


@pytest.mark.parametrize("eth_cfg,hw,rx_cfg,with_flags", [
    (0, ef.HW, 0, True), (MCAST, ef.HW, 0, True), (0, None, 0, True), (MCAST, None, 0, True),
    (0, ef.OTHER, 0, True), (MCAST, ef.HW, netcsum.RXCFG_UDP_DISCARD_NO_CHK_SUM, True), (0, ef.HW, 0, False)])
def test_rx_burst_ether_configurations(eth_cfg, hw, rx_cfg, with_flags):
    for layout in ("packed1", "slot1520"):
        b = burst(layout, 257)
        got = run_device(b, eth_cfg, hw, rx_cfg, with_flags)
        check(b, got, eth_cfg, hw, rx_cfg)
        if rx_cfg:
            assert (got[0] == netcsum.RX_DROP_UDP_NO_CHK_SUM).any()


@pytest.mark.parametrize("layout,n_chunks", [("packed3", 0), ("packed3", 3), ("slot1520", 0), ("slot1520", 3),
                                             ("slot1536", 3), ("fixed", 0), ("fixed", 3),
                                             ("packed3", 7), ("slot1520", 7)])   # 7 chunks: every slot reused, the last short
def test_rx_burst_ether_host_form(layout, n_chunks):
    b = burst(layout, 257)
    dev = run_device(b)
    ring = torch.from_numpy(b.buf).pin_memory().numpy()                  # a pinned receive ring
    act, fl, l2 = (np.full(b.n, 0xEE, np.uint8) for _ in range(3))
    netcsum.rx_burst_ether_host(ring[b.lead:], b.n, act, l2, flags=fl, eth_cfg=MCAST, hw_addr=ef.HW, n_chunks=n_chunks,
                                **call_args(b, lambda a: a))
    assert netcsum.last_launch().startswith("ether_demux b=")
    assert np.array_equal(act, dev[0]) and np.array_equal(fl, dev[1]) and np.array_equal(l2, dev[2])
    want_l2, _ = check(b, (act, fl, l2))
    assert netcsum.rx_burst_ether_tally(l2) == [int((want_l2 == c).sum()) for c in range(netcsum.L2_NBR_CLASSES)]
    act2, l22 = np.full(b.n, 0xEE, np.uint8), np.full(b.n, 0xEE, np.uint8)
    netcsum.rx_burst_ether_host(ring[b.lead:], b.n, act2, l22, eth_cfg=MCAST, hw_addr=ef.HW, n_chunks=n_chunks,
                                **call_args(b, lambda a: a))             # no flags array
    assert np.array_equal(act2, act) and np.array_equal(l22, l2)


def test_two_bursts_back_to_back_on_one_stream():
    """The second call's descriptors take the first one's place in the stream's scratch lease; stream
    order keeps them apart, and each call keeps its own results."""
    s = torch.cuda.Stream()
    runs = []
    with torch.cuda.stream(s):
        for layout, n in (("slot1520", 257), ("packed2", 1031), ("fixed", 65), ("slot1520", 257)):
            b = burst(layout, n)
            t = torch.from_numpy(b.buf).to(DEV, non_blocking=False)
            to = lambda a: torch.from_numpy(a).to(DEV)
            kw = call_args(b, to)
            act, fl, l2 = (torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV) for _ in range(3))
            runs.append((b, t, kw, act, fl, l2))
        s.synchronize()
        for b, t, kw, act, fl, l2 in runs:                               # enqueued without a wait in between
            netcsum.rx_burst_ether(t[b.lead:], b.n, act, l2, flags=fl, eth_cfg=MCAST, hw_addr=ef.HW, stream=s, **kw)
            assert netcsum.last_launch().startswith("ether_demux b=")
    s.synchronize()
    for b, t, kw, act, fl, l2 in runs:
        check(b, (act.cpu().numpy(), fl.cpu().numpy(), l2.cpu().numpy()))


def test_graph_capture_follows_the_tx_scratch_rule():
    """The descriptors' lease under stream capture: after one uncaptured call on the stream the burst is
    captured into a HIP graph (its slot is then pinned to the graph); a later uncaptured burst on the
    same stream takes a slot of its own; the graph, replayed afterwards, still gives its own burst's
    results."""
    s = torch.cuda.Stream()
    b1, b2 = burst("slot1520", 257), burst("packed1", 1031)
    with torch.cuda.stream(s):
        t1, t2 = torch.from_numpy(b1.buf).to(DEV), torch.from_numpy(b2.buf).to(DEV)
        kw1, kw2 = (call_args(b, lambda a: torch.from_numpy(a).to(DEV)) for b in (b1, b2))
        act1, fl1, l21 = (torch.full((b1.n,), 0xEE, dtype=torch.uint8, device=DEV) for _ in range(3))
        act2, fl2, l22 = (torch.full((b2.n,), 0xEE, dtype=torch.uint8, device=DEV) for _ in range(3))
        netcsum.rx_burst_ether(t1[b1.lead:], b1.n, act1, l21, flags=fl1, eth_cfg=MCAST, hw_addr=ef.HW, stream=s, **kw1)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        netcsum.rx_burst_ether(t1[b1.lead:], b1.n, act1, l21, flags=fl1, eth_cfg=MCAST, hw_addr=ef.HW, stream=s, **kw1)
    with torch.cuda.stream(s):
        netcsum.rx_burst_ether(t2[b2.lead:], b2.n, act2, l22, flags=fl2, eth_cfg=MCAST, hw_addr=ef.HW, stream=s, **kw2)
    s.synchronize()
    check(b2, (act2.cpu().numpy(), fl2.cpu().numpy(), l22.cpu().numpy()))
    for x in (act1, fl1, l21):
        x.fill_(0xEE)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    check(b1, (act1.cpu().numpy(), fl1.cpu().numpy(), l21.cpu().numpy()))
