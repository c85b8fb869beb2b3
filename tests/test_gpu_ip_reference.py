"""GPU parity of NetUtil_MI355X_RxBurst / RxValidateIP / RxBurstHost / RxBurstEther with the reference's own
IPv4 receive path, from tests/golden/reference_ip_vectors.json alone (what the untouched NetIPv4_Rx and
the ICMPv4, IGMP, UDP and TCP receive functions above it did with each datagram; see
test_ip_reference_cpu.py for the fixture, the rule tables and the one exception: a DROP where the
reference counted an earlier, non-checksum check).

Every fixture datagram — the per-protocol payload, bit, IHL and option sweeps, the structural faults, the
generated set — goes through the device as one burst, under rx_cfg 0 (held against the "ipv4" build) and
NETCSUM_RXCFG_UDP_DISCARD_NO_CHK_SUM (the "udpdis" build), in two layouts:

  packed1   offset/length datagrams back to back at their odd lengths, the first at +1, all four offset
            residues mod 4, the 9 036-octet datagram among them, the last datagram ending the allocation;
  slot1536  1536-B slots, datagram at +2, received lengths: the datagrams of up to 1 522 octets;

each judged by the run-stream form (pkt_stream_kernel, the default) and by the lane-group form
(pkt_batch_kernel, TUNE_KERNEL 2), asserted from last_launch(); once more from pinned host memory
(rx_burst_host); and once as Ethernet II frames (the interface's address, type 0x0800) through
rx_burst_ether: the datagrams of at least 46 octets, which make a frame of the minimum size without
padding (padding would change what the IP layer receives).

Checked: actions and flags against rules 1, 2, 3 and 5 of test_ip_reference_cpu.py, the flags of
rx_validate_ip equal to rx_burst's, and rx_burst_tally of the actions equal to the recorded movements of
each checksum counter plus the exception rows' DROPs, which are counted separately. Output buffers are
pre-filled with 0xEE.
"""
import functools

import numpy as np
import pytest

import ipvec as iv
import netcsum
import test_ip_reference_cpu as pin

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOT, SLOT_LEAD, SLOT_MAX = 1536, 2, 1522
HW = bytes.fromhex("02a1b2c3d4e5")
ETH_SRC = bytes.fromhex("0250607080a0")
FORMS = {0: "pkt_stream_kernel", 2: "pkt_batch_kernel"}


@pytest.fixture(autouse=True)
def _defaults():
    netcsum.tune(netcsum.TUNE_KERNEL, 0)
    yield
    netcsum.tune(netcsum.TUNE_KERNEL, 0)


@functools.lru_cache(maxsize=None)
def fixture():
    fx = iv.load()
    names, dg, _ = iv.all_dgrams(fx)
    return fx, names, dg, {lib: iv.outcomes_of(fx, lib) for lib in iv.LIBS}


@functools.lru_cache(maxsize=None)
def layout(kind):
    """-> (indices of the fixture datagrams in the burst, allocation, offsets, lengths) as numpy."""
    _, _, dg, _ = fixture()
    if kind == "packed1":
        idx = list(range(len(dg)))
        while not dg[idx[-1]]:                                               # (the last datagram is to end the allocation)
            idx.pop()
        lens = np.array([len(dg[i]) for i in idx], np.uint16)
        off = 1 + np.concatenate(([0], np.cumsum(lens[:-1].astype(np.uint64)))).astype(np.uint64)
        assert max(lens) > 9000 and len({int(o) % 4 for o in off}) == 4 and int(off[0]) == 1
    elif kind == "slot1536":
        idx = [i for i, d in enumerate(dg) if len(d) <= SLOT_MAX]
        while not dg[idx[-1]]:
            idx.pop()
        lens = np.array([len(dg[i]) for i in idx], np.uint16)
        off = (SLOT_LEAD + np.arange(len(idx), dtype=np.uint64) * np.uint64(SLOT)).astype(np.uint64)
    else:                                                                    # "ether": Ethernet II frames, packed at +1
        idx = [i for i, d in enumerate(dg) if len(d) >= 46]
        lens = np.array([14 + len(dg[i]) for i in idx], np.uint16)
        off = 1 + np.concatenate(([0], np.cumsum(lens[:-1].astype(np.uint64)))).astype(np.uint64)
    buf = np.full(int(off[-1]) + int(lens[-1]), 0xA5, np.uint8)              # nothing readable behind the last datagram
    for i, o in zip(idx, off):
        d = (HW + ETH_SRC + b"\x08\x00" if kind == "ether" else b"") + dg[i]
        buf[int(o):int(o) + len(d)] = np.frombuffer(d, np.uint8)
    return idx, buf, off.astype(np.int64), lens.view(np.int16)


def check(lib, idx, action, flags):
    """Rules 1, 2, 3, 5 per datagram, then the tally."""
    _, names, dg, recs = fixture()
    assert not (action == 0xEE).any() and not (flags == 0xEE).any()
    want, exc = [0] * netcsum.RX_NBR_ACTIONS, [0] * netcsum.RX_NBR_ACTIONS
    for k, i in enumerate(idx):
        r = recs[lib][i]
        kind = pin.check_rules(names[i], dg[i], r, int(flags[k]), int(action[k]), None)
        code = pin.recorded_drop(r)
        if kind == "exception":
            exc[int(action[k])] += 1
        elif code is not None:
            want[code] += 1
    tally = netcsum.rx_burst_tally(np.asarray(action, np.uint8))
    for a in range(1, 8):
        assert tally[a] == want[a] + exc[a], (lib, a, tally, want, exc)
    assert (want[4] > 0) == (lib == "udpdis") and 4 * sum(exc) <= sum(tally[1:8])
    if len(idx) > len(dg) // 2:                                              # (the Ethernet form judges the longer datagrams only)
        assert all(want[a] >= 20 for a in (1, 2, 3, 5, 6)) and (want[4] >= 20) == (lib == "udpdis")


@pytest.mark.parametrize("kernel", sorted(FORMS))
@pytest.mark.parametrize("kind", ["packed1", "slot1536"])
@pytest.mark.parametrize("lib", iv.LIBS)
def test_rx_burst_follows_the_recorded_reference(lib, kind, kernel):
    idx, buf, off, lens = layout(kind)
    n = len(idx)
    t, o, ln = torch.from_numpy(buf).to(DEV), torch.from_numpy(off).to(DEV), torch.from_numpy(lens).to(DEV)
    act = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    flg = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    flg_v = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    netcsum.tune(netcsum.TUNE_KERNEL, kernel)
    netcsum.rx_burst(t, n, act, flg, off=o, lens=ln, rx_cfg=pin.RX_CFG[lib])
    assert netcsum.last_launch().startswith(FORMS[kernel]), netcsum.last_launch()
    netcsum.rx_validate_ip(t, n, flg_v, off=o, lens=ln)
    assert netcsum.last_launch().startswith(FORMS[kernel]), netcsum.last_launch()
    torch.cuda.synchronize()
    flags = flg.cpu().numpy()
    assert (flg_v.cpu().numpy() == flags).all()
    check(lib, idx, act.cpu().numpy(), flags)


@pytest.mark.parametrize("lib", iv.LIBS)
def test_rx_burst_host_follows_the_recorded_reference(lib):
    idx, buf, off, lens = layout("packed1")
    n = len(idx)
    ring = torch.from_numpy(buf).pin_memory().numpy()
    act, flg = np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    netcsum.rx_burst_host(ring, n, act, flg, off=off, lens=lens, rx_cfg=pin.RX_CFG[lib])
    check(lib, idx, act, flg)


@pytest.mark.parametrize("lib", iv.LIBS)
def test_rx_burst_ether_follows_the_recorded_reference(lib):
    idx, buf, off, lens = layout("ether")
    n = len(idx)
    t, o, ln = torch.from_numpy(buf).to(DEV), torch.from_numpy(off).to(DEV), torch.from_numpy(lens).to(DEV)
    act, flg, l2 = (torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV) for _ in range(3))
    netcsum.rx_burst_ether(t, n, act, l2, flags=flg, off=o, lens=ln, rx_cfg=pin.RX_CFG[lib], eth_cfg=netcsum.ETHCFG_MCAST_RX, hw_addr=HW)
    torch.cuda.synchronize()
    assert (l2.cpu().numpy() == netcsum.L2_ETHER_IPV4).all()
    check(lib, idx, act.cpu().numpy(), flg.cpu().numpy())
