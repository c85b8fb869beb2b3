"""GPU parity of NetUtil_MI355X_RxBurstEther / RxBurstEtherHost with the reference's own 802.x receive
path, from tests/golden/reference_ether_vectors.json alone (what the untouched NetIF_802x_Rx did with
each frame; see test_ether_reference_cpu.py for the fixture, the outcome -> class table and the one
exception: frames typed IPv6 under the two IPv4-only builds of the reference).

Every fixture frame — the rows of both mixes, the single-field sweeps, the pairs, the generated set — goes
through the demux kernel as one burst per reference configuration (v4v6 and v4 with
NETCSUM_ETHCFG_MCAST_RX, v4nomcast without), in two layouts:

  packed1   offset/length frames back to back at their odd lengths, the first at +1, the 9 018- and
            65 535-octet frames among them, the last frame ending the allocation;
  slot1536  1536-B slots, frame at +2, received lengths and no offsets: the frames of up to 1 522 octets;

and once per configuration through the host-memory form. Checked: d_l2 against the recorded class of
every frame, and the tally of d_l2 against the recorded RxInvFrameCtr / RxInvAddrDestCtr /
RxInvAddrSrcCtr deltas. Actions and flags are test_gpu_ether.py's matter.
"""
import functools

import numpy as np
import pytest

import ethervec as ev
import netcsum
import test_ether_reference_cpu as pin

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOT, SLOT_LEAD, SLOT_MAX = 1536, 2, 1522


@functools.lru_cache(maxsize=None)
def fixture():
    fx = ev.load()
    names, frames = ev.all_frames(fx)
    return fx, names, frames


@functools.lru_cache(maxsize=None)
def layout(kind):
    """-> (indices of the fixture frames in the burst, allocation, lead, call arguments as numpy)."""
    _, _, frames = fixture()
    if kind == "packed1":
        idx = list(range(len(frames)))
        lens = np.array([len(frames[i]) for i in idx], np.uint16)
        off = 1 + np.concatenate(([0], np.cumsum(lens[:-1].astype(np.uint64)))).astype(np.uint64)
        buf = np.full(int(off[-1]) + int(lens[-1]), 0xA5, np.uint8)
        for i, o in zip(idx, off):
            buf[int(o):int(o) + len(frames[i])] = np.frombuffer(frames[i], np.uint8)
        assert max(lens) == 65535 and lens[-1] > 0 and len({int(o) % 4 for o in off}) == 4
        return idx, buf, 0, dict(off=off.astype(np.int64), lens=lens.view(np.int16))
    idx = [i for i, f in enumerate(frames) if len(f) <= SLOT_MAX]
    while not frames[idx[-1]]:                                           # (the last frame is to end the allocation)
        idx.pop()
    lens = np.array([len(frames[i]) for i in idx], np.uint16)
    buf = np.full(SLOT_LEAD + (len(idx) - 1) * SLOT + int(lens[-1]), 0xA5, np.uint8)
    for k, i in enumerate(idx):
        buf[SLOT_LEAD + k * SLOT:SLOT_LEAD + k * SLOT + len(frames[i])] = np.frombuffer(frames[i], np.uint8)
    return idx, buf, SLOT_LEAD, dict(lens=lens.view(np.int16), stride=SLOT)


def check(lib, idx, l2):
    fx, names, frames = fixture()
    recs, _ = ev.outcomes_of(fx, lib)
    want_ctr, differing = dict.fromkeys(pin.CTRS, 0), 0
    for k, i in enumerate(idx):
        r = recs[i]
        want = pin.recorded_class(r, fx["ctr_names"])
        got = int(l2[k])
        for name, v in zip(fx["ctr_names"], r["ctr"]):
            if name in want_ctr:
                want_ctr[name] += v
        if got != want[0]:
            hdr = pin.V6_CLASSES.get(got, (None, 0))[1]
            assert pin.is_v6_exception(lib, r, (got, hdr)) and pin.typed_ipv6(frames[i]), \
                (lib, names[i], frames[i][:23].hex(), len(frames[i]), got, want)
            differing += 1
    assert (differing == 0) == (lib == "v4v6")
    tally = netcsum.rx_burst_ether_tally(np.asarray(l2, np.uint8))
    got_ctr = dict.fromkeys(pin.CTRS, 0)
    for cls, name in pin.COUNTER_OF.items():
        got_ctr[name] += tally[cls]
    if lib != "v4v6":                                                    # an IPv4-only stack's invalid-type discard
        got_ctr["RxInvFrameCtr"] += sum(tally[c] for c in pin.V6_CLASSES)
    assert got_ctr == want_ctr and all(want_ctr.values())


@pytest.mark.parametrize("kind", ["packed1", "slot1536"])
@pytest.mark.parametrize("lib", ev.LIBS)
def test_rx_burst_ether_equals_the_recorded_reference(lib, kind):
    idx, buf, lead, kw = layout(kind)
    n = len(idx)
    t = torch.from_numpy(buf).to(DEV)
    dkw = {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    act = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    l2 = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    netcsum.rx_burst_ether(t[lead:], n, act, l2, eth_cfg=pin.ETH_CFG[lib], hw_addr=ev.HW, **dkw)
    assert netcsum.last_launch().startswith(f"ether_demux b={(n + 255) // 256} | ")
    torch.cuda.synchronize()
    check(lib, idx, l2.cpu().numpy())


@pytest.mark.parametrize("lib", ev.LIBS)
def test_rx_burst_ether_host_equals_the_recorded_reference(lib):
    idx, buf, lead, kw = layout("packed1")
    n = len(idx)
    ring = torch.from_numpy(buf).pin_memory().numpy()
    act, l2 = np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    netcsum.rx_burst_ether_host(ring[lead:], n, act, l2, eth_cfg=pin.ETH_CFG[lib], hw_addr=ev.HW, **kw)
    check(lib, idx, l2)
