"""The 802.x frame demux against the reference's own IF/net_if_802x.c (CPU; no kernel launches).

tests/golden/reference_ether_vectors.json holds what the untouched NetIF_802x_Rx did with each frame
(tests/golden/make_ether_vectors.py recorded it through oracle/ref/glue_802x.c; tests/ethervec.py reads
it): three builds of the reference — v4v6 (IPv4 + IPv6, hence multicast receive), v4 (the template:
IPv4 with IGMP, multicast receive) and v4nomcast (IPv4, multicast off) — and per frame the error the
buffer was discarded with or the upper-layer receive function that was called, the buffer fields that
function saw, and the 802x error counters' deltas.

One table here (CLASS_OF_*) maps a recorded outcome to a NETCSUM_L2_* class and header length. It is
read off the class list of include/netcsum_mi355x.h (2b'''') — which names, per class, the
NET_IF_ERR_* code or the receive function — not off the code under test. With it, for v4v6 with
eth_cfg = MCAST_RX, v4 with MCAST_RX and v4nomcast with 0:

* ether_frames.classify (the Python rules) and netcsum.ether_class (the C rules the demux kernel
  shares) equal the recorded class and header length on every case;
* DataLen as the IP / ARP receive functions saw it equals octets received - header length;
* rx_burst_ether_tally over the classes gives RxInvFrameCtr, RxInvAddrDestCtr and RxInvAddrSrcCtr equal
  to the summed recorded deltas.

The one exception, asserted as such: frames typed IPv6 under the two IPv4-only builds. The reference
has no case for type 0x86DD there and discards them with the invalid-type error of their header form
(and counts RxInvFrameCtr); this project returns ETHER_IPV6 / SNAP_IPV6. The tests assert that
difference itself and that it is the only one: an IPv4-only stack must treat the *_IPV6 classes as its
invalid-type discard, and eth_cfg without MCAST_RX corresponds to no IPv6-enabled reference build
(IPv6 on Ethernet enables MLDP and with it multicast receive, Source/net_cfg_net.h).

The promiscuous form (hw_addr == NULL) has no reference counterpart — NetIF_802x_RxPktFrameDemux
always compares the destination — and stays pinned to the Python rules only (test_ether_cpu.py).

Where oracle/_ref/ holds the libraries, the recorder's --check and a seeded live differential of
20 000 generated frames per configuration run too; they skip, saying so, where it does not.
"""
import os
import re
import sys

import numpy as np
import pytest

import ether_frames as ef
import ethervec as ev
import netcsum

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN_DIR)
import make_ether_vectors as rec  # noqa: E402  (the recorder: no rule of this project in it)

needs_ref = pytest.mark.skipif(not ev.libs_available(),
                               reason="oracle/_ref/lib802x_ref_*.so are absent (no reference tree at build time)")
MCAST = netcsum.ETHCFG_MCAST_RX
ETH_CFG = {"v4v6": MCAST, "v4": MCAST, "v4nomcast": 0}
LIVE_FRAMES = 20000


def _header_classes():
    """{name: value} of the NETCSUM_L2_* defines, from the header's text."""
    text = open(os.path.join(netcsum.REPO, "include", "netcsum_mi355x.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define NETCSUM_L2_(\w+)\s+(\d+)u", text)}


L2 = _header_classes()
# include/netcsum_mi355x.h, the class list of (2b''''): the receive function and header form of the six
# accepted classes, the NET_IF_ERR_* code of each rejected one, and the counter each class belongs to
CLASS_OF_STUB = {("NetIPv4_Rx", 14): L2["ETHER_IPV4"], ("NetIPv6_Rx", 14): L2["ETHER_IPV6"], ("NetIPv4_Rx", 22): L2["SNAP_IPV4"],
                 ("NetIPv6_Rx", 22): L2["SNAP_IPV6"], ("NetARP_Rx", 14): L2["ETHER_ARP"], ("NetARP_Rx", 22): L2["SNAP_ARP"]}
CLASS_OF_ERR = {"NET_IF_ERR_INVALID_ADDR_DEST": L2["INV_ADDR_DEST"], "NET_IF_ERR_INVALID_ADDR_SRC": L2["INV_ADDR_SRC"],
                "NET_IF_ERR_INVALID_ETHER_TYPE": L2["INV_ETHER_TYPE"], "NET_IF_ERR_INVALID_LEN_FRAME": L2["INV_LEN_FRAME"],
                "NET_IF_ERR_INVALID_LLC_DSAP": L2["INV_LLC_DSAP"], "NET_IF_ERR_INVALID_LLC_SSAP": L2["INV_LLC_SSAP"],
                "NET_IF_ERR_INVALID_LLC_CTRL": L2["INV_LLC_CTRL"], "NET_IF_ERR_INVALID_SNAP_CODE": L2["INV_SNAP_CODE"],
                "NET_IF_ERR_INVALID_SNAP_TYPE": L2["INV_SNAP_TYPE"]}
COUNTER_OF = {L2["INV_FRAME_SIZE"]: "RxInvFrameCtr", L2["INV_ADDR_DEST"]: "RxInvAddrDestCtr", L2["INV_ADDR_SRC"]: "RxInvAddrSrcCtr",
              **{L2[k]: "RxInvFrameCtr" for k in ("INV_ETHER_TYPE", "INV_LEN_FRAME", "INV_LLC_DSAP", "INV_LLC_SSAP", "INV_LLC_CTRL",
                                                  "INV_SNAP_CODE", "INV_SNAP_TYPE")}}
V6_CLASSES = {L2["ETHER_IPV6"]: ("NET_IF_ERR_INVALID_ETHER_TYPE", 14), L2["SNAP_IPV6"]: ("NET_IF_ERR_INVALID_SNAP_TYPE", 22)}
CTRS = ("RxInvFrameCtr", "RxInvAddrDestCtr", "RxInvAddrSrcCtr")


def recorded_class(r, ctr_names):
    """(class, header length) of one recorded outcome, with the record's own consistency checked."""
    ctr = dict(zip(ctr_names, r["ctr"]))
    assert r["ctr_err_other"] == 0 and r["stub_calls"] + r["discards"] == 1 and ctr["RxPktDisCtr"] == r["discards"], r
    assert ctr["NullPtrCtr"] == ctr["RxInvProtocolCtr"] == ctr["TxPktDisCtr"] == ctr["TxInvProtocolCtr"] == 0, r
    if r["stub"] != "none":                                     # accepted: handed to ARP / IPv4 / IPv6
        assert r["err"] == "NET_IF_ERR_NONE" and r["ix"] == r["if_hdr_len"] and not any(ctr[k] for k in CTRS), r
        return CLASS_OF_STUB[(r["stub"], r["if_hdr_len"])], r["if_hdr_len"]
    assert r["err"] == "NET_ERR_RX" and r["if_hdr_len"] == 0, r
    if r["err_discard"] == "NET_ERR_NONE":                      # discarded before any check set an error: the frame size
        cls = L2["INV_FRAME_SIZE"]
    else:
        cls = CLASS_OF_ERR[r["err_discard"]]
    assert {k: ctr[k] for k in CTRS} == {k: int(k == COUNTER_OF[cls]) for k in CTRS}, r
    return cls, 0


def is_v6_exception(lib, rec_r, got):
    """The one allowed difference: an IPv4-only build discarded the frame for its type, we say *_IPV6."""
    if lib == "v4v6" or got[0] not in V6_CLASSES:
        return False
    err, hdr = V6_CLASSES[got[0]]
    return rec_r["stub"] == "none" and rec_r["err_discard"] == err and got[1] == hdr


def typed_ipv6(f: bytes) -> bool:
    """The frame's Ethernet II type or, behind a length word, its SNAP type is 0x86DD (octets only)."""
    if len(f) < 22:
        return False
    return f[12:14] == b"\x86\xdd" or (int.from_bytes(f[12:14], "big") <= 1500 and f[20:22] == b"\x86\xdd")


@pytest.fixture(scope="module")
def fx():
    return ev.load()


@pytest.fixture(scope="module")
def frames(fx):
    return ev.all_frames(fx)                                    # (names, frames); checks the generated set's SHA-256


# ------------------------------------------------------------------ always: the fixture alone
def test_fixture_is_small_and_covers_what_it_should(fx, frames):
    assert os.path.getsize(ev.FIXTURE) <= rec.MAX_BYTES
    names = set(frames[0])
    assert len(names) == len(frames[0]) and fx["generated"]["count"] >= 2000 and bytes.fromhex(fx["hw"]) == ev.HW == ef.HW
    for n in rec.RECEIVED:
        assert f"received {n}: e2 v4" in names and f"received {n}: snap v4, length field 0" in names
    for w in (0, 1, 46, 1499, 1500, 1501, 1535, 1536, 0x7FF, 0x800, 0x801, 0x805, 0x806, 0x807, 0x86DC, 0x86DD, 0x86DE, 0xFFFF):
        assert f"word {w:#06x} at 60 received" in names and f"snap type {w:#06x}" in names
    for k in range(14, 20):
        for b in range(8):
            assert f"octet {k} bit {b} flipped" in names
    for k in range(6):
        assert f"dst differs in octet {k} by 0x02" in names and f"src all zero but octet {k}" in names
        assert f"src all ones but octet {k}" in names
    for n in (63, 64, 65, 1518):
        assert {f"length field received - 18 {d:+d} at {n} received" for d in (-1, 0, 1)} <= names
    assert sum(nm.startswith("pair: ") for nm in names) >= 12
    # every row of the two mixes is there, under its name
    import random
    mix = [nm for nm, _ in ef.frame_mix(random.Random(fx["mix_seed"]))]
    mix += ["fixed1514: " + nm for nm, _ in ef.fixed_len_mix(random.Random(fx["mix_seed"]))]
    assert [c["name"] for c in fx["cases"][:fx["mix_rows"]]] == mix
    # per library: the configuration it was built in, and every class it can produce at least 8 times
    assert {k: fx["out"][k]["cfg"] for k in ev.LIBS} == {k: rec.CFG_WANT[k] for k in ev.LIBS}
    for lib in ev.LIBS:
        recs, _ = ev.outcomes_of(fx, lib)
        count = np.bincount([recorded_class(r, fx["ctr_names"])[0] for r in recs], minlength=16)
        want = set(range(16)) - (set() if lib == "v4v6" else set(V6_CLASSES))
        assert {c for c in range(16) if count[c]} == want, (lib, count)
        assert min(count[c] for c in want) >= rec.MIN_PER_OUTCOME, (lib, count)


def test_every_frame_regenerates(fx, frames):
    names, fr = frames
    g = fx["generated"]
    assert ev.frames_sha256(fr[len(fx["cases"]):]) == g["sha256"]        # (all_frames checked it; stated here)
    assert max(len(f) for f in fr) == 65535 and min(len(f) for f in fr) == 0
    for c, f in zip(fx["cases"], fr):
        assert len(f) == c["n"] and f[:ev.HEAD].hex() == c["head"], c["name"]


@pytest.mark.parametrize("lib", ev.LIBS)
def test_both_rule_sets_equal_the_recorded_reference(fx, frames, lib):
    names, fr = frames
    recs, data_len = ev.outcomes_of(fx, lib)
    eth_cfg = ETH_CFG[lib]
    differing, l2, want_ctr = [], [], dict.fromkeys(CTRS, 0)
    for i, (nm, f, r) in enumerate(zip(names, fr, recs)):
        want = recorded_class(r, fx["ctr_names"])
        got_c, got_py = netcsum.ether_class(f, eth_cfg, ev.HW), ef.classify(f, eth_cfg, ev.HW)
        l2.append(got_c[0])
        for k, v in zip(fx["ctr_names"], r["ctr"]):
            if k in want_ctr:
                want_ctr[k] += v
        if got_c != want or got_py != want:
            for who, got in (("netcsum_ether.h", got_c), ("ether_frames.py", got_py)):
                assert is_v6_exception(lib, r, got) and typed_ipv6(f), (who, nm, f[:23].hex(), len(f), got, want, r)
            differing.append(i)
        elif want[1]:                                           # DataLen as the upper layer saw it
            assert int(data_len[i]) == len(f) - want[1], (nm, int(data_len[i]))
    # the differing cases are exactly the frames the IPv6-enabled build handed to NetIPv6_Rx and this build
    # discarded for their type: none beyond them, none of them left out
    if lib == "v4v6":
        assert differing == []
    else:
        v6recs, _ = ev.outcomes_of(fx, "v4v6")
        expect = [i for i, (a, b) in enumerate(zip(v6recs, recs)) if a["stub"] == "NetIPv6_Rx" and b["stub"] == "none"
                  and b["err_discard"] in ("NET_IF_ERR_INVALID_ETHER_TYPE", "NET_IF_ERR_INVALID_SNAP_TYPE")]
        assert differing == expect and len(differing) >= 2 * rec.MIN_PER_OUTCOME
        assert not any(r["stub"] == "NetIPv6_Rx" for r in recs)
    # the driver's tally: an IPv4-only stack counts the *_IPV6 classes as its invalid-type discard
    tally = netcsum.rx_burst_ether_tally(np.array(l2, np.uint8))
    got_ctr = dict.fromkeys(CTRS, 0)
    for cls, k in COUNTER_OF.items():
        got_ctr[k] += tally[cls]
    if lib != "v4v6":
        got_ctr["RxInvFrameCtr"] += sum(tally[c] for c in V6_CLASSES)
    assert got_ctr == want_ctr and all(want_ctr.values())


def test_multicast_off_with_ipv6_is_no_reference_build(fx, frames):
    """eth_cfg = 0 lets a caller drop group destinations and still get the *_IPV6 classes. No build of the
    reference is in that state: the IPv6-enabled one accepts every group destination the recorded frames
    carry, the multicast-off one knows no IPv6. Both halves are shown on the recorded frames."""
    names, fr = frames
    v6, _ = ev.outcomes_of(fx, "v4v6")
    nm4, _ = ev.outcomes_of(fx, "v4nomcast")
    group_v6 = [i for i, f in enumerate(fr) if len(f) >= 60 and f[0] & 1 and f[:6] != ev.BCAST and v6[i]["stub"] == "NetIPv6_Rx"]
    assert len(group_v6) >= rec.MIN_PER_OUTCOME
    for i in group_v6:
        assert netcsum.ether_class(fr[i], 0, ev.HW) == (L2["INV_ADDR_DEST"], 0)
        assert nm4[i]["err_discard"] == "NET_IF_ERR_INVALID_ADDR_DEST"
        assert netcsum.ether_class(fr[i], MCAST, ev.HW)[0] in V6_CLASSES


# ------------------------------------------------------------------ with the reference libraries
@needs_ref
def test_recorder_check_reproduces_the_committed_fixture(fx):
    with open(ev.FIXTURE) as f:
        assert f.read() == rec.generate(fx)


@needs_ref
@pytest.mark.parametrize("lib", ev.LIBS)
def test_live_differential_reference_vs_the_c_rules(lib):
    """20 000 seeded frames (ethervec.gen_frame: 0-1600 octets, biased towards every check) through the live
    library and netcsum.ether_class, under the same exception rule."""
    ref = ev.Ref802x(lib)
    assert ref.cfg == rec.CFG_WANT[lib]
    seen, n_exc = set(), 0
    for k, f in enumerate(ev.gen_frames("ether/live/" + lib, LIVE_FRAMES)):
        r, data_len = ref.rx(f)
        want = recorded_class(r, ref.ctr_names)
        got = netcsum.ether_class(f, ETH_CFG[lib], ev.HW)
        if got != want:
            assert is_v6_exception(lib, r, got) and typed_ipv6(f), (k, f[:23].hex(), len(f), got, want, r)
            n_exc += 1
        else:
            assert not (lib != "v4v6" and typed_ipv6(f) and want[0] in (L2["INV_ETHER_TYPE"], L2["INV_SNAP_TYPE"])), (k, f[:23].hex())
            if want[1]:
                assert data_len == len(f) - want[1]
        seen.add(want[0])
    assert seen == set(range(16)) - (set() if lib == "v4v6" else set(V6_CLASSES))
    assert (n_exc == 0) == (lib == "v4v6")
