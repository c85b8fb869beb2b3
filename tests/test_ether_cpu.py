"""CPU-side checks of the Ethernet-frame Rx burst (include/netcsum_mi355x.h (2b''''); no kernel launches):

* NetUtil_MI355X_EtherClass (the C rules of include/netcsum_ether.h, which the demux kernel shares)
  equals the Python restatement of the reference's 802.x receive checks (tests/ether_frames.py) on the
  whole frame mix — every class, every single wrong field, the order of checks — under both multicast
  settings, with and without the interface's address, and on 2 000 random frames per seed whose first
  23 octets are biased towards each check;
* NetUtil_MI355X_RxBurstEtherTally counts classes and rejects what RxBurstTally rejects;
* the burst entry points reject bad arguments before any device work;
* tests/c_ether/ether_caller.c (its own main, its own expectations) builds with
  -fsanitize=address,undefined -Werror -pedantic from host/netcsum_ether.c alone and exits 0.
"""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import ether_frames as ef
import netcsum

REPO = netcsum.REPO
E_NULL, E_ARG, OK = netcsum.NET_ERR_FAULT_NULL_PTR, netcsum.NET_UTIL_ERR_MI355X_INVALID_ARG, netcsum.NET_UTIL_ERR_NONE
CONFIGS = [(0, ef.HW), (netcsum.ETHCFG_MCAST_RX, ef.HW), (0, None), (netcsum.ETHCFG_MCAST_RX, None)]


def test_constants_are_the_header_s():
    names = ["ETHER_IPV4", "ETHER_IPV6", "SNAP_IPV4", "SNAP_IPV6", "ETHER_ARP", "SNAP_ARP", "INV_FRAME_SIZE", "INV_ADDR_DEST",
             "INV_ADDR_SRC", "INV_ETHER_TYPE", "INV_LEN_FRAME", "INV_LLC_DSAP", "INV_LLC_SSAP", "INV_LLC_CTRL", "INV_SNAP_CODE",
             "INV_SNAP_TYPE", "NBR_CLASSES"]
    hdr = open(os.path.join(REPO, "include", "netcsum_mi355x.h")).read()
    for k, nm in enumerate(names):                              # dense from 0: IP classes, ARP classes, INV_*
        assert getattr(netcsum, "L2_" + nm) == k
        assert f"#define NETCSUM_L2_{nm}" in hdr
        assert int(hdr.split(f"#define NETCSUM_L2_{nm}")[1].split()[0].rstrip("u")) == k
        if nm != "NBR_CLASSES":
            assert getattr(ef, nm) == k
    assert netcsum.ETHCFG_MCAST_RX == 1 and netcsum.RX_NBR_ACTIONS == 9


@pytest.mark.parametrize("eth_cfg,hw", CONFIGS)
def test_ether_class_equals_the_python_rules_on_the_mix(eth_cfg, hw):
    mix = ef.frame_mix(random.Random(5))
    seen = set()
    for name, f in mix:
        want = ef.classify(f, eth_cfg, hw)
        assert netcsum.ether_class(f, eth_cfg, hw) == want, name
        seen.add(want[0])
    want_seen = set(range(netcsum.L2_NBR_CLASSES)) - ({ef.INV_ADDR_DEST} if hw is None else set())
    assert seen == want_seen                                    # the mix reaches every class


def test_mix_rows_get_the_class_the_issue_names():
    """A few rows by name, so that a mistake shared by both classifiers would still show."""
    mix = dict(ef.frame_mix(random.Random(5)))
    cls = lambda name, cfg=0, hw=ef.HW: netcsum.ether_class(mix[name], cfg, hw)
    assert cls("e2 v4 tcp") == (ef.ETHER_IPV4, 14) and cls("snap v6 tcp bad l4") == (ef.SNAP_IPV6, 22)
    assert cls("e2 type 0x8100") == cls("e2 type 0x8035") == cls("e2 type 0x05dd") == (ef.INV_ETHER_TYPE, 0)
    assert cls("len 1500 (snap path, v4 garbage)") == (ef.SNAP_IPV4, 22)
    assert cls("snap len+1") == (ef.INV_LEN_FRAME, 0) and cls("snap 64 octets, wrong len field") == (ef.INV_LEN_FRAME, 0)
    assert cls("snap 60 octets, wrong len field") == cls("snap 63 octets, wrong len field") == (ef.SNAP_IPV4, 22)
    assert cls("received 59") == (ef.INV_FRAME_SIZE, 0) and cls("received 60") == (ef.ETHER_IPV4, 14)
    assert cls("dst mcast v4") == (ef.INV_ADDR_DEST, 0) and cls("dst mcast v4", 1) == (ef.ETHER_IPV4, 14)
    assert cls("dst other v4") == cls("dst other hi v4") == (ef.INV_ADDR_DEST, 0)
    assert cls("dst other v4", 0, None) == (ef.ETHER_IPV4, 14)
    assert cls("dst other + src null") == (ef.INV_ADDR_DEST, 0) and cls("dst other + src null", 0, None) == (ef.INV_ADDR_SRC, 0)
    assert cls("src bcast + bad type") == (ef.INV_ADDR_SRC, 0) and cls("src null + snap dsap") == (ef.INV_ADDR_SRC, 0)
    assert cls("type v4, nibble 6") == (ef.ETHER_IPV4, 14) and cls("snap type v6, nibble 4") == (ef.SNAP_IPV6, 22)
    # ... and the datagram the checksum pass is to see: none for a type / version mismatch
    assert ef.ip_datagram(mix["type v4, nibble 6"])[2] == b"" and ef.ip_datagram(mix["type v6, nibble 7"])[2] == b""
    assert ef.ip_datagram(mix["snap v4 tcp"])[2] == mix["snap v4 tcp"][22:]


def test_runt_is_classified_unread():
    assert netcsum.lib().NetUtil_MI355X_EtherClass(None, 59, 0, None, None) == ef.INV_FRAME_SIZE
    assert netcsum.ether_class(b"", 0, ef.HW) == (ef.INV_FRAME_SIZE, 0)


@pytest.mark.parametrize("seed", range(3))
def test_ether_class_equals_the_python_rules_on_random_frames(seed):
    rng = random.Random(seed)
    seen = set()
    for k in range(2000):
        f = ef.random_frame(rng)
        eth_cfg, hw = CONFIGS[k & 3]
        want = ef.classify(f, eth_cfg, hw)
        assert netcsum.ether_class(f, eth_cfg, hw) == want, (k, f[:23].hex(), len(f))
        seen.add(want[0])
    assert seen == set(range(netcsum.L2_NBR_CLASSES))           # the bias reaches the SNAP branch's end


def test_tally_and_its_errors():
    rng = random.Random(3)
    l2 = np.array([rng.randrange(netcsum.L2_NBR_CLASSES) for _ in range(1000)], np.uint8)
    assert netcsum.rx_burst_ether_tally(l2) == [int((l2 == c).sum()) for c in range(netcsum.L2_NBR_CLASSES)]
    assert netcsum.rx_burst_ether_tally([]) == [0] * netcsum.L2_NBR_CLASSES
    L = netcsum.lib()
    ctr = np.full(netcsum.L2_NBR_CLASSES, 7, np.uint32)
    bad = l2.copy()
    bad[999] = netcsum.L2_NBR_CLASSES
    assert L.NetUtil_MI355X_RxBurstEtherTally(bad.ctypes.data, 1000, ctr.ctypes.data) == E_ARG
    assert (ctr == 7).all()                                     # nothing counted
    assert L.NetUtil_MI355X_RxBurstEtherTally(l2.ctypes.data, 1000, ctr.ctypes.data) == OK      # adds to the counters
    assert [int(x) - 7 for x in ctr] == netcsum.rx_burst_ether_tally(l2)
    assert L.NetUtil_MI355X_RxBurstEtherTally(None, 1, ctr.ctypes.data) == E_NULL
    assert L.NetUtil_MI355X_RxBurstEtherTally(l2.ctypes.data, 1, None) == E_NULL
    assert L.NetUtil_MI355X_RxBurstEtherTally(None, 0, ctr.ctypes.data) == OK


def test_burst_entry_points_check_arguments_before_device_work():
    L = netcsum.lib()
    hw = (ctypes.c_uint8 * 6)(*ef.HW)
    #                               base off  len  stride flen n  rx eth hw  act fl   l2  stream / chunks
    assert L.NetUtil_MI355X_RxBurstEther(None, None, None, 64, 64, 0, 0, 0, None, None, None, None, None) == OK
    assert L.NetUtil_MI355X_RxBurstEther(16, None, None, 64, 64, 3, 0, 0, hw, None, None, 16, None) == E_NULL   # actions
    assert L.NetUtil_MI355X_RxBurstEther(16, None, None, 64, 64, 3, 0, 0, hw, 16, None, None, None) == E_NULL   # classes
    assert L.NetUtil_MI355X_RxBurstEther(None, None, None, 64, 64, 3, 0, 0, hw, 16, None, 16, None) == E_NULL   # base
    assert L.NetUtil_MI355X_RxBurstEther(16, None, None, 64, 64, 3, 2, 0, hw, 16, None, 16, None) == E_ARG      # rx_cfg
    assert L.NetUtil_MI355X_RxBurstEther(16, None, None, 64, 64, 3, 0, 2, hw, 16, None, 16, None) == E_ARG      # eth_cfg
    assert L.NetUtil_MI355X_RxBurstEther(16, None, None, 64, 64, 0, 0, 4, hw, 16, None, 16, None) == E_ARG      # ... n = 0 too
    assert L.NetUtil_MI355X_RxBurstEtherHost(None, None, None, 64, 64, 0, 0, 0, None, None, None, None, 4) == OK
    assert L.NetUtil_MI355X_RxBurstEtherHost(8, None, None, 64, 64, 3, 0, 0, hw, None, None, 8, 4) == E_NULL
    assert L.NetUtil_MI355X_RxBurstEtherHost(8, None, None, 64, 64, 3, 0, 0, hw, 8, None, None, 4) == E_NULL
    assert L.NetUtil_MI355X_RxBurstEtherHost(None, None, None, 64, 64, 3, 0, 0, hw, 8, None, 8, 4) == E_NULL
    assert L.NetUtil_MI355X_RxBurstEtherHost(8, None, None, 64, 64, 3, 4, 0, hw, 8, None, 8, 4) == E_ARG
    assert L.NetUtil_MI355X_RxBurstEtherHost(8, None, None, 64, 64, 3, 0, 8, hw, 8, None, 8, 4) == E_ARG
    # the binding: errors come back as NET_ERRs without a device, undersized buffers never reach the library
    buf, act, l2 = np.zeros(1000, np.uint8), np.zeros(5, np.uint8), np.zeros(5, np.uint8)
    assert netcsum.rx_burst_ether(buf, 5, None, l2, stride=64, frame_len=64, stream=0, check=False) == E_NULL
    assert netcsum.rx_burst_ether(buf, 5, act, l2, stride=64, frame_len=64, eth_cfg=2, stream=0, check=False) == E_ARG
    with pytest.raises(RuntimeError):
        netcsum.rx_burst_ether(buf, 5, act, l2, stride=64, frame_len=64, rx_cfg=6, stream=0)
    with pytest.raises(ValueError):
        netcsum.rx_burst_ether(buf, 5, act, l2[:4], stride=64, frame_len=64, stream=0)              # classes
    with pytest.raises(ValueError):
        netcsum.rx_burst_ether(buf, 5, act, l2, stride=250, frame_len=64, stream=0)                 # frames
    with pytest.raises(ValueError):
        netcsum.rx_burst_ether(buf, 5, act, l2, stride=200, lens=np.zeros(4, np.uint16), stream=0)  # lengths
    with pytest.raises(ValueError):
        netcsum.rx_burst_ether(buf, 5, act, l2, stride=64, frame_len=64, hw_addr=b"\x02" * 5, stream=0)
    with pytest.raises(ValueError):
        netcsum.rx_burst_ether_host(buf, 5, act[:4], l2, stride=64, frame_len=64)


def test_c_caller_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ether_caller_asan")
    cmd = ["gcc", "-std=c99", "-D_DEFAULT_SOURCE", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pedantic",
           "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c_ether", "ether_caller.c"),
           os.path.join(REPO, "uc-tcp-ip_amd", "host", "netcsum_ether.c"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert r.stdout.startswith("ether_caller ok")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
