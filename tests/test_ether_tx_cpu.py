"""CPU-side checks of the Ethernet-frame Tx burst (include/netcsum_mi355x.h (2b'''''); no kernel launches):

* NetUtil_MI355X_EtherTxClass (the C rule NetCsum_L2TxClass of include/netcsum_ether.h, which the Tx demux
  kernel shares) equals the Python restatement of the reference's transmit path (tests/ether_tx_frames.py)
  on the Tx frame mix, on the Rx tests' random frames, and on every frame of
  tests/golden/reference_ether_vectors.json;
* on those recorded frames the Tx class equals the Rx class of a promiscuous interface wherever that one is
  an ETHER_* class or INV_FRAME_SIZE (the two rules differ only in the checks Tx does not make);
* the rule reads nothing of a frame shorter than 60 octets;
* the helpers' expected frames rebuild what the reference builds with the offload flags off;
* the two entry points reject bad arguments before any device work;
* tests/c_ether_tx/ether_tx_caller.c (its own main, its own expectations) builds with
  -fsanitize=address,undefined -Werror -pedantic from host/netcsum_ether.c alone and exits 0.
"""
import os
import random
import subprocess

import numpy as np
import pytest

import ether_frames as ef
import ether_tx_frames as etx
import ethervec
import netcsum

REPO = netcsum.REPO
E_NULL, E_ARG, OK = netcsum.NET_ERR_FAULT_NULL_PTR, netcsum.NET_UTIL_ERR_MI355X_INVALID_ARG, netcsum.NET_UTIL_ERR_NONE
ETHER_OR_SIZE = (ef.ETHER_IPV4, ef.ETHER_IPV6, ef.ETHER_ARP, ef.INV_FRAME_SIZE)


def test_tx_class_equals_the_python_rule_on_the_mix():
    mix = etx.frame_mix(random.Random(5))
    seen = set()
    for name, f in mix:
        want = etx.classify(f)
        assert netcsum.ether_tx_class(f) == want, name
        seen.add(want[0])
    assert seen == {ef.ETHER_IPV4, ef.ETHER_IPV6, ef.ETHER_ARP, ef.INV_FRAME_SIZE, ef.INV_ETHER_TYPE}


def test_mix_rows_get_the_class_the_contract_names():
    """A few rows by name, so that a mistake shared by both classifiers would still show."""
    mix = dict(etx.special_frames(random.Random(5)))
    cls = lambda name: netcsum.ether_tx_class(mix[name])
    assert cls("arp") == (ef.ETHER_ARP, 14)
    assert cls("type 0x88cc") == cls("type 0x8100") == cls("snap v4 tcp") == cls("snap v4 udp 60") == (ef.INV_ETHER_TYPE, 0)
    assert cls("runt 59") == (ef.INV_FRAME_SIZE, 0) and cls("exactly 60 (ack, 6 octets of padding)") == (ef.ETHER_IPV4, 14)
    assert cls("type v4, nibble 6") == (ef.ETHER_IPV4, 14) and cls("type v6, nibble 4") == (ef.ETHER_IPV6, 14)
    assert cls("src null (no address check)") == (ef.ETHER_IPV4, 14) and cls("v4 tcp 1514") == (ef.ETHER_IPV4, 14)
    # ... and the datagram the checksum pass is given: none for a type / version mismatch, ARP, INV_*
    for name in ("type v4, nibble 6", "type v6, nibble 4", "arp", "snap v4 tcp", "runt 59"):
        assert etx.datagram(mix[name])[1] == b"", name
    assert etx.datagram(mix["v4 tcp 1514"])[1] == mix["v4 tcp 1514"][14:]
    assert etx.tx_model(b"") == (b"", netcsum.PKT_MALFORMED)


@pytest.mark.parametrize("seed", range(3))
def test_tx_class_equals_the_python_rule_on_random_frames(seed):
    rng = random.Random(seed)
    seen = set()
    for k in range(2000):
        f = ef.random_frame(rng)
        want = etx.classify(f)
        assert netcsum.ether_tx_class(f) == want, (k, f[:23].hex(), len(f))
        seen.add(want[0])
    assert seen == {ef.ETHER_IPV4, ef.ETHER_IPV6, ef.ETHER_ARP, ef.INV_FRAME_SIZE, ef.INV_ETHER_TYPE}


def test_tx_class_on_the_reference_s_recorded_frames_and_against_rx():
    names, frames = ethervec.all_frames(ethervec.load())
    n_same = 0
    for name, f in zip(names, frames):
        tx = netcsum.ether_tx_class(f)
        assert tx == etx.classify(f), name
        rx = netcsum.ether_class(f, hw_addr=None)
        if rx[0] in ETHER_OR_SIZE:
            assert tx == rx, (name, tx, rx)
            n_same += 1
    assert n_same > 100


def test_length_rule_reads_nothing():
    assert netcsum.ether_tx_class(b"\x08", length=59) == (ef.INV_FRAME_SIZE, 0)     # a 1-octet buffer
    assert netcsum.lib().NetUtil_MI355X_EtherTxClass(None, 59, None) == ef.INV_FRAME_SIZE
    assert netcsum.ether_tx_class(b"") == (ef.INV_FRAME_SIZE, 0)
    f = dict(etx.special_frames(random.Random(1)))["exactly 60 (ack, 6 octets of padding)"]
    assert netcsum.ether_tx_class(f, length=59) == (ef.INV_FRAME_SIZE, 0) and netcsum.ether_tx_class(f)[0] == ef.ETHER_IPV4


def test_expected_frames_rebuild_the_reference_s():
    """The composition the GPU tests rely on: header + tx_burst_model(datagram incl. padding) is the
    Ethernet header, the datagram the reference builds with the offload flags off, then the padding."""
    rng = random.Random(9)
    n_pad = 0
    for i in range(300):
        v6 = bool(i % 2)
        kind = rng.choice(etx.V6_KINDS if v6 else etx.V4_KINDS)
        name, f, ref = etx.ip_frame(rng, v6, kind, rng.choice([rng.randint(0, 30), rng.randint(0, 1400)]), rng.random() < 0.8)
        _, _, out = etx.expect([f])
        assert out[0] == ref, (i, name)
        n_pad += len(f) == 60
    assert n_pad > 5


def test_entry_points_check_arguments_before_device_work():
    L = netcsum.lib()
    #                                   base off  len  stride flen n  flags l2  stream / chunks
    assert L.NetUtil_MI355X_TxBurstEther(None, None, None, 64, 64, 0, None, None, None) == OK
    assert L.NetUtil_MI355X_TxBurstEther(16, None, None, 64, 64, 3, None, None, None) == E_NULL             # classes
    assert L.NetUtil_MI355X_TxBurstEther(None, None, None, 64, 64, 3, None, 16, None) == E_NULL             # base
    assert L.NetUtil_MI355X_TxBurstEther(16, None, None, 64, 64, 0x80000000, None, 16, None) == E_ARG
    assert L.NetUtil_MI355X_TxBurstEther(None, None, None, 64, 64, 0x80000000, None, 16, None) == E_NULL    # NULL first
    assert L.NetUtil_MI355X_TxBurstEtherHost(None, None, None, 64, 64, 0, None, None, 4) == OK
    assert L.NetUtil_MI355X_TxBurstEtherHost(8, None, None, 64, 64, 3, None, None, 4) == E_NULL
    assert L.NetUtil_MI355X_TxBurstEtherHost(None, None, None, 64, 64, 3, None, 8, 4) == E_NULL
    assert L.NetUtil_MI355X_TxBurstEtherHost(8, None, None, 64, 64, 0xFFFFFFFF, None, 8, 0) == E_ARG
    assert L.NetUtil_MI355X_TxBurstEtherHost(None, None, None, 64, 64, 0xFFFFFFFF, None, 8, 0) == E_NULL
    # the binding: errors come back as NET_ERRs without a device, undersized buffers never reach the library
    buf, l2 = np.zeros(1000, np.uint8), np.zeros(5, np.uint8)
    assert netcsum.tx_burst_ether(buf, 5, None, stride=64, frame_len=64, stream=0, check=False) == E_NULL
    with pytest.raises(RuntimeError):
        netcsum.tx_burst_ether(buf, 5, None, stride=64, frame_len=64, stream=0)
    with pytest.raises(ValueError):
        netcsum.tx_burst_ether(buf, 5, l2[:4], stride=64, frame_len=64, stream=0)                   # classes
    with pytest.raises(ValueError):
        netcsum.tx_burst_ether(buf, 5, l2, stride=250, frame_len=64, stream=0)                      # frames
    with pytest.raises(ValueError):
        netcsum.tx_burst_ether(buf, 5, l2, stride=200, lens=np.zeros(4, np.uint16), stream=0)       # lengths
    with pytest.raises(ValueError):
        netcsum.tx_burst_ether(buf, 5, l2, flags=np.zeros(4, np.uint8), stride=64, frame_len=64, stream=0)
    with pytest.raises(ValueError):
        netcsum.tx_burst_ether_host(buf, 5, l2[:4], stride=64, frame_len=64)
    assert netcsum.tx_burst_ether_host(buf, 5, None, stride=64, frame_len=64, check=False) == E_NULL


def test_c_caller_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ether_tx_caller_asan")
    cmd = ["gcc", "-std=c99", "-D_DEFAULT_SOURCE", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pedantic",
           "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c_ether_tx", "ether_tx_caller.c"),
           os.path.join(REPO, "uc-tcp-ip_amd", "host", "netcsum_ether.c"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert r.stdout.startswith("ether_tx_caller ok")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
