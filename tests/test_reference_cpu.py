"""The oracles against the reference's own net_util.c.

tests/golden/reference_vectors.json holds what the reference's untouched Source/net_util.c returned
(value and *p_err) for the four checksum functions, the CRC-32 routines and the reflection; it was
recorded by tests/golden/make_reference_vectors.py from the libraries `make -C oracle` builds into
oracle/_ref/ where a reference tree is present. The first group of tests needs the fixture alone and
always runs: the C oracle, the numpy oracle, the oracle's batch entry points and the drop-in's
host-only CRC paths must reproduce every recorded value. The second group runs where oracle/_ref/ holds
the libraries (and skips, saying so, where it does not): the NET_BUF layout, the older golden file, the
recorder's --check and a seeded live differential, all against the live reference.
"""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import netcsum
import oracle
import oracle_np as onp
import refvec
from helpers import to_np_buf

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN_DIR)
import make_reference_vectors as rec  # noqa: E402  (the ctypes binding of the reference libraries; no oracle in it)

needs_ref = pytest.mark.skipif(not rec.ref_available(),
                               reason="oracle/_ref/libnetutil_ref.so is absent (no reference tree at build time)")


@pytest.fixture(scope="module")
def vec():
    return refvec.load()


def _checksum_cases(vec, lib):
    return [c for c in vec["small"] + vec["large"] if c["lib"] == lib]


# ------------------------------------------------------------------ always: the fixture alone
def test_fixture_is_small_and_covers_what_it_should(vec):
    assert os.path.getsize(refvec.FIXTURE) <= rec.MAX_BYTES
    notes = " ".join(c["note"] for c in vec["small"] + vec["large"] + vec["crc"])
    for must in ("RFC 1071", "IPv4 header KAT", "hdr 0B", "hdr 60B", "buf 0B pseudo1 ", "buf 65B pseudo40", "chain 6x",
                 "invalid proto", "NULL chain, 11-B", "all-ff", "all-zero", "all-carry", "DBG: NULL header", "DBG: size 0",
                 "DBG: only buffer empty", "DBG: index NONE", "buf 1499B", "buf 65535B", "total 131070 B", "total 131073 B",
                 "crc 0B", "crc 64B", "crc 1514B", "cbf43926"):
        assert must in notes, must
    assert {s["family"] for s in vec["sets"]} >= {"seg_hdrstream_kernel", "seg_hdr_kernel", "seg_small_kernel",
                                                   "seg_stream_kernel", "seg_pipe_kernel", "seg_stream_varlen_kernel",
                                                   "seg_live_varlen_kernel"}
    assert {s["family"] for s in vec["crc_sets"]} >= {"crc_lane_kernel", "crc_ilv_kernel"}
    for s in vec["sets"] + vec["crc_sets"]:
        assert s["n"] <= 4096 and s["bytes"] <= 40_000_000, s["id"]
    assert vec["net_buf_layout"] == rec.MIRROR_LAYOUT


def test_every_generated_input_has_its_recorded_sha256(vec):
    n = 0
    for c in vec["small"] + vec["large"]:
        for b in (c.get("chain") or []):
            if isinstance(b["data"], dict):
                refvec.bytes_of(b["data"])                    # raises on a mismatch
                n += 1
    for c in vec["crc"]:
        if isinstance(c["data"], dict):
            refvec.bytes_of(c["data"])
            n += 1
    for s in vec["sets"] + vec["crc_sets"]:
        sd = refvec.SetData(s)                               # raises on a mismatch
        assert hashlib.sha256(refvec.shake(s["seed"], s["bytes"])).hexdigest() == s["sha256"] and sd.bytes == s["bytes"]
        n += 1
    assert n >= 30


def _c_oracle(c, dbg):
    """(calc, verify, err_calc, err_verify) of the C oracle for a checksum case, same at every offset."""
    got = set()
    if c["kind"] == "hdr":
        data = refvec.bytes_of(c["data"])
        for off in c["offsets"]:
            hb = netcsum.HostBytes(data, off) if data is not None else None
            p, n = (hb.ptr if hb else None), c.get("size", len(data) if data is not None else 0)
            (v1, e1), (v2, e2) = oracle.hdr_calc(p, n, dbg), oracle.hdr_verify(p, n, dbg)
            got.add((v1, v2, e1, e2))
    else:
        chain, pseudo = refvec.chain_of(c), refvec.bytes_of(c["pseudo"])
        for off in c["pseudo_offsets"]:
            ch = netcsum.Chain(chain) if chain is not None else None
            ph = netcsum.HostBytes(pseudo, off) if pseudo is not None else None
            args = (ch.ptr if ch else None, ph.ptr if ph else None, len(pseudo) if pseudo is not None else 0)
            (v1, e1), (v2, e2) = oracle.data_calc(*args, dbg), oracle.data_verify(*args, dbg)
            got.add((v1, v2, e1, e2))
    assert len(got) == 1, (c["note"], got)
    return got.pop()


def _recorded(c):
    return (c["calc"], c["verify"], c["err_calc"], c["err_verify"])


def test_c_oracle_reproduces_the_checksum_vectors(vec):
    cases = _checksum_cases(vec, "ref")
    assert len(cases) > 200
    for c in cases:
        assert _c_oracle(c, False) == _recorded(c), c["note"]


def test_c_oracle_dbg_reproduces_the_dbg_vectors(vec):
    cases = _checksum_cases(vec, "dbg")
    assert len(cases) >= 15 and {c["err_calc"] for c in cases} >= {23, 200, 210, 211, 622}
    for c in cases:
        assert _c_oracle(c, True) == _recorded(c), c["note"]


def _np_oracle(c, dbg):
    if c["kind"] == "hdr":
        data = refvec.bytes_of(c["data"])[:c.get("size")] if "size" in c else refvec.bytes_of(c["data"])
        return (onp.hdr_calc(data), onp.hdr_verify(data), 200, 200)
    chain = refvec.chain_of(c)
    bufs = [to_np_buf(dict({"proto": netcsum.NET_PROTOCOL_TYPE_TCP_V4}, **b)) for b in chain] if chain is not None else None
    ph = refvec.bytes_of(c["pseudo"])
    (v1, e1), (v2, e2) = onp.data_calc(bufs, ph, dbg), onp.data_verify(bufs, ph, dbg)
    return (v1, v2, e1, e2)


def test_numpy_oracle_reproduces_the_checksum_vectors(vec):
    for c in _checksum_cases(vec, "ref"):
        assert _np_oracle(c, False) == _recorded(c), c["note"]
    for c in _checksum_cases(vec, "dbg"):
        if c["kind"] == "data":                               # (its header functions have no DBG form)
            assert _np_oracle(c, True) == _recorded(c), c["note"]


def test_oracle_crc_and_reflect_reproduce_the_vectors(vec):
    assert len(vec["crc"]) > 65
    for c in vec["crc"]:
        data = refvec.bytes_of(c["data"])
        assert oracle.crc32_calc(data) == (c["crc"], c["err_crc"]), c["note"]
        assert oracle.crc32_calc(data, cpl=True) == (c["cpl"], c["err_cpl"]), c["note"]
    for r in vec["reflect"]:
        assert oracle.reflect32(r["val"]) == r["out"], hex(r["val"])


def test_dropin_host_crc_and_reflect_reproduce_the_vectors(vec):
    """NetUtil_32BitCRC_Calc / _CalcCpl of up to 4096 octets and NetUtil_32BitReflect of the drop-in are
    host C (test_crc_cpu.py): no device is needed for them, so they are pinned here as well."""
    for c in vec["crc"]:
        data = refvec.bytes_of(c["data"])
        if data is not None and len(data) > 4096:
            continue
        for off in c["offsets"]:
            hb = netcsum.HostBytes(data, off) if data is not None else None
            p, n = (hb.ptr if hb else None), (len(data) if data is not None else 0)
            assert netcsum.CRC32Calc(p, n) == (c["crc"], c["err_crc"]), (c["note"], off)
            assert netcsum.CRC32Calc(p, n, cpl=True) == (c["cpl"], c["err_cpl"]), (c["note"], off)
    for r in vec["reflect"]:
        assert netcsum.Reflect32(r["val"]) == r["out"], hex(r["val"])


def test_oracle_batch_entry_points_reproduce_the_sets(vec):
    for s in vec["sets"]:
        sd = refvec.SetData(s)
        lens16 = sd.lens.astype(np.uint16)
        for op in (0, 1, 2, 3):
            if op >= 2 and sd.first is not None:
                continue                                      # chains: DATA ops only
            base = sd.base if op in (0, 2) else sd.verify_input(refvec.want(s, op - 1))
            ph, pl = (sd.pseudo, sd.pseudo_len) if op < 2 else (None, 0)
            if s["kind"] == "strided":
                got = oracle.batch_strided(base, sd.stride, sd.seg_len, ph, pl, pl, sd.n, op, seg_offset=sd.base_off)
            elif sd.first is None:
                got = oracle.batch_varlen(base, sd.off, lens16, ph, pl, pl, op)
            else:
                got = oracle.batch_chains(base, sd.off, lens16, sd.first, ph, pl, pl, sd.n, op)
            bad = np.nonzero(got != refvec.want(s, op))[0]
            assert bad.size == 0, (s["id"], op, bad[:5])
    for s in vec["crc_sets"]:
        sd = refvec.SetData(s)
        for cpl in (False, True):
            if s["kind"] == "crc_strided":
                got = oracle.crc32_batch(sd.base, sd.n, cpl, stride=sd.stride, length=sd.seg_len)
            else:
                got = oracle.crc32_batch(sd.base, sd.n, cpl, off=sd.off, lens=sd.lens.astype(np.uint32))
            assert np.array_equal(got, refvec.unpack(s["out"]["cpl" if cpl else "crc"], np.uint32, sd.n)), (s["id"], cpl)


def test_set_families_are_the_launch_names_rows(vec):
    for s in vec["sets"] + vec["crc_sets"]:
        assert refvec.launch_family(s) == s["family"]


# ------------------------------------------------------------------ with oracle/_ref: the live reference
@needs_ref
def test_reference_net_buf_layout_is_the_mirror():
    lay = rec.probe_layout()
    assert lay == rec.MIRROR_LAYOUT
    # and what include/netcsum_netbuf.h states: every offset and size the probe prints appears there
    hdr = open(os.path.join(netcsum.REPO, "include", "netcsum_netbuf.h")).read()
    c_src = r"""
        #include <stddef.h>
        #include <stdio.h>
        #include "netcsum_netbuf.h"
        #define F(f) printf("%s %zu\n", #f, offsetof(NET_BUF_HDR, f))
        int main(void) { F(NextBufPtr); F(ProtocolHdrType); F(ICMP_MsgIx); F(ICMP_HdrLen); F(TransportHdrIx);
            F(TransportHdrLen); F(DataLen); F(TotLen); printf("DataPtr %zu\n", offsetof(NET_BUF, DataPtr));
            printf("sizeof_NET_BUF_HDR %zu\n", sizeof(NET_BUF_HDR)); printf("sizeof_NET_BUF %zu\n", sizeof(NET_BUF));
            printf("sizeof_ProtocolHdrType %zu\n", sizeof(((NET_BUF_HDR *)0)->ProtocolHdrType)); return 0; }"""
    assert "NET_BUF_HDR" in hdr
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "p.c"), "w") as f:
            f.write(c_src)
        subprocess.run(["gcc", "-I", os.path.join(netcsum.REPO, "include"), "-o", os.path.join(td, "p"),
                        os.path.join(td, "p.c")], check=True)
        out = subprocess.run([os.path.join(td, "p")], check=True, capture_output=True, text=True).stdout
    assert {k: int(v) for k, v in (ln.split() for ln in out.splitlines())} == lay


@needs_ref
def test_existing_golden_file_equals_the_live_reference():
    ref = rec.Reference()
    cases = json.load(open(os.path.join(GOLDEN_DIR, "netutil_golden.json")))["cases"]
    assert len(cases) == 651
    for c in cases:
        if c["kind"] == "hdr":
            hb = netcsum.HostBytes(bytes.fromhex(c["data"]), c["offset"])
            assert ref.call("hdr_calc", hb.ptr, hb.len) == (c["calc"], c["err"]), c["note"]
            assert ref.call("hdr_verify", hb.ptr, hb.len) == (c["verify"], c["err"]), c["note"]
            continue
        chain = None
        if c["chain"] is not None:
            chain = [dict(b, data=bytes.fromhex(b["data"])) for b in c["chain"]]
        ch = netcsum.Chain(chain) if chain is not None else None
        ph = netcsum.HostBytes(bytes.fromhex(c["pseudo"]), c["pseudo_offset"]) if c["pseudo"] is not None else None
        args = (ch.ptr if ch else None, ph.ptr if ph else None, ph.len if ph else 0)
        assert ref.call("data_calc", *args) == (c["calc"], c["err"]), c["note"]
        assert ref.call("data_verify", *args) == (c["verify"], c["err"]), c["note"]


@needs_ref
def test_recorder_check_reproduces_the_committed_fixture():
    with open(refvec.FIXTURE) as f:
        assert f.read() == rec.generate()


LIVE_CASES = 8000          # chains; plus LIVE_CASES // 3 CRC inputs (sized by count: the same cases every run)


def _live_bytes(rng, n, pat):
    return rng.randbytes(n) if pat == "random" else refvec.pattern_bytes(pat, n)


def _live_buf(rng, length, pat):
    proto = rng.choice(rec.PROTOS)
    lead, hdr = rng.randint(0, 9), rng.randint(0, min(length, 60))
    b = {"data": _live_bytes(rng, lead + length + rng.randint(0, 5), pat), "proto": proto, "offset": rng.randint(0, 7)}
    if proto in (60, 61):
        b.update(icmp_ix=lead, icmp_hdr_len=hdr, data_len=length - hdr)
    elif proto == 48:
        b.update(tot_len=lead + length, data_len=length)
    else:
        b.update(transport_ix=lead, transport_hdr_len=hdr, data_len=length - hdr)
    return b


@needs_ref
def test_live_differential_reference_vs_both_oracles():
    """Seeded random chains (1..6 buffers, totals 0..65535 B, pseudo-headers of 0 / 1 / 11 / 12 / 40 B at
    alignments 0..7, every pattern) through the reference at -O2 and -O0, the C oracle and the numpy oracle;
    every third case through the DBG library against dbg=True; CRC inputs of 0..2000 B."""
    ref = rec.Reference()
    rng = random.Random(0x11FE)
    for k in range(LIVE_CASES):
        nbuf = rng.randint(1, 6)
        total = rng.choice((rng.randint(0, 64), rng.randint(0, 2000), rng.randint(0, 2000), rng.randint(0, 65535)))
        if k % 97 == 0:
            total = 65535
        pat = rng.choice(("random", "random", "random", "zero", "ff", "carry"))
        cuts = sorted(rng.randint(0, total) for _ in range(nbuf - 1))
        lens = [b - a for a, b in zip([0] + cuts, cuts + [total])]
        chain = [_live_buf(rng, x, pat) for x in lens]
        if k % 41 == 0:
            chain[rng.randrange(nbuf)]["proto"] = rng.choice((0, 40, 62, 80))
        plen = rng.choice((0, 1, 11, 12, 40))
        pseudo = _live_bytes(rng, plen, pat) if (plen or rng.random() < 0.5) else None
        dbg = k % 3 == 2
        ch = netcsum.Chain(chain) if k % 53 else None
        ph = netcsum.HostBytes(pseudo, rng.randint(0, 7)) if pseudo is not None else None
        args = (ch.ptr if ch else None, ph.ptr if ph else None, plen if pseudo is not None else 0)
        bufs = [to_np_buf(b) for b in chain] if ch else None
        for fn, np_fn in (("data_calc", onp.data_calc), ("data_verify", onp.data_verify)):
            want = ref.call(fn, *args, dbg=dbg)
            assert getattr(oracle, fn)(*args, dbg) == want, (k, fn, dbg, lens, plen)
            assert np_fn(bufs, pseudo, dbg) == want, (k, fn, dbg, lens, plen)
        if nbuf == 1 and total <= 2000 and total > 0:       # the header functions on the same bytes
            hb = netcsum.HostBytes(chain[0]["data"][:total], rng.randint(0, 7))
            for fn, np_fn in (("hdr_calc", onp.hdr_calc), ("hdr_verify", onp.hdr_verify)):
                want = ref.call(fn, hb.ptr, total, dbg=dbg)
                assert getattr(oracle, fn)(hb.ptr, total, dbg) == want, (k, fn)
                assert (np_fn(chain[0]["data"][:total]), 200) == want, (k, fn)
    for k in range(LIVE_CASES // 3):
        n = rng.choice((rng.randint(0, 70), rng.randint(0, 2000)))
        data = _live_bytes(rng, n, rng.choice(("random", "random", "zero", "ff", "carry")))
        hb = netcsum.HostBytes(data, rng.randint(0, 7))
        assert oracle.crc32_calc(data) == ref.call("crc", hb.ptr, n), (k, n)
        assert oracle.crc32_calc(data, cpl=True) == ref.call("crc_cpl", hb.ptr, n), (k, n)
        v = rng.getrandbits(32)
        assert oracle.reflect32(v) == ref.o2.reflect(v) == ref.o0.reflect(v)
