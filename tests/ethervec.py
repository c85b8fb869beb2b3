"""Reader of tests/golden/reference_ether_vectors.json: what the reference's own NetIF_802x_Rx
(IF/net_if_802x.c, built by oracle/Makefile `ref` with the recording stubs of oracle/ref/glue_802x.c)
did with each frame, recorded by tests/golden/make_ether_vectors.py. The recorder, the CPU tests
(test_ether_reference_cpu.py) and the GPU tests (test_gpu_ether_reference.py) all build their frames
here, so a case means the same octets to each of them. Nothing here computes an expected value, and
nothing here uses the classification rules of this project (include/netcsum_ether.h, ether_frames.py).

Frames. An explicit case is {"name", "n": octets received, "head": hex of its first min(n, 64) octets};
octets 64 .. n-1 are hashlib.shake_256("ether/tail/" + name).digest(n - 64). The generated set is
`count` frames drawn by gen_frame() from one ShakeRng(seed) stream, in order; "sha256" is over every
frame's 2-octet little-endian length followed by its octets. No frame depends on the random module.

Outcomes. fixture["outcomes"] is the table of distinct records (everything the glue reports except
DataLen); fixture["out"][lib]["outcome"] holds one index into it per frame (explicit cases first, then
the generated set) and ["data_len"] the recorded DataLen, both packed as in refvec.pack().
"""
from __future__ import annotations

import hashlib
import json
import os
import struct

import numpy as np

import refvec

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_ether_vectors.json")
REF_DIR = os.path.join(os.path.dirname(HERE), "oracle", "_ref")
LIBS = ("v4v6", "v4", "v4nomcast")
LIB_FILES = {"v4v6": "lib802x_ref_v4v6.so", "v4v6_O0": "lib802x_ref_v4v6_O0.so", "v4": "lib802x_ref_v4.so",
             "v4nomcast": "lib802x_ref_v4nomcast.so"}
HEAD = 64                                   # octets of an explicit case stored as hex

HW = bytes.fromhex("02a1b2c3d4e5")          # the interface's address in every case
OTHER = bytes.fromhex("02a1b2c3d4e6")
OTHER_HI = bytes.fromhex("06a1b2c3d4e5")
SRC = bytes.fromhex("0250607080a0")
BCAST = b"\xff" * 6
MCAST = bytes.fromhex("01005e0000fb")
NULL = bytes(6)
T_IPV4, T_IPV6, T_ARP = 0x0800, 0x86DD, 0x0806
STUBS = ("none", "NetARP_Rx", "NetIPv4_Rx", "NetIPv6_Rx")


def libs_available() -> bool:
    return all(os.path.exists(os.path.join(REF_DIR, f)) for f in LIB_FILES.values())


def load():
    with open(FIXTURE) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------- explicit cases
def tail_bytes(name: str, n: int) -> bytes:
    return refvec.shake("ether/tail/" + name, n - HEAD) if n > HEAD else b""


def case_frame(case) -> bytes:
    head = bytes.fromhex(case["head"])
    assert len(head) == min(case["n"], HEAD), case["name"]
    return head + tail_bytes(case["name"], case["n"])


# ------------------------------------------------------------------------------------- generated frames
class ShakeRng:
    """A stream of shake_256(seed) octets read in order: the same numbers on any Python."""

    def __init__(self, seed: str, reserve: int = 1 << 16):
        self.seed, self.pos, self.buf = seed, 0, b""
        self._grow(reserve)

    def _grow(self, n):
        self.buf = refvec.shake(self.seed, max(n, 2 * len(self.buf)))

    def randbytes(self, n: int) -> bytes:
        if self.pos + n > len(self.buf):
            self._grow(self.pos + n)
        self.pos += n
        return self.buf[self.pos - n:self.pos]

    def u32(self) -> int:
        return struct.unpack("<I", self.randbytes(4))[0]

    def below(self, n: int) -> int:         # 0 .. n-1 (n far below 2^32: the bias is of no concern here)
        return self.u32() % n

    def randint(self, lo: int, hi: int) -> int:
        return lo + self.below(hi - lo + 1)

    def choice(self, seq):
        return seq[self.below(len(seq))]

    def chance(self, per_mille: int) -> bool:
        return self.below(1000) < per_mille


def gen_frame(rng: ShakeRng) -> bytes:
    """Random octets, 0-1600 of them, with octets 0-22 biased towards the values that reach each check:
    the bias of ether_frames.random_frame, drawn from a ShakeRng."""
    n = (rng.randint(0, 1600), rng.randint(56, 68), rng.randint(0, 1600))[rng.below(3)]
    f = bytearray(rng.randbytes(n))

    def put(k, b):
        f[k:k + len(b)] = b
        del f[n:]

    put(0, rng.choice([HW, HW, HW, BCAST, MCAST, OTHER, OTHER_HI, rng.randbytes(6)]))
    if rng.chance(100):
        put(6, rng.choice([NULL, BCAST, bytes(5) + b"\x01", b"\xff" * 5 + b"\xfe"]))
    c = rng.below(1000)
    if c < 300:
        put(12, struct.pack("!H", rng.choice([T_IPV4, T_IPV6, T_ARP, 0x8035, 0x8100, 1501, 1536])))
    elif c < 900:
        good = (n - 18) & 0xFFFF
        tl = rng.choice([good, good, good, (n - 17) & 0xFFFF, 1500, 0, rng.randint(0, 1500)])
        put(12, struct.pack("!H", min(tl, 1500)))
        for k, ok in ((14, 0xAA), (15, 0xAA), (16, 0x03), (17, 0), (18, 0), (19, 0)):
            if rng.chance(900):
                put(k, bytes([ok]))
        if rng.chance(900):
            put(20, struct.pack("!H", rng.choice([T_IPV4, T_IPV6, T_ARP, T_ARP + 1])))
    if rng.chance(500):
        put(rng.choice([14, 22]), bytes([rng.choice([0x45, 0x60, 0x75, 0x4F])]))
    return bytes(f)


def gen_frames(seed: str, count: int):
    rng = ShakeRng(seed, reserve=count * 900)
    return [gen_frame(rng) for _ in range(count)]


def frames_sha256(frames) -> str:
    h = hashlib.sha256()
    for f in frames:
        h.update(struct.pack("<H", len(f)))
        h.update(f)
    return h.hexdigest()


def all_frames(fx):
    """-> (names, frames) of the whole fixture: the explicit cases, then the generated set (checked
    against its recorded SHA-256)."""
    names = [c["name"] for c in fx["cases"]]
    frames = [case_frame(c) for c in fx["cases"]]
    g = fx["generated"]
    gen = gen_frames(g["seed"], g["count"])
    if frames_sha256(gen) != g["sha256"]:
        raise AssertionError("the generated frame set does not have the recorded SHA-256")
    return names + [f"generated[{i}]" for i in range(g["count"])], frames + gen


def outcomes_of(fx, lib):
    """-> (records, data_len): per frame the outcome record (a dict of fx["outcomes"]) and DataLen."""
    n = len(fx["cases"]) + fx["generated"]["count"]
    ix = np.frombuffer(refvec.base64.b64decode(fx["out"][lib]["outcome"]), np.uint8)
    assert ix.size == n
    dl = refvec.unpack(fx["out"][lib]["data_len"], np.uint16, n)
    return [fx["outcomes"][i] for i in ix], dl


# ------------------------------------------------------------------------------------- the live libraries
class Ref802x:
    """One build of the reference's net_if_802x.c behind oracle/ref/glue_802x.c."""

    def __init__(self, lib: str):
        import ctypes
        u32 = ctypes.c_uint32

        class Out(ctypes.Structure):
            _fields_ = [("err", ctypes.c_int32), ("err_discard", ctypes.c_int32), ("discards", u32), ("stub", u32),
                        ("stub_calls", u32), ("ix", u32), ("if_hdr_len", u32), ("data_len", u32), ("flags", u32),
                        ("ctr", u32 * 8), ("ctr_global", u32 * 8), ("ctr_err_other", u32)]

        self.ct, self.Out = ctypes, Out
        L = ctypes.CDLL(os.path.join(REF_DIR, LIB_FILES[lib]))
        L.Ref802x_Rx.argtypes = [ctypes.c_char_p, ctypes.c_uint16, ctypes.c_char_p, ctypes.POINTER(Out)]
        L.Ref802x_Rx.restype = ctypes.c_int
        L.Ref802x_Cfg.restype = u32
        L.Ref802x_ErrNames.restype = L.Ref802x_CtrNames.restype = ctypes.c_char_p
        self.L = L
        self.cfg = int(L.Ref802x_Cfg())
        self.errs = {k: int(v) for k, v in (ln.split() for ln in L.Ref802x_ErrNames().decode().splitlines())}
        self.err_name = {v: k for k, v in self.errs.items()}
        self.ctr_names = L.Ref802x_CtrNames().decode().split()

    def rx(self, frame: bytes, hw: bytes = HW):
        """-> (record without DataLen, DataLen). Error codes are recorded by name."""
        o = self.Out()
        buf = self.ct.create_string_buffer(bytes(frame), max(len(frame), 1))     # exactly the octets received
        assert self.L.Ref802x_Rx(buf, len(frame), hw, self.ct.byref(o)) == 0
        dis = self.ctr_names.index("RxPktDisCtr")             # (the global one is NetBuf_FreeBuf's to count)
        assert [c for k, c in enumerate(o.ctr) if k != dis] == [c for k, c in enumerate(o.ctr_global) if k != dis], \
            "interface and global 802x error counters differ"
        rec = {"err": self.err_name[o.err], "err_discard": self.err_name[o.err_discard], "discards": o.discards,
               "stub": STUBS[o.stub], "stub_calls": o.stub_calls, "ix": o.ix, "if_hdr_len": o.if_hdr_len, "flags": o.flags,
               "ctr": list(o.ctr), "ctr_err_other": o.ctr_err_other}
        return rec, int(o.data_len)
