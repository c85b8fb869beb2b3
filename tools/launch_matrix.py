"""The launch decisions of the batch ABI, recorded: a seeded list of small cases on each side of every
threshold the host-side launch policy has, each returning NetUtil_MI355X_LastLaunch() after the call —
the kernel form, run length and plan the library chose. tests/test_gpu_launch_names.py replays the
list against tests/golden/launch_names.json; tests/test_abi_cpu.py replays tune_accept() (no device)
against tests/golden/tune_accept.json.

    python tools/launch_matrix.py            # on an MI355X: (re)writes both fixtures from the built library
    python tools/launch_matrix.py --tune     # CPU only: the Tune accept set alone

The fixtures are a record of what a known-good library decided; a refactor of the host layer replays
them and never re-records them.

Every case binds a plan id of its own (NetUtil_MI355X_PlanBind), so a plan another case (or test) left
at the same device addresses never reaches it, and resets every knob it set. No case is above 64 Ki
items; plan-ahead is forced with TUNE_PLAN_AHEAD 1 instead of reaching its automatic thresholds."""
import json
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _sub in ("uc-tcp-ip_amd",):
    _p = os.path.join(REPO, _sub)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import netcsum as nc  # noqa: E402

GOLDEN_NAMES = os.path.join(REPO, "tests", "golden", "launch_names.json")
GOLDEN_TUNE = os.path.join(REPO, "tests", "golden", "tune_accept.json")

# ------------------------------------------------------------------ the Tune accept set (no device)
TUNE_KEYS = list(range(-1, 41))
TUNE_VALUES = list(range(-3, 71)) + [127, 128, 129, 255, 256, 257, 512, 4096, 4097, 1 << 20, (1 << 20) + 1,
                                     10 ** 6, 10 ** 6 + 1]


def tune_accept():
    """key -> the NET_ERR of NetUtil_MI355X_Tune(key, v) for v in TUNE_VALUES, from a thread of its own
    (knobs are per thread: the caller's tuning is left alone)."""
    got = {}

    def work():
        L = nc.lib()
        for k in TUNE_KEYS:
            got[str(k)] = [int(L.NetUtil_MI355X_Tune(k, v)) for v in TUNE_VALUES]

    th = threading.Thread(target=work)
    th.start()
    th.join()
    return got


# ------------------------------------------------------------------ the launch matrix (MI355X)
DEFAULTS = {nc.TUNE_GRID_BLOCKS: 0, nc.TUNE_GROUP_LANES: 0, nc.TUNE_KERNEL: 0, nc.TUNE_CHUNKS: 0, nc.TUNE_TILE: -1,
            nc.TUNE_TX_PASSES: 0, nc.TUNE_PKT_BOUND: -1, nc.TUNE_BURST_ZERO_COPY: 3, nc.TUNE_PLAN_AHEAD: -1,
            nc.TUNE_CHAIN_COMBINE: -1}
SLOT_BYTES = 2048
MAX_N = 1 << 16
HDR = 64                                   # header bytes written per frame (covers every field Tx stores)


def _case(cid, kind, tune=(), batches=1, **kw):
    assert all(k in DEFAULTS for k, _ in tune), cid
    return dict(id=cid, kind=kind, tune=tuple(tune), batches=batches, **kw)


def cases():
    out = []
    T = nc
    # strided segments: (len, stride, pseudo, n, base offset)
    seg = [("hdr20_packed", 20, 20, 0, 4096, 0), ("hdr20_stride24", 20, 24, 0, 4096, 0),
           ("seg12_stride128", 12, 128, 0, 4096, 0), ("seg1500_4k", 1500, 1500, 12, 4096, 0),
           ("seg1500_64k", 1500, 1500, 12, 65536, 0), ("seg1024_64k", 1024, 1024, 12, 65536, 0),
           ("seg9000_8k", 9000, 9000, 12, 8192, 0), ("seg700_odd_sparse", 700, 1111, 12, 4096, 1)]
    for cid, ln, st, ph, n, bo in seg:
        out.append(_case("strided/" + cid, "strided", seg_len=ln, stride=st, pseudo=ph, n=n, base_off=bo))
    tuned = [("kernel1", [(T.TUNE_KERNEL, 1)]), ("kernel2", [(T.TUNE_KERNEL, 2)]), ("kernel3", [(T.TUNE_KERNEL, 3)]),
             ("kernel4", [(T.TUNE_KERNEL, 4)]), ("tile4", [(T.TUNE_TILE, 4)]), ("grid64", [(T.TUNE_GRID_BLOCKS, 64)]),
             ("group16_chunks6", [(T.TUNE_GROUP_LANES, 16), (T.TUNE_CHUNKS, 6)])]
    for cid, tune in tuned:
        out.append(_case("strided/seg1500_4k/" + cid, "strided", tune, seg_len=1500, stride=1500, pseudo=12, n=4096,
                         base_off=0))
    # offset/length segments
    out.append(_case("varlen/packed_40_9000", "varlen_packed", n=16384))
    out.append(_case("varlen/pool1480_in_1520", "varlen_pool", batches=5, n=65536, seg_len=1480, slot=1520, every=1))
    out.append(_case("varlen/pool1480_wide", "varlen_pool", batches=5, n=16384, seg_len=1480, slot=1520, every=4))
    out.append(_case("varlen/pool1480_sparse", "varlen_pool", batches=5, n=4096, seg_len=1480, slot=1520, every=11))
    out.append(_case("varlen/pool1480_in_1520/ahead", "varlen_pool", [(T.TUNE_PLAN_AHEAD, 1)], batches=2, n=65536,
                     seg_len=1480, slot=1520, every=1))
    # packets
    layouts = [("packed1500", 1500, 0, False), ("slot1520", 1520, 14, False), ("slot2048", 2048, 64, False),
               ("offlen1520", 1520, 14, True)]
    for tx in (False, True):
        for ver in (4, 6, 0):
            for lname, slot, lead, offlen in layouts:
                for n in (256, 16384, 65536):
                    out.append(_case(f"pkt/{'tx' if tx else 'rx'}/v{ver}/{lname}/n{n}", "pkt", tx=tx, ver=ver, slot=slot,
                                     lead=lead, offlen=offlen, n=n, batches=2 if n >= 16384 else 1))
    for b in range(5):
        out.append(_case(f"pkt/rx/v4/slot1520/bound{b}", "pkt", [(T.TUNE_PKT_BOUND, b)], tx=False, ver=4, slot=1520,
                         lead=14, offlen=False, n=16384, batches=2))
    for tx in (False, True):
        for ver in (4, 6):
            out.append(_case(f"pkt/{'tx' if tx else 'rx'}/v{ver}/slot1520/kernel2", "pkt", [(T.TUNE_KERNEL, 2)], tx=tx,
                             ver=ver, slot=1520, lead=14, offlen=False, n=4096))
    for tp in (1, 2):
        out.append(_case(f"pkt/tx/v4/slot1520/tx_passes{tp}", "pkt", [(T.TUNE_TX_PASSES, tp)], tx=True, ver=4, slot=1520,
                         lead=14, offlen=False, n=16384))
    out.append(_case("pkt/rx/v4/slot1520/ahead", "pkt", [(T.TUNE_PLAN_AHEAD, 1)], tx=False, ver=4, slot=1520, lead=14,
                     offlen=False, n=65536, batches=2))
    out.append(_case("pkt/rx/v0/offlen1520/ahead", "pkt", [(T.TUNE_PLAN_AHEAD, 1)], tx=False, ver=0, slot=1520, lead=14,
                     offlen=True, n=65536, batches=2))
    # chains
    for k in (0, 1, 3, 4, 5):
        out.append(_case(f"chains/kernel{k}", "chains", [(T.TUNE_KERNEL, k)]))
    for g in (16, 32, 64):
        out.append(_case(f"chains/group{g}", "chains", [(T.TUNE_GROUP_LANES, g)]))
    out.append(_case("chains/combine64", "chains", [(T.TUNE_CHAIN_COMBINE, 64)]))
    # host bursts from a pinned ring
    for tx in (False, True):
        for offlen in (False, True):
            for zc in (0, 1, 2, 3):
                out.append(_case(f"burst/{'tx' if tx else 'rx'}/{'offlen' if offlen else 'slot1520'}/zc{zc}", "burst",
                                 [(T.TUNE_BURST_ZERO_COPY, zc)], tx=tx, offlen=offlen, ext=False))
    out.append(_case("burst/tx/slot1520/ext_hdr_copy_path", "burst", tx=True, offlen=False, ext=True))
    # CRC-32
    out.append(_case("crc/strided_64", "crc", seg_len=64, n=4096, varlen=False))
    out.append(_case("crc/strided_1500", "crc", seg_len=1500, n=4096, varlen=False))
    out.append(_case("crc/varlen", "crc", seg_len=0, n=4096, varlen=True))
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids)
    return out


def frame_sizes(n, ver, uniform):
    """Datagram sizes of a ring: 1500 B each, or the 7 : 4 : 1 mix of small / 576 / 1500 B."""
    if uniform:
        return np.full(n, 1500, np.int64)
    small = 40 if ver == 4 else 60
    pick = np.random.default_rng(11).choice(3, size=n, p=[7 / 12, 4 / 12, 1 / 12])
    return np.array([small, 576, 1500], np.int64)[pick]


def frame_headers(sizes, ver):
    """(n, HDR) uint8: the first bytes of each frame — an IPv4 (20 B) or IPv6 (40 B) header and a TCP
    header (data offset 5), UDP for the 576-B datagrams; ver 0 alternates IPv4 / IPv6. Checksum fields
    zero (Tx computes them; Rx verdicts are not what this tool looks at)."""
    n = len(sizes)
    h = np.random.default_rng(12).integers(0, 256, size=(n, HDR), dtype=np.uint8)
    udp = sizes == 576
    v6 = np.full(n, ver == 6) if ver else (np.arange(n) % 2 == 1)
    # IPv4
    h4 = h.copy()
    h4[:, 0] = 0x45
    h4[:, 1] = 0
    h4[:, 2] = (sizes >> 8) & 0xFF
    h4[:, 3] = sizes & 0xFF
    h4[:, 6] = 0x40
    h4[:, 7] = 0
    h4[:, 8] = 64
    h4[:, 9] = np.where(udp, 17, 6)
    h4[:, 10:12] = 0
    # IPv6 (datagrams too small for an IPv6 + TCP header become 60 B)
    h6 = h.copy()
    s6 = np.maximum(sizes, 60)
    h6[:, 0] = 0x60
    h6[:, 4] = ((s6 - 40) >> 8) & 0xFF
    h6[:, 5] = (s6 - 40) & 0xFF
    h6[:, 6] = np.where(udp, 17, 6)
    h6[:, 7] = 64
    for hx, l4, sz in ((h4, 20, sizes), (h6, 40, s6)):
        ulen = sz - l4
        hx[:, l4 + 4] = np.where(udp, (ulen >> 8) & 0xFF, hx[:, l4 + 4])
        hx[:, l4 + 5] = np.where(udp, ulen & 0xFF, hx[:, l4 + 5])
        hx[:, l4 + 6] = np.where(udp, 0, hx[:, l4 + 6])
        hx[:, l4 + 7] = np.where(udp, 0, hx[:, l4 + 7])
        hx[:, l4 + 12] = np.where(udp, hx[:, l4 + 12], 0x50)
        hx[:, l4 + 16:l4 + 18] = np.where(udp[:, None], hx[:, l4 + 16:l4 + 18], 0)
    return np.where(v6[:, None], h6, h4)


def ext_long_datagram():
    """An IPv6 datagram whose Destination Options header is 1040 B of PadN options — past the window the
    burst kernels walk, so a zero-copy Tx burst finishes it on the copy path — then TCP with 100 B."""
    opts = (bytes([1, 253]) + bytes(253)) * 4 + bytes([1, 16]) + bytes(16)
    ext = bytes([6, 129]) + opts
    assert len(ext) == 1040
    tcp = bytearray(20 + 100)
    tcp[12] = 0x50
    l4 = ext + bytes(tcp)
    hdr = bytes([0x60, 0, 0, 0, len(l4) >> 8, len(l4) & 0xFF, 60, 64]) + bytes(range(32))
    return np.frombuffer(hdr + l4, np.uint8)


class Matrix:
    """The device buffers every case shares (allocated and filled once) and run(case)."""

    def __init__(self, device="cuda"):
        import torch
        torch.cuda.init()
        self.torch = torch
        self.dev = device
        self.big = torch.empty(MAX_N * SLOT_BYTES + 4096, dtype=torch.uint8, device=device)
        nc.fill(self.big, MAX_N * SLOT_BYTES, 0x5EED0001, 0)
        self.pseudo = torch.empty(MAX_N * 12 + 64, dtype=torch.uint8, device=device)
        nc.fill(self.pseudo, MAX_N * 12, 0x5EED0002, 0)
        self.out = torch.zeros(MAX_N * 8, dtype=torch.uint8, device=device)
        self.flags = torch.zeros(MAX_N, dtype=torch.uint8, device=device)
        torch.cuda.synchronize()
        self._plan_ids = {c["id"]: 0x4C4D0000 + i for i, c in enumerate(cases())}

    # -- helpers
    def _dev(self, a):
        return self.torch.from_numpy(a).to(self.dev)

    def _sync_name(self):
        self.torch.cuda.synchronize()
        return nc.last_launch()

    def run(self, case):
        """Makes the case's call(s), synchronises, and returns last_launch() — for a case of several
        batches on the same layout, each batch's string, joined by ' || '."""
        nc.plan_bind(self._plan_ids[case["id"]])
        try:
            for k, v in case["tune"]:
                nc.tune(k, v)
            call = getattr(self, "_" + case["kind"])(case)
            names = []
            for _ in range(case["batches"]):
                call()                      # (the binding raises unless NET_UTIL_ERR_NONE)
                names.append(self._sync_name())
            return " || ".join(names)
        finally:
            for k, _ in case["tune"]:
                nc.tune(k, DEFAULTS[k])
            nc.plan_bind(0)

    # -- one builder per kind: prepares the inputs, returns the call
    def _strided(self, c):
        n, ln, st, bo = c["n"], c["seg_len"], c["stride"], c["base_off"]
        assert bo + (n - 1) * st + ln <= MAX_N * SLOT_BYTES
        base = self.big[bo:]
        ph = self.pseudo if c["pseudo"] else None
        op = nc.OP_DATA_CALC if c["pseudo"] else nc.OP_HDR_CALC
        return lambda: nc.batch_strided(base, st, ln, ph, c["pseudo"], c["pseudo"], n, self.out, op)

    def _varlen_packed(self, c):
        n = c["n"]
        lens = np.random.default_rng(21).integers(40, 9001, size=n).astype(np.uint16)
        off = np.zeros(n, np.uint64)
        off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        assert int(off[-1]) + int(lens[-1]) <= MAX_N * SLOT_BYTES
        off_d, len_d = self._dev(off.view(np.int64)), self._dev(lens.view(np.int16))
        return lambda: nc.batch_varlen(self.big, off_d, len_d, self.pseudo, 12, 12, n, self.out, nc.OP_DATA_CALC)

    def _varlen_pool(self, c):
        n, slot = c["n"], c["slot"] * c["every"]
        assert (n - 1) * slot + 34 + c["seg_len"] <= MAX_N * SLOT_BYTES
        off = np.arange(n, dtype=np.uint64) * np.uint64(slot) + np.uint64(34)
        lens = np.full(n, c["seg_len"], np.uint16)
        off_d, len_d = self._dev(off.view(np.int64)), self._dev(lens.view(np.int16))
        return lambda: nc.batch_varlen(self.big, off_d, len_d, self.pseudo, 12, 12, n, self.out, nc.OP_DATA_CALC)

    def _pkt(self, c):
        n, slot, lead, ver = c["n"], c["slot"], c["lead"], c["ver"]
        assert n * slot <= MAX_N * SLOT_BYTES and lead + HDR <= slot
        sizes = frame_sizes(n, ver or 4, uniform=slot != 1520)
        self.big[: n * slot].view(n, slot)[:, lead:lead + HDR] = self._dev(frame_headers(sizes, ver))
        kw = dict(stride=slot, pkt_len=slot - lead)
        if c["offlen"]:
            off = np.arange(n, dtype=np.uint64) * np.uint64(slot)
            lens = np.maximum(sizes, 60).astype(np.uint16)
            kw = dict(off=self._dev(off.view(np.int64)), lens=self._dev(lens.view(np.int16)))
        name = ("tx_finalize_" if c["tx"] else "rx_validate_") + {4: "ipv4", 6: "ipv6", 0: "ip"}[ver]
        fn, base = getattr(nc, name), self.big[lead:]
        return lambda: fn(base, n, self.flags, **kw)

    def _chains(self, c):
        n, pieces = 1024, 5
        rng = np.random.default_rng(31)
        lens = rng.integers(1, 1461, size=n * pieces).astype(np.uint16)
        off = np.arange(n * pieces, dtype=np.uint64) * np.uint64(1520) + rng.integers(0, 32, size=n * pieces).astype(np.uint64)
        first = (np.arange(n + 1, dtype=np.uint32) * np.uint32(pieces))
        off_d, len_d = self._dev(off.view(np.int64)), self._dev(lens.view(np.int16))
        first_d = self._dev(first.view(np.int32))
        return lambda: nc.batch_chains(self.big, off_d, len_d, first_d, self.pseudo, 12, 12, n, self.out,
                                       nc.OP_DATA_CALC, n_pieces=n * pieces)

    def _burst(self, c):
        n, slot, lead = 64, 1520, 14
        sizes = frame_sizes(n, 4, uniform=False)
        buf = np.random.default_rng(41).integers(0, 256, size=n * slot + 256, dtype=np.uint8)
        buf[: n * slot].reshape(n, slot)[:, lead:lead + HDR] = frame_headers(sizes, 0)
        if c["ext"]:
            d = ext_long_datagram()
            assert len(d) <= slot - lead
            buf[5 * slot + lead:5 * slot + lead + len(d)] = d
        ring = self.torch.from_numpy(buf).pin_memory()
        self._keep = ring
        fl, act = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        kw = dict(stride=slot, pkt_len=slot - lead)
        if c["offlen"]:
            kw = dict(off=np.arange(n, dtype=np.uint64) * np.uint64(slot), lens=np.full(n, slot - lead, np.uint16))
        base = ring[lead:]
        if c["tx"]:
            return lambda: nc.tx_burst_host(base, n, fl, **kw)
        return lambda: nc.rx_burst_host(base, n, act, fl, **kw)

    def _crc(self, c):
        n = c["n"]
        out = self.out.view(self.torch.int32)
        if not c["varlen"]:
            return lambda: nc.crc32_strided(self.big, c["seg_len"], c["seg_len"], n, out)
        lens = np.random.default_rng(51).integers(1, 1501, size=n).astype(np.uint32)
        off = np.arange(n, dtype=np.uint64) * np.uint64(1520)
        off_d, len_d = self._dev(off.view(np.int64)), self._dev(lens.view(np.int32))
        return lambda: nc.crc32_varlen(self.big, off_d, len_d, n, out)


def record_names():
    m = Matrix()
    names = {}
    for c in cases():
        names[c["id"]] = m.run(c)
        print(c["id"], "->", names[c["id"]], flush=True)
    nc.thread_release()
    return names


def _write(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if "--tune" not in sys.argv[1:]:
        import torch  # noqa: F401  (before the library is loaded, as in the tests: one HIP runtime, torch's)
        _write(GOLDEN_NAMES, record_names())
        print("wrote", GOLDEN_NAMES)
    _write(GOLDEN_TUNE, {"values": TUNE_VALUES, "err": tune_accept()})
    print("wrote", GOLDEN_TUNE)
