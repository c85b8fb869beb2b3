"""GPU parity against vectors recorded from the reference's own net_util.c.

Everything expected here comes from tests/golden/reference_vectors.json (tests/refvec.py reads it;
tests/golden/make_reference_vectors.py recorded it from the untouched Source/net_util.c): no oracle of
this project computes a value, and neither the reference tree nor oracle/_ref/ is read.

* the drop-in functions over every recorded single-call vector;
* the batch ABI under the default policy over every recorded set and op, bit for bit, and the kernel
  family NetUtil_MI355X_LastLaunch() names must be the one tests/golden/launch_names.json records for the
  shape, so the coverage of each family cannot move away silently;
* the 1500-B set under every forced segment kernel form, the chain set under every chain kernel;
* the single-call vectors laid out as rows of one offset/length batch (edge lengths 0, 1, 2, 3, 63, 64,
  65, 65535 side by side in one launch) and the multi-buffer ones as one chain batch. The batch ABI takes
  one pseudo-header length per call, so those go by pseudo-header length: one call per length and op.
"""
import json

import numpy as np
import pytest

import netcsum
import refvec

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"

VEC = refvec.load()
SETS = {s["id"]: s for s in VEC["sets"]}
CRC_SETS = {s["id"]: s for s in VEC["crc_sets"]}
with open(refvec.LAUNCH_NAMES) as _f:
    LAUNCH_NAMES = json.load(_f)
_plan_ids = iter(range(0x5EF00000, 0x5EF10000))


def _reset_tuning():
    for k in (netcsum.TUNE_GRID_BLOCKS, netcsum.TUNE_GROUP_LANES, netcsum.TUNE_BLOCK_THREADS,
              netcsum.TUNE_KERNEL, netcsum.TUNE_CHUNKS, netcsum.TUNE_GRID_MULT):
        netcsum.tune(k, 0)
    netcsum.tune(netcsum.TUNE_NT_LOADS, -1)
    netcsum.tune(netcsum.TUNE_TILE, -1)
    netcsum.tune(netcsum.TUNE_CHAIN_COMBINE, -1)


@pytest.fixture(autouse=True)
def _tuning_defaults():
    _reset_tuning()
    yield
    _reset_tuning()
    netcsum.plan_bind(0)


@pytest.fixture(scope="module")
def set_data():
    """Each set's inputs, built once and left unchanged."""
    cache = {}

    def get(sid):
        if sid not in cache:
            cache[sid] = refvec.SetData(SETS[sid] if sid in SETS else CRC_SETS[sid])
        return cache[sid]

    return get


def _dev(a, dtype=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if dtype is not None else a).to(DEV)


def _family(name: str) -> str:
    return name.split("<")[0].split(" ")[0]


def _run_set(sd, base_host, op, fresh_plan=True):
    """One batch call of set `sd` over `base_host` for `op` -> (results, last_launch())."""
    if fresh_plan:
        netcsum.plan_bind(next(_plan_ids))       # plans are keyed per layout: every call is a first batch
    base = _dev(base_host)
    ph = _dev(sd.pseudo) if (sd.pseudo is not None and op < 2) else None
    pl = sd.pseudo_len if op < 2 else 0
    out = torch.zeros(sd.n, dtype=torch.int16 if op in (0, 2) else torch.uint8, device=DEV)
    if sd.kind == "strided":
        assert sd.base_off + (sd.n - 1) * sd.stride + sd.seg_len <= base.numel()
        netcsum.batch_strided(base[sd.base_off:], sd.stride, sd.seg_len, ph, pl, pl, sd.n, out, op)
    else:
        assert int((sd.off + sd.lens).max()) <= base.numel()
        off, ln = _dev(sd.off, np.int64), _dev(sd.lens.astype(np.uint16), np.int16)
        if sd.first is None:
            netcsum.batch_varlen(base, off, ln, ph, pl, pl, sd.n, out, op)
        else:
            assert int(sd.first[-1]) == sd.rows()
            netcsum.batch_chains(base, off, ln, _dev(sd.first, np.int32), ph, pl, pl, sd.n, out, op, n_pieces=sd.rows())
    torch.cuda.synchronize()
    r = out.cpu().numpy()
    return (r.view(np.uint16) if op in (0, 2) else r), netcsum.last_launch()


def _ops(sd):
    return (0, 1) if sd.first is not None else (0, 1, 2, 3)


def _input(sd, s, op):
    """CALC ops run over the set's input, VERIFY ops over it with the recorded CALC results stored."""
    return sd.base if op in (0, 2) else sd.verify_input(refvec.want(s, op - 1))


def _assert_same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, [(int(i), int(got[i]), int(want[i])) for i in bad[:5]])


# ------------------------------------------------------------------------------------ drop-in
def test_dropin_checksums_reproduce_every_reference_vector():
    n = 0
    for c in VEC["small"] + VEC["large"]:
        if c["lib"] != "ref":
            continue
        if c["kind"] == "hdr":
            data = refvec.bytes_of(c["data"])
            for off in c["offsets"]:
                hb = netcsum.HostBytes(data, off)
                assert netcsum.HdrCalc(hb.ptr, hb.len) == (c["calc"], c["err_calc"]), (c["note"], off)
                assert netcsum.HdrVerify(hb.ptr, hb.len) == (c["verify"], c["err_verify"]), (c["note"], off)
        else:
            chain, pseudo = refvec.chain_of(c), refvec.bytes_of(c["pseudo"])
            for off in c["pseudo_offsets"]:
                ch = netcsum.Chain(chain) if chain is not None else None
                ph = netcsum.HostBytes(pseudo, off) if pseudo is not None else None
                args = (ch.ptr if ch else None, ph.ptr if ph else None, len(pseudo) if pseudo is not None else 0)
                assert netcsum.DataCalc(*args) == (c["calc"], c["err_calc"]), (c["note"], off)
                assert netcsum.DataVerify(*args) == (c["verify"], c["err_verify"]), (c["note"], off)
        n += 1
    assert n > 200


def test_dropin_crc_and_reflect_reproduce_every_reference_vector():
    device_path = 0
    for c in VEC["crc"]:
        data = refvec.bytes_of(c["data"])
        for off in c["offsets"]:
            hb = netcsum.HostBytes(data, off) if data is not None else None
            p, n = (hb.ptr if hb else None), (len(data) if data is not None else 0)
            assert netcsum.CRC32Calc(p, n) == (c["crc"], c["err_crc"]), (c["note"], off)
            assert netcsum.CRC32Calc(p, n, cpl=True) == (c["cpl"], c["err_cpl"]), (c["note"], off)
        device_path += data is not None and len(data) > 4096
    assert device_path >= 3                          # (up to 4096 octets the drop-in's CRC is host C)
    for r in VEC["reflect"]:
        assert netcsum.Reflect32(r["val"]) == r["out"], hex(r["val"])


# ------------------------------------------------------------------------------------ batch ABI, default policy
@pytest.mark.parametrize("sid", sorted(SETS))
def test_batch_sets_default_policy(sid, set_data):
    s, sd = SETS[sid], set_data(sid)
    family = refvec.launch_family(s)
    for op in _ops(sd):
        got, name = _run_set(sd, _input(sd, s, op), op)
        assert _family(name) == family, (sid, op, name)
        _assert_same(got, refvec.want(s, op), (sid, op, name))
        if op in (1, 3):
            assert 0 < int(got.sum()) < sd.n


def test_pool_set_again_on_its_plan(set_data):
    """A second and third batch on the same pool layout may run in the plan the first one left (the
    live-sector stream): whatever form it takes, the recorded values."""
    sid = "varlen/pool1480_in_1520"
    s, sd = SETS[sid], set_data(sid)
    netcsum.plan_bind(next(_plan_ids))
    base = _dev(sd.base)
    ph, off, ln = _dev(sd.pseudo), _dev(sd.off, np.int64), _dev(sd.lens.astype(np.uint16), np.int16)
    names = []
    for _ in range(3):
        out = torch.zeros(sd.n, dtype=torch.int16, device=DEV)
        netcsum.batch_varlen(base, off, ln, ph, 12, 12, sd.n, out, 0)
        torch.cuda.synchronize()
        names.append(netcsum.last_launch())
        _assert_same(out.cpu().numpy().view(np.uint16), refvec.want(s, 0), (sid, names))
    assert _family(names[0]) == s["family"], names


@pytest.mark.parametrize("sid", sorted(CRC_SETS))
def test_crc_sets_default_policy(sid, set_data):
    s, sd = CRC_SETS[sid], set_data(sid)
    family = refvec.launch_family(s)
    base = _dev(sd.base)
    for cpl in (False, True):
        out = torch.zeros(sd.n, dtype=torch.int32, device=DEV)
        if sd.kind == "crc_strided":
            assert (sd.n - 1) * sd.stride + sd.seg_len <= base.numel()
            netcsum.crc32_strided(base, sd.stride, sd.seg_len, sd.n, out, cpl=cpl)
        else:
            assert int((sd.off + sd.lens).max()) <= base.numel()
            netcsum.crc32_varlen(base, _dev(sd.off, np.int64), _dev(sd.lens.astype(np.uint32), np.int32), sd.n, out, cpl=cpl)
        torch.cuda.synchronize()
        name = netcsum.last_launch()
        assert _family(name) == family, (sid, name)
        _assert_same(out.cpu().numpy().view(np.uint32), refvec.unpack(s["out"]["cpl" if cpl else "crc"], np.uint32, sd.n),
                     (sid, cpl, name))


# ------------------------------------------------------------------------------------ batch ABI, forced forms
@pytest.mark.parametrize("kernel", [1, 2, 3, 4])
def test_seg1500_set_under_each_forced_form(kernel, set_data):
    sid = "strided/seg1500_pseudo12"
    s, sd = SETS[sid], set_data(sid)
    family = _family(LAUNCH_NAMES[f"strided/seg1500_4k/kernel{kernel}"])
    assert family == {1: "seg_batch_kernel", 2: "seg_pipe_kernel", 3: "seg_lds_kernel", 4: "seg_tile_kernel"}[kernel]
    netcsum.tune(netcsum.TUNE_KERNEL, kernel)
    for op in (0, 1, 2, 3):
        got, name = _run_set(sd, _input(sd, s, op), op)
        if op < 2 or kernel != 4:                    # (the set's shape with its pseudo-header is the recorded row)
            assert _family(name) == family, (kernel, op, name)
        _assert_same(got, refvec.want(s, op), (sid, kernel, op, name))


CHAIN_PASS1 = {0: "seg_live_varlen_kernel", 1: "chain_wave_kernel", 2: "chain_piece_kernel", 3: "chain_live_piece_kernel",
               4: "chain_piece_kernel", 5: "seg_live_varlen_kernel"}


@pytest.mark.parametrize("kernel", [0, 1, 2, 3, 4, 5])
def test_chain_set_under_each_chain_kernel(kernel, set_data):
    sid = "chains/2_45_pieces"
    s, sd = SETS[sid], set_data(sid)
    if f"chains/kernel{kernel}" in LAUNCH_NAMES:
        assert _family(LAUNCH_NAMES[f"chains/kernel{kernel}"]) == CHAIN_PASS1[kernel]
    netcsum.tune(netcsum.TUNE_KERNEL, kernel)
    for op in (0, 1):
        got, name = _run_set(sd, _input(sd, s, op), op)
        assert _family(name) == CHAIN_PASS1[kernel], (kernel, op, name)
        _assert_same(got, refvec.want(s, op), (sid, kernel, op, name))


# ------------------------------------------------------------------------------------ vectors as batches
def _valid(c):
    return c["lib"] == "ref" and c["err_calc"] == netcsum.NET_UTIL_ERR_NONE


class _Packer:
    """Pieces appended to one buffer, each at a chosen address modulo 8 (the device base is 256-B aligned)."""

    def __init__(self):
        self.buf = bytearray(b"\xa5" * 3)
        self.off, self.len = [], []

    def add(self, piece: bytes, align: int):
        self.buf += b"\x5a" * ((align - len(self.buf)) % 8)
        self.off.append(len(self.buf))
        self.len.append(len(piece))
        self.buf += piece

    def arrays(self):
        return (np.frombuffer(bytes(self.buf) + b"\xa5" * 8, np.uint8).copy(), np.array(self.off, np.uint64),
                np.array(self.len, np.uint16))


def _pseudo_rows(cases, plen):
    """The cases' pseudo-headers at stride plen + 3 (odd and even addresses in turn)."""
    if plen == 0:
        return None, 0
    stride = plen + 3
    a = np.zeros(len(cases) * stride + 8, np.uint8)
    for i, c in enumerate(cases):
        a[i * stride:i * stride + plen] = np.frombuffer(refvec.bytes_of(c["pseudo"]), np.uint8)
    return a, stride


def _by_pseudo_len(cases):
    groups = {}
    for c in cases:
        groups.setdefault(len(c["pseudo"]) // 2 if isinstance(c["pseudo"], str) else 0, []).append(c)
    return groups


def test_single_buffer_vectors_as_one_varlen_batch():
    cases = [c for c in VEC["small"] + VEC["large"] if c["kind"] == "data" and _valid(c) and c["chain"] is not None
             and len(c["chain"]) == 1]
    groups = _by_pseudo_len(cases)
    assert sorted(groups) == [0, 1, 11, 12, 40]
    for plen, group in sorted(groups.items()):
        pk = _Packer()
        for c in group:
            b = refvec.chain_of(c)[0]
            pk.add(refvec.piece_of(b), refvec.piece_align(b))
        lens = set(pk.len)
        assert lens >= {0, 1, 2, 3, 19, 20, 21, 40, 63, 64, 65}, (plen, sorted(lens))
        if plen == 12:
            assert lens >= {1499, 1500, 1501, 4520, 8999, 9000, 65535}, sorted(lens)
        base, off, ln = pk.arrays()
        assert int(off[-1]) + int(ln[-1]) <= base.size
        pseudo, pstride = _pseudo_rows(group, plen)
        base_d, off_d, ln_d = _dev(base), _dev(off, np.int64), _dev(ln, np.int16)
        ph_d = _dev(pseudo) if pseudo is not None else None
        n = len(group)
        for op, key in ((0, "calc"), (1, "verify")):
            netcsum.plan_bind(next(_plan_ids))
            out = torch.zeros(n, dtype=torch.int16 if op == 0 else torch.uint8, device=DEV)
            netcsum.batch_varlen(base_d, off_d, ln_d, ph_d, pstride, plen, n, out, op)
            torch.cuda.synchronize()
            r = out.cpu().numpy()
            got = r.view(np.uint16) if op == 0 else r
            bad = [(c["note"], int(g), c[key]) for c, g in zip(group, got) if int(g) != c[key]]
            assert not bad, (plen, op, netcsum.last_launch(), bad[:5])


def test_header_vectors_as_one_varlen_batch():
    cases = [c for c in VEC["small"] if c["kind"] == "hdr" and _valid(c)]
    assert len(cases) >= 64
    pk, rows = _Packer(), []
    for c in cases:
        for off in c["offsets"]:
            pk.add(refvec.bytes_of(c["data"]), off)
            rows.append(c)
    base, off, ln = pk.arrays()
    assert int(off[-1]) + int(ln[-1]) <= base.size
    base_d, off_d, ln_d = _dev(base), _dev(off, np.int64), _dev(ln, np.int16)
    for op, key in ((2, "calc"), (3, "verify")):
        netcsum.plan_bind(next(_plan_ids))
        out = torch.zeros(len(rows), dtype=torch.int16 if op == 2 else torch.uint8, device=DEV)
        netcsum.batch_varlen(base_d, off_d, ln_d, None, 0, 0, len(rows), out, op)
        torch.cuda.synchronize()
        r = out.cpu().numpy()
        got = r.view(np.uint16) if op == 2 else r
        bad = [(c["note"], int(g), c[key]) for c, g in zip(rows, got) if int(g) != c[key]]
        assert not bad, (op, netcsum.last_launch(), bad[:5])


def test_multi_buffer_vectors_as_one_chain_batch():
    cases = [c for c in VEC["small"] + VEC["large"] if c["kind"] == "data" and _valid(c)
             and (c["chain"] is None or len(c["chain"]) > 1)]
    groups = _by_pseudo_len(cases)
    assert len(cases) >= 40 and {0, 12} <= set(groups)
    for plen, group in sorted(groups.items()):
        pk, first = _Packer(), [0]
        for c in group:
            for b in (refvec.chain_of(c) or []):
                pk.add(refvec.piece_of(b), refvec.piece_align(b))
            first.append(len(pk.off))
        if not pk.off:
            pk.add(b"", 0)                           # (a batch of NULL chains alone still passes arrays)
        base, off, ln = pk.arrays()
        assert int((off + ln.astype(np.uint64)).max()) <= base.size
        pseudo, pstride = _pseudo_rows(group, plen)
        base_d, off_d, ln_d = _dev(base), _dev(off, np.int64), _dev(ln, np.int16)
        first_d = _dev(np.array(first, np.uint32), np.int32)
        ph_d = _dev(pseudo) if pseudo is not None else None
        n = len(group)
        for op, key in ((0, "calc"), (1, "verify")):
            out = torch.zeros(n, dtype=torch.int16 if op == 0 else torch.uint8, device=DEV)
            netcsum.batch_chains(base_d, off_d, ln_d, first_d, ph_d, pstride, plen, n, out, op, n_pieces=first[-1])
            torch.cuda.synchronize()
            r = out.cpu().numpy()
            got = r.view(np.uint16) if op == 0 else r
            bad = [(c["note"], int(g), c[key]) for c, g in zip(group, got) if int(g) != c[key]]
            assert not bad, (plen, op, netcsum.last_launch(), bad[:5])
