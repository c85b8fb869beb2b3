"""The launchers' fallback edges, which the other parametrisations skip: every lane-group and chunk
count of TUNE_KERNEL 1, 2 and 3 with and without non-temporal loads, the chain batch's groups and the
CRC forms' table widths and lane counts. Each run equals the oracle, and leaves the
NetUtil_MI355X_LastLaunch() string — with the NET_ERR each NetUtil_MI355X_Tune call returned — that the
library left before its launchers read their instantiations from tables: tests/golden/dispatch_edges.json,
recorded once from that library by walk() below and never re-recorded. A value Tune refuses (TUNE_CHUNKS 5
and 7, TUNE_CRC_WIDE 3, a TUNE_CRC_LANES that is no power of two, TUNE_GROUP_LANES 5) leaves the knob at
its default, which each run sets first; such a run records the refusal and the default's launch.

Shapes: 257 segments of 100 B at stride 104 with a 12-B pseudo-header, and 257 offset/length segments of
mixed odd lengths <= 300 B; 33 chains of 1-5 pieces; 65 x 100 B for the CRC."""
import json
import os

import numpy as np
import pytest

import netcsum
import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(netcsum.REPO, "tests", "golden", "dispatch_edges.json")
N = 257


def _tune(key, value, default):
    """Sets the knob to its default, then asks for value -> the NET_ERR of that request."""
    netcsum.tune(key, default)
    return int(netcsum.lib().NetUtil_MI355X_Tune(key, value))


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(DEV)


class Inputs:
    """Host and device copies of every shape, and the oracle's results, made once."""

    def __init__(self):
        rng = np.random.default_rng(20261)
        self.seg = rng.integers(0, 256, size=N * 104 + 64, dtype=np.uint8)
        self.ph = rng.integers(0, 256, size=N * 12 + 64, dtype=np.uint8)
        self.lens = (2 * rng.integers(0, 150, size=N) + 1).astype(np.uint16)          # odd, 1..299
        self.off = np.zeros(N, np.uint64)
        self.off[1:] = np.cumsum(self.lens[:-1].astype(np.uint64))                    # packed: odd starts too
        self.base = rng.integers(0, 256, size=int(self.off[-1]) + 300 + 64, dtype=np.uint8)
        self.want_strided = oracle.batch_strided(self.seg, 104, 100, self.ph, 12, 12, N, 0)
        self.want_varlen = oracle.batch_varlen(self.base, self.off, self.lens, self.ph, 12, 12, 0)
        # 33 chains of 1-5 pieces, each piece 1..1460 B, in 1520-B slots at odd and even starts
        self.n_ch = 33
        per = rng.integers(1, 6, size=self.n_ch)
        self.first = np.zeros(self.n_ch + 1, np.uint32)
        self.first[1:] = np.cumsum(per)
        npc = int(self.first[-1])
        self.p_len = rng.integers(1, 1461, size=npc).astype(np.uint16)
        self.p_off = np.arange(npc, dtype=np.uint64) * np.uint64(1520) + rng.integers(0, 32, size=npc).astype(np.uint64)
        self.cbase = rng.integers(0, 256, size=npc * 1520 + 64, dtype=np.uint8)
        self.want_chains = oracle.batch_chains(self.cbase, self.p_off, self.p_len, self.first, self.ph, 12, 12, self.n_ch, 0)
        self.crc = rng.integers(0, 256, size=65 * 100 + 64, dtype=np.uint8)
        self.want_crc = oracle.crc32_batch(self.crc, 65, True, stride=100, length=100)
        self.d = {k: _dev(getattr(self, k), t) for k, t in
                  (("seg", np.uint8), ("ph", np.uint8), ("lens", np.int16), ("off", np.int64), ("base", np.uint8),
                   ("first", np.int32), ("p_len", np.int16), ("p_off", np.int64), ("cbase", np.uint8), ("crc", np.uint8))}

    def strided(self):
        out = torch.zeros(N, dtype=torch.int16, device=DEV)
        netcsum.batch_strided(self.d["seg"], 104, 100, self.d["ph"], 12, 12, N, out)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint16), self.want_strided

    def varlen(self):
        out = torch.zeros(N, dtype=torch.int16, device=DEV)
        netcsum.batch_varlen(self.d["base"], self.d["off"], self.d["lens"], self.d["ph"], 12, 12, N, out)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint16), self.want_varlen

    def chains(self):
        out = torch.zeros(self.n_ch, dtype=torch.int16, device=DEV)
        netcsum.batch_chains(self.d["cbase"], self.d["p_off"], self.d["p_len"], self.d["first"], self.d["ph"], 12, 12,
                             self.n_ch, out, n_pieces=int(self.first[-1]))
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint16), self.want_chains

    def crcs(self):
        out = torch.zeros(65, dtype=torch.int32, device=DEV)
        netcsum.crc32_strided(self.d["crc"], 100, 100, 65, out, cpl=True)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32), self.want_crc


T = netcsum
KNOBS = {T.TUNE_KERNEL: 0, T.TUNE_GROUP_LANES: 0, T.TUNE_CHUNKS: 0, T.TUNE_NT_LOADS: -1, T.TUNE_CRC_KERNEL: 0,
         T.TUNE_CRC_WIDE: 1, T.TUNE_CRC_LANES: 0, T.TUNE_CRC_NT: 0}          # each knob's default


def _settings(part):
    """part -> [(id, [(knob, value), ...], the Inputs method names)]"""
    out = []
    if part.startswith("kernel"):
        kern = int(part[-1])
        for g in (1, 4, 8, 16, 32, 64):
            for k in range(1, 9):
                for nt in (0, 1):
                    out.append((f"{part}/g{g}/k{k}/nt{nt}", [(T.TUNE_KERNEL, kern), (T.TUNE_GROUP_LANES, g),
                                                            (T.TUNE_CHUNKS, k), (T.TUNE_NT_LOADS, nt)],
                                ("strided", "varlen")))
    elif part == "chains":
        for g in (0, 16, 32, 64, 8, 5):                     # 8: a lane group the chain batch has no kernel for
            out.append((f"chains/g{g}", [(T.TUNE_GROUP_LANES, g)], ("chains",)))
    else:
        for ck in (0, 1, 3):
            out.append((f"crc/kernel{ck}", [(T.TUNE_CRC_KERNEL, ck)], ("crcs",)))
        for w in (0, 1, 2, 3):
            for lanes in range(1, 17):
                for nt in (0, 1):
                    out.append((f"crc/ilv/w{w}/lanes{lanes}/nt{nt}", [(T.TUNE_CRC_KERNEL, 2), (T.TUNE_CRC_WIDE, w),
                                                                      (T.TUNE_CRC_LANES, lanes), (T.TUNE_CRC_NT, nt)],
                                ("crcs",)))
    return out


PARTS = ["kernel1", "kernel2", "kernel3", "chains", "crc"]


def walk(inputs, part):
    """id -> 'NET_ERRs of the Tune calls | last_launch() of each call', every result checked against the oracle."""
    got = {}
    try:
        for cid, knobs, calls in _settings(part):
            errs = [_tune(k, v, KNOBS[k]) for k, v in knobs]
            names = []
            for call in calls:
                have, want = getattr(inputs, call)()
                bad = np.nonzero(have != want)[0]
                assert bad.size == 0, (cid, call, [(int(i), int(have[i]), int(want[i])) for i in bad[:5]])
                names.append(netcsum.last_launch())
            got[cid] = ",".join(map(str, errs)) + " | " + " || ".join(names)
    finally:
        for k, v in KNOBS.items():
            netcsum.tune(k, v)
    return got


@pytest.fixture(scope="module")
def inputs():
    return Inputs()


@pytest.mark.parametrize("part", PARTS)
def test_fallback_edges(inputs, part):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = walk(inputs, part)
    assert sorted(got) == sorted(k for k in golden if k.startswith(part + "/"))
    diff = {k: (v, golden[k]) for k, v in got.items() if v != golden[k]}
    assert not diff, list(diff.items())[:5]


if __name__ == "__main__":                                   # records the fixture (from the library before the tables)
    inp = Inputs()
    rec = {}
    for p in PARTS:
        rec.update(walk(inp, p))
    with open(os.environ.get("DISPATCH_EDGES_OUT", GOLDEN), "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", len(rec), "entries")
