#!/usr/bin/env python3
"""Record tests/golden/reference_ether_vectors.json from the reference's own IF/net_if_802x.c.

`make -C oracle` builds the untouched net_if_802x.c of a reference tree, with the recording stubs of
oracle/ref/glue_802x.c above it, into oracle/_ref/ in three configurations (lib802x_ref_v4v6.so: IPv4
and IPv6, multicast receive on by implication; lib802x_ref_v4.so: the template as shipped, IPv4 with
IGMP, multicast receive on; lib802x_ref_v4nomcast.so: IPv4 only, multicast off) and an -O0 twin of the
first. This script hands NetIF_802x_Rx one frame at a time and writes down what came back: *p_err, *p_err
as it stood when the buffer was discarded (the discard routine overwrites it with NET_ERR_RX), which
upper-layer stub ran and the buffer fields it saw, and the deltas of the 802x error counters. No rule
of this project computes anything here: the only expectations are the named rows below whose outcome
can be stated without any code, which are asserted. Every case must give the same record at -O0 and -O2.

    python tests/golden/make_ether_vectors.py           # rewrites the fixture
    python tests/golden/make_ether_vectors.py --check   # regenerates in memory, compares with the file

The frames are described in tests/ethervec.py. The rows of ether_frames.frame_mix / fixed_len_mix are
built with the random module when the fixture is first written; the fixture stores their deciding octets
as hex, and --check takes those rows' octets from the committed file, so that nothing that is compared
rests on the random module (a difference from what the random module gives today is only reported).
"""
import collections
import json
import os
import random
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for sub in ("oracle", "uc-tcp-ip_amd", "tests"):
    sys.path.insert(0, os.path.join(REPO, sub))

import ethervec as ev   # noqa: E402
import refvec           # noqa: E402

MAX_BYTES = 377023      # the cap of tests/golden/reference_vectors.json: this fixture stays below it too
GEN_SEED, GEN_COUNT = "ether/generated/0", 2400
MIN_PER_OUTCOME = 8
MIX_SEED = 5
HW, SRC, OTHER = ev.HW, ev.SRC, ev.OTHER
WORDS = (0, 1, 46, 1499, 1500, 1501, 1535, 1536, 0x07FF, 0x0800, 0x0801, 0x0805, 0x0806, 0x0807, 0x86DC, 0x86DD, 0x86DE,
         0xFFFF)
RECEIVED = (0, 1, 13, 14, 22, 23, 59, 60, 61, 63, 64, 65, 1514, 1518, 1522, 9018, 65535)
SNAP_OK = bytes.fromhex("aaaa03000000")

# configuration bits of Ref802x_Cfg(): IPv4, IPv6, multicast receive, ARP, error counters, DBG checks
CFG_WANT = {"v4v6": 0x1F, "v4v6_O0": 0x1F, "v4": 0x1D, "v4nomcast": 0x19}


def head_of(name, n, dst=HW, src=SRC, tl=0x0800, llc=None, snap_type=None, first=0x45):
    """The first min(n, 64) octets of a frame: shake_256 filler with the named fields stored over it."""
    f = bytearray(refvec.shake("ether/head/" + name, ev.HEAD))
    f[0:6], f[6:12], f[12:14] = dst, src, struct.pack("!H", tl & 0xFFFF)
    if llc is not None:
        f[14:20] = llc
        f[20:22] = struct.pack("!H", 0x0800 if snap_type is None else snap_type)
        f[22] = first
    else:
        f[14] = first
    return bytes(f[:min(n, ev.HEAD)])


def explicit_cases(mix_rows):
    cases, seen = [], set()

    def add(name, n, head):
        assert name not in seen and len(head) == min(n, ev.HEAD), name
        seen.add(name)
        cases.append({"name": name, "n": n, "head": bytes(head).hex()})

    def e2(name, n=100, **kw):
        add(name, n, head_of(name, n, **kw))

    def snap(name, n=100, length=None, llc=SNAP_OK, **kw):
        tl = (n - 18) & 0xFFFF if length is None else length
        add(name, n, head_of(name, n, tl=tl, llc=llc, **kw))

    for name, f in mix_rows:                                    # the rows of the two mixes, as built
        add(name, len(f), f[:ev.HEAD])
    # octets received
    for n in RECEIVED:
        e2(f"received {n}: e2 v4", n)
        snap(f"received {n}: snap v4, length field min(n - 18, 1500)", n, length=min((n - 18) & 0xFFFF, 1500))
        snap(f"received {n}: snap v4, length field 0", n, length=0)
    # the type / length word: at 60 octets (no length check), at 64, and where the word is the right length
    for w in WORDS:
        snap(f"word {w:#06x} at 60 received", 60, length=w)
        snap(f"word {w:#06x} at 64 received", 64, length=w)
        if w <= 1500 and w + 18 > 64:
            snap(f"word {w:#06x} at {w + 18} received", w + 18, length=w)
        add(f"word {w:#06x} at 100 received, v6 behind", 100, head_of(f"word6 {w}", 100, tl=w, first=0x60))
    # the 802.3 length field around received - 18
    for n in (63, 64, 65, 1518):
        for d in (-1, 0, 1):
            snap(f"length field received - 18 {d:+d} at {n} received", n, length=n - 18 + d)
    # every single bit of the LLC / SNAP octets
    for k in range(14, 20):
        for b in range(8):
            llc = bytearray(SNAP_OK)
            llc[k - 14] ^= 1 << b
            snap(f"octet {k} bit {b} flipped", llc=bytes(llc))
            snap(f"octet {k} bit {b} flipped, 60 received", 60, length=7, llc=bytes(llc))
    # SNAP types
    for w in WORDS:
        snap(f"snap type {w:#06x}", snap_type=w, first=0x60 if w == 0x86DD else 0x45)
    # destination address
    for k in range(6):
        for m in (0x02, 0x80):
            d = bytearray(HW)
            d[k] ^= m
            e2(f"dst differs in octet {k} by {m:#04x}", dst=bytes(d))
            snap(f"dst differs in octet {k} by {m:#04x}: snap", dst=bytes(d))
    for nm, d in (("all ones", ev.BCAST), ("all ones but the last bit", b"\xff" * 5 + b"\xfe"),
                  ("all ones but the group bit", b"\xfe" + b"\xff" * 5), ("hw with the group bit", bytes([HW[0] | 1]) + HW[1:]),
                  ("ipv4 group", ev.MCAST), ("ipv6 group", bytes.fromhex("333300000001")), ("group bit alone", b"\x01" + bytes(5)),
                  ("all zero", bytes(6)), ("hw", HW)):
        e2(f"dst {nm}: e2 v4", dst=d)
        e2(f"dst {nm}: e2 v6", dst=d, tl=0x86DD, first=0x60)
        snap(f"dst {nm}: snap arp", dst=d, snap_type=0x0806)
    # source address
    for nm, s in (("all zero", bytes(6)), ("all ones", ev.BCAST)):
        e2(f"src {nm}", src=s)
        snap(f"src {nm}: snap", src=s)
        for k in range(6):
            x = bytearray(s)
            x[k] ^= 0x01
            e2(f"src {nm} but octet {k}", src=bytes(x))
    e2("src the interface's own address", src=HW)
    e2("src a group address", src=ev.MCAST)
    # two checks failing at once, for each adjacent pair in the reference's order of checks
    e2("pair: received 59 + dst other", 59, dst=OTHER)
    e2("pair: received 59 + dst other + src null + bad type", 59, dst=OTHER, src=bytes(6), tl=0x8100)
    e2("pair: dst other + src null", dst=OTHER, src=bytes(6))
    e2("pair: dst other + src all ones", dst=OTHER, src=ev.BCAST)
    e2("pair: src null + bad type", src=bytes(6), tl=0x8100)
    snap("pair: src all ones + length field", src=ev.BCAST, length=83)
    e2("pair: dst other + bad type", dst=OTHER, tl=0x8100)
    snap("pair: length field + dsap", length=83, llc=bytes.fromhex("ab aa 03 00 00 00"))
    snap("pair: dsap + ssap", llc=bytes.fromhex("ab ab 03 00 00 00"))
    snap("pair: ssap + ctrl", llc=bytes.fromhex("aa ab 13 00 00 00"))
    snap("pair: ctrl + code[0]", llc=bytes.fromhex("aa aa 13 01 00 00"))
    snap("pair: code[0] + code[1]", llc=bytes.fromhex("aa aa 03 01 01 00"))
    snap("pair: code[1] + code[2]", llc=bytes.fromhex("aa aa 03 00 01 01"))
    snap("pair: code[2] + snap type", llc=bytes.fromhex("aa aa 03 00 00 01"), snap_type=0x8100)
    snap("pair: length field + snap type", length=81, snap_type=0x8100)
    snap("pair: everything after the length field", length=83, llc=bytes.fromhex("00 00 00 01 01 01"), snap_type=0)
    return cases


# rows whose outcome can be stated without any code: name -> (what ran or the check that failed, IF_HdrLen);
# "v6": NetIPv6_Rx where IPv6 is built, the invalid-type error of that header form where it is not
NAMED = {
    "received 59": ("size", 0), "received 0": ("size", 0), "received 60": ("NetIPv4_Rx", 14),
    "e2 v4 tcp": ("NetIPv4_Rx", 14), "snap v4 tcp": ("NetIPv4_Rx", 22), "e2 arp": ("NetARP_Rx", 14), "snap arp": ("NetARP_Rx", 22),
    "e2 v6 tcp": ("v6", 14), "snap v6 tcp": ("v6", 22),
    "snap len+1": ("NET_IF_ERR_INVALID_LEN_FRAME", 0), "snap len-1": ("NET_IF_ERR_INVALID_LEN_FRAME", 0),
    "snap len+1 dsap": ("NET_IF_ERR_INVALID_LEN_FRAME", 0), "snap dsap": ("NET_IF_ERR_INVALID_LLC_DSAP", 0),
    "snap ssap": ("NET_IF_ERR_INVALID_LLC_SSAP", 0), "snap ctrl": ("NET_IF_ERR_INVALID_LLC_CTRL", 0),
    "snap code[0]": ("NET_IF_ERR_INVALID_SNAP_CODE", 0), "snap code[2]": ("NET_IF_ERR_INVALID_SNAP_CODE", 0),
    "snap type": ("NET_IF_ERR_INVALID_SNAP_TYPE", 0), "e2 type 0x8100": ("NET_IF_ERR_INVALID_ETHER_TYPE", 0),
    "e2 type 0x05dd": ("NET_IF_ERR_INVALID_ETHER_TYPE", 0), "snap dsap+ssap": ("NET_IF_ERR_INVALID_LLC_DSAP", 0),
    "dst other v4": ("NET_IF_ERR_INVALID_ADDR_DEST", 0), "dst bcast v4": ("NetIPv4_Rx", 14),
    "src null": ("NET_IF_ERR_INVALID_ADDR_SRC", 0), "src bcast": ("NET_IF_ERR_INVALID_ADDR_SRC", 0),
    "src almost null": ("NetIPv4_Rx", 14), "dst other + src null": ("NET_IF_ERR_INVALID_ADDR_DEST", 0),
    "src bcast + bad type": ("NET_IF_ERR_INVALID_ADDR_SRC", 0), "src null + snap dsap": ("NET_IF_ERR_INVALID_ADDR_SRC", 0),
    "pair: received 59 + dst other": ("size", 0), "pair: dsap + ssap": ("NET_IF_ERR_INVALID_LLC_DSAP", 0),
    "pair: code[2] + snap type": ("NET_IF_ERR_INVALID_SNAP_CODE", 0),
    "pair: length field + dsap": ("NET_IF_ERR_INVALID_LEN_FRAME", 0),
    "length field received - 18 +0 at 64 received": ("NetIPv4_Rx", 22),
    "length field received - 18 +1 at 64 received": ("NET_IF_ERR_INVALID_LEN_FRAME", 0),
    "length field received - 18 +1 at 63 received": ("NetIPv4_Rx", 22),
}
NAMED_MCAST = {"dst mcast v4": ("NetIPv4_Rx", 14)}              # ... with multicast receive; else the destination error


def what_of(rec):
    """'size', the stub's name, or the error the buffer was discarded with: a reading of the record for
    the named rows and the coverage count (the tests have their own table)."""
    if rec["stub"] != "none":
        return rec["stub"]
    assert rec["discards"] == 1 and rec["err"] == "NET_ERR_RX", rec
    return "size" if rec["err_discard"] == "NET_ERR_NONE" else rec["err_discard"]


def check_named(lib, names, recs):
    v6, mcast = lib == "v4v6", lib != "v4nomcast"
    by_name = dict(zip(names, recs))
    for name, (what, hdr) in list(NAMED.items()) + list(NAMED_MCAST.items()):
        rec = by_name[name]
        if what == "v6" and not v6:
            what, hdr = ("NET_IF_ERR_INVALID_ETHER_TYPE" if hdr == 14 else "NET_IF_ERR_INVALID_SNAP_TYPE"), 0
        elif what == "v6":
            what = "NetIPv6_Rx"
        if name in NAMED_MCAST and not mcast:
            what, hdr = "NET_IF_ERR_INVALID_ADDR_DEST", 0
        assert (what_of(rec), rec["if_hdr_len"]) == (what, hdr), (lib, name, rec)


def check_coverage(lib, recs):
    count = collections.Counter((what_of(r), r["if_hdr_len"]) for r in recs)
    want = {("size", 0), ("NetARP_Rx", 14), ("NetARP_Rx", 22), ("NetIPv4_Rx", 14), ("NetIPv4_Rx", 22)}
    want |= {(e, 0) for e in ("NET_IF_ERR_INVALID_ADDR_DEST", "NET_IF_ERR_INVALID_ADDR_SRC", "NET_IF_ERR_INVALID_LEN_FRAME",
                              "NET_IF_ERR_INVALID_ETHER_TYPE", "NET_IF_ERR_INVALID_LLC_DSAP", "NET_IF_ERR_INVALID_LLC_SSAP",
                              "NET_IF_ERR_INVALID_LLC_CTRL", "NET_IF_ERR_INVALID_SNAP_CODE", "NET_IF_ERR_INVALID_SNAP_TYPE")}
    if lib == "v4v6":
        want |= {("NetIPv6_Rx", 14), ("NetIPv6_Rx", 22)}
    assert set(count) == want, (lib, set(count) ^ want)
    assert min(count.values()) >= MIN_PER_OUTCOME, (lib, count)
    return count


def mix_rows_now():
    import ether_frames as ef
    rows = [(nm, f) for nm, f in ef.frame_mix(random.Random(MIX_SEED))]
    rows += [("fixed1514: " + nm, f) for nm, f in ef.fixed_len_mix(random.Random(MIX_SEED))]
    return rows


def generate(committed=None):
    libs = {k: ev.Ref802x(k) for k in ev.LIB_FILES}
    for k, L in libs.items():
        assert L.cfg == CFG_WANT[k], (k, hex(L.cfg))
        assert L.errs == libs["v4v6"].errs and L.ctr_names == libs["v4v6"].ctr_names
    if committed is None:
        rows = mix_rows_now()
    else:                                                       # --check: the mix rows' octets as recorded
        n_mix = committed["mix_rows"]
        rows = [(c["name"], ev.case_frame(c)) for c in committed["cases"][:n_mix]]
        try:
            now = mix_rows_now()
            if [(nm, len(f), f[:ev.HEAD]) for nm, f in now] != [(nm, len(f), f[:ev.HEAD]) for nm, f in rows]:
                print("note: ether_frames' mixes built with this Python's random module differ from the recorded rows")
        except Exception as e:                                  # (the mixes need the package; the check does not)
            print(f"note: ether_frames' mixes not rebuilt ({e})")
    cases = explicit_cases(rows)
    names = [c["name"] for c in cases]
    frames = [ev.case_frame(c) for c in cases]
    for (nm, f), fr in zip(rows, frames):
        assert len(f) == len(fr) and f[:ev.HEAD] == fr[:ev.HEAD], nm
    gen = ev.gen_frames(GEN_SEED, GEN_COUNT)
    names += [f"generated[{i}]" for i in range(GEN_COUNT)]
    frames += gen

    table, out, calls, coverage = [], {}, 0, {}
    for lib in ev.LIBS:
        ix, dl, recs = [], [], []
        for nm, f in zip(names, frames):
            rec, d = libs[lib].rx(f)
            calls += 1
            if lib == "v4v6":
                calls += 1
                if libs["v4v6_O0"].rx(f) != (rec, d):
                    raise AssertionError(f"{nm}: -O2 gives {rec, d}, -O0 gives {libs['v4v6_O0'].rx(f)}")
            if rec not in table:
                table.append(rec)
            ix.append(table.index(rec)), dl.append(d), recs.append(rec)
        check_named(lib, names, recs)
        coverage[lib] = {f"{w}/{h}": c for (w, h), c in sorted(check_coverage(lib, recs).items())}
        out[lib] = {"cfg": libs[lib].cfg, "outcome": refvec.base64.b64encode(np.array(ix, np.uint8).tobytes()).decode(),
                    "data_len": refvec.pack(np.array(dl, np.uint16)), "upper": None}
    assert len(table) < 256
    doc = {
        "generator": "tests/golden/make_ether_vectors.py",
        "source": "what NetIF_802x_Rx of the reference's IF/net_if_802x.c (V3.06.01) did with each frame, behind the recording "
                  "stubs of oracle/ref/glue_802x.c, built by oracle/Makefile `ref`: LP64 little-endian; libraries v4v6 (IPv4 + "
                  "IPv6), v4 (template configuration), v4nomcast (IPv4, multicast off); -O0 and -O2 builds of v4v6 agree on every "
                  "case. err_discard is *p_err when the buffer was discarded (NET_ERR_NONE, the start value, for a frame "
                  "rejected by size); 'upper' is reserved for what real upper layers return once they replace the stubs",
        "hw": HW.hex(), "errs": libs["v4v6"].errs, "ctr_names": libs["v4v6"].ctr_names, "stubs": list(ev.STUBS),
        "mix_rows": len(rows), "mix_seed": MIX_SEED, "cases": cases,
        "generated": {"seed": GEN_SEED, "count": GEN_COUNT, "sha256": ev.frames_sha256(gen)},
        "outcomes": table, "out": out, "coverage": coverage, "reference_calls": calls,
    }
    return json.dumps(doc, separators=(",", ":")) + "\n"


def main():
    if not ev.libs_available():
        sys.exit("oracle/_ref/lib802x_ref_*.so are missing: `make -C oracle` with a reference tree builds them")
    check = "--check" in sys.argv[1:]
    committed = None
    if check:
        with open(ev.FIXTURE) as f:
            have = f.read()
        committed = json.loads(have)
    text = generate(committed)
    assert len(text.encode()) <= MAX_BYTES, len(text.encode())
    if check:
        if have != text:
            sys.exit("tests/golden/reference_ether_vectors.json differs from what the reference libraries give now")
        print(f"check ok: {len(text.encode())} bytes reproduce")
        return
    with open(ev.FIXTURE, "w") as f:
        f.write(text)
    doc = json.loads(text)
    print(f"wrote {ev.FIXTURE}: {len(text.encode())} bytes, {len(doc['cases'])} explicit cases ({doc['mix_rows']} mix rows), "
          f"{GEN_COUNT} generated, {len(doc['outcomes'])} distinct outcomes, {doc['reference_calls']} reference calls")
    for lib, c in doc["coverage"].items():
        print(" ", lib, c)


if __name__ == "__main__":
    main()
