"""The kernel files' launch options on the CPU (uc-tcp-ip_amd/csrc/netcsum_tune.h: netcsum::KernelTune
and the resolvers the launchers and the policy call): tests/c_tune/tune_caller.cpp, a stand-alone program
that includes that header alone, built here with -fsanitize=address,undefined -Wall -Wextra -Werror and
run as a subprocess (nothing is loaded into Python).

The cases: the default-constructed struct, and each of the thirteen options at each value of its accept
set in NetUtil_MI355X_Tune's table (netcsum_abi.hip kTuneRows; tests/golden/tune_accept.json is that
table as recorded) — a listed set whole, a range at its ends, 0 and 1. For every case the program prints
the fields and every resolver; the expectations below are the rules as the header's comments state them,
written out, so the defaults are pinned in one place: -1 "each kernel's default", except that -1 means ON
for LIVE_COMPACT and STORE_GATHER, 16384 B for VARLEN_RUN_BYTES, per-run results for HDR_BURST and 0
for CHAIN_GRID and TX_FLUSH; the CRC options default to 0, 0, 0 and CRC_WIDE to 1.
"""
import os
import subprocess

import pytest

import netcsum

REPO = netcsum.REPO

DEFAULTS = dict(stream_waves=-1, stream_touch=-1, stream_xcd=-1, tx_flush=-1, crc_kernel=0, crc_nt=0, crc_lanes=0,
                crc_wide=1, hdr_burst=-1, varlen_run_bytes=-1, live_compact=-1, store_gather=-1, chain_grid=-1)
ACCEPT = dict(stream_waves=[-1, 0, 3, 4, 5, 6, 7, 8], stream_touch=[-1, 0, 1], stream_xcd=[-1, 0, 1, 4096],
              tx_flush=[-1, 0, 1, 2, 3, 4], crc_kernel=[0, 1, 2, 3], crc_nt=[0, 1], crc_lanes=[0, 1, 2, 4, 8, 16],
              crc_wide=[0, 1, 2], hdr_burst=[-1, 0, 1], varlen_run_bytes=[-1, 0, 1, 1 << 20], live_compact=[-1, 0, 1],
              store_gather=[-1, 0, 1], chain_grid=[-1, 0, 1, 16])
# w workgroups of 4 waves per CU: the largest 512-B multiple of which w fit 160 KiB; outside 3..8 no cap
LDS_BYTES = {0: 0, 1: 0, 2: 0, 3: 54272, 4: 40960, 5: 32768, 6: 27136, 7: 23040, 8: 20480, 9: 0}


def expected(k):
    e = {name: k[name] for name in DEFAULTS}
    for auto in range(10):
        e[f"lds_bytes({auto})"] = LDS_BYTES[k["stream_waves"] if k["stream_waves"] >= 0 else auto]
    e["waves_tuned"] = int(k["stream_waves"] >= 0)
    for auto in (0, 1):
        e[f"touch({auto})"] = auto if k["stream_touch"] < 0 else int(k["stream_touch"] != 0)
        e[f"xcd({auto})"] = auto if k["stream_xcd"] < 0 else int(k["stream_xcd"] != 0)
    for auto in (0, 1, 256):
        e[f"xcd_mode({auto})"] = auto if k["stream_xcd"] < 0 else k["stream_xcd"]
    e["live_compact()"] = int(k["live_compact"] != 0)
    e["store_gather()"] = int(k["store_gather"] != 0)
    e["run_bytes()"] = 16384 if k["varlen_run_bytes"] < 0 else k["varlen_run_bytes"]
    e["hdr_burst()"] = 1 if k["hdr_burst"] < 0 else int(k["hdr_burst"] > 0)
    e["chain_grid()"] = max(k["chain_grid"], 0)
    e["tx_flush_mode()"] = max(k["tx_flush"], 0)
    return e


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tune") / "tune_caller_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-I" + os.path.join(REPO, "uc-tcp-ip_amd", "csrc"),
           os.path.join(REPO, "tests", "c_tune", "tune_caller.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(exe, cases):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input="".join(f"{n} {v}\n" for n, v in cases), capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    out = [{kv.split("=")[0]: int(kv.split("=")[1]) for kv in line.split()} for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def test_header_includes_no_hip():
    with open(os.path.join(REPO, "uc-tcp-ip_amd", "csrc", "netcsum_tune.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<stdint.h>"]


def test_defaults(exe):
    (got,) = run(exe, [("default", 0)])
    assert got == expected(DEFAULTS)
    # the rules at the defaults, as literals
    assert [got[f"lds_bytes({w})"] for w in (0, 3, 4, 5, 6, 7, 8)] == [0, 54272, 40960, 32768, 27136, 23040, 20480]
    assert (got["waves_tuned"], got["touch(0)"], got["touch(1)"], got["xcd(0)"], got["xcd(1)"]) == (0, 0, 1, 0, 1)
    assert (got["xcd_mode(0)"], got["xcd_mode(1)"], got["xcd_mode(256)"]) == (0, 1, 256)
    assert (got["live_compact()"], got["store_gather()"]) == (1, 1)            # -1 means on
    assert (got["run_bytes()"], got["hdr_burst()"], got["chain_grid()"], got["tx_flush_mode()"]) == (16384, 1, 0, 0)
    assert (got["crc_kernel"], got["crc_nt"], got["crc_lanes"], got["crc_wide"]) == (0, 0, 0, 1)


def test_every_option_at_every_accepted_value(exe):
    assert set(ACCEPT) == set(DEFAULTS) and len(ACCEPT) == 13
    cases = [(name, v) for name, vals in ACCEPT.items() for v in vals]
    for (name, v), got in zip(cases, run(exe, cases)):
        assert got == expected(dict(DEFAULTS, **{name: v})), (name, v)


def test_accept_sets_are_the_recorded_table_s():
    """ACCEPT above against tests/golden/tune_accept.json (the NET_ERR recorded per key and probed value): every
    value here is an accepted one, the smallest and the largest accepted are among them, and 0 and 1 where
    accepted."""
    import json
    with open(os.path.join(REPO, "tests", "golden", "tune_accept.json")) as f:
        rec = json.load(f)
    for name, vals in ACCEPT.items():
        key = getattr(netcsum, "TUNE_" + name.upper())
        ok = {v for v, e in zip(rec["values"], rec["err"][str(key)]) if e == netcsum.NET_UTIL_ERR_NONE}
        assert set(vals) <= ok, name
        assert (min(vals), max(vals)) == (min(ok), max(ok)), name
        assert ok & {0, 1} <= set(vals), name
        if len(ok) <= 8:                                           # a listed set, or a range this short: whole
            assert set(vals) == ok, name
