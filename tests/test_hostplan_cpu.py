"""The host-memory batches' planning on the CPU (uc-tcp-ip_amd/csrc/netcsum_hostplan.h: the chunk planner,
the slot layout, descriptor staging and the two Tx record appliers that netcsum_hostmem.hip's one pipeline
driver and its in-place bursts use). tests/c_hostplan/hostplan_caller.cpp, a stand-alone program, includes
the header as plain C++ — it includes nothing from HIP —, is built here with -fsanitize=address,undefined
-Wall -Wextra -Werror and run as a subprocess (nothing is loaded into Python). The program works out every
expected value itself, by brute force over the items or from literals, and exits non-zero at the first
difference:

plan     n in {1, 2, 7, 29} x n_chunks in {0, 1, 3, 7, 64} x the four descriptor shapes (neither, offsets
         and lengths, lengths only, offsets only with a fixed length; offsets out of order, one length 0):
         the chunks partition [0, n) in order, every chunk but the last has per = ceil(n / clamp(n_chunks))
         items, each [lo, hi) is the min / max over the chunk's items, the maximum is the largest span;
         staging rebases offsets to lo and copies lengths.
layout   regions 256-B aligned, in request order, disjoint, covered by the total; an empty region takes no
         room; for the five ...Host forms at per = 5, without and with their optional parts, the offsets
         equal the sums of al256() those forms spelled out by hand before, and the host slot is empty
         exactly for the forms that reuse a slot without a host wait.
records  four items of distinct octets, strided and by offsets, the datagram at +0 and at +14, store masks
         none / IP / transport / both and one EXT_HDR item: the buffer differs from the original in exactly
         the expected octets, the flags are the records', the EXT_HDR item is untouched and comes back in
         the skip list with its offset and length; the copy pipeline's gathered records likewise.
"""
import os
import subprocess

import pytest

import netcsum

REPO = netcsum.REPO


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostplan") / "hostplan_caller_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-I" + os.path.join(REPO, "include"),
           "-I" + os.path.join(REPO, "uc-tcp-ip_amd", "csrc"), os.path.join(REPO, "tests", "c_hostplan", "hostplan_caller.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize("part,at_least", [("plan", 400), ("layout", 100), ("records", 8000)])
def test_hostplan(exe, part, at_least):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, part], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    word, checks = r.stdout.split()
    assert word == "ok" and int(checks) >= at_least                  # (the checks ran: none was compiled away)


def test_the_header_includes_nothing_from_hip():
    src = open(os.path.join(REPO, "uc-tcp-ip_amd", "csrc", "netcsum_hostplan.h")).read()
    assert "#include <hip" not in src and "netcsum_kernels.h" not in src and "netcsum_host.h" not in src
