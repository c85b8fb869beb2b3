"""The launchers' one dispatch idiom and the kernel families' tables on the CPU
(uc-tcp-ip_amd/csrc/netcsum_dispatch.h, netcsum_tables.h). tests/c_dispatch/dispatch_caller.cpp, a
stand-alone program, includes the two headers as plain C++17 — nothing from HIP —, is built here with
-fsanitize=address,undefined -Wall -Wextra -Werror and run as a subprocess (nothing is loaded into Python).
Its callables return the constants they were handed; it exits non-zero at the first difference:

helper   Of: over -70..69 exactly the listed values select themselves, every other value reports no match.
         Or: listed values select themselves, every other the stated fallback. Flag hands over bools.
         Four axes at once: all constants arrive in the order given, one unlisted Of value misses the pick,
         the callable runs once. Tuples: exactly the listed tuples select themselves (no per-axis match),
         unsigned run-time values and bool members included.
tables   the real tables against their sets written out as literals from the code before the tables
         existed: the tile form's 16 (G, P, K), the header tile's 45 (P, S, H) and its stage rule, the packet
         stream's 10 (D, BND, VL), the packet kernel's 7 (G, K), the depth lists 4/6/8, 4/8 and 8-else-4.
"""
import os
import subprocess

import pytest

import netcsum

REPO = netcsum.REPO
CSRC = os.path.join(REPO, "uc-tcp-ip_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dispatch") / "dispatch_caller_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-I" + CSRC,
           os.path.join(REPO, "tests", "c_dispatch", "dispatch_caller.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize("part,at_least", [("helper", 10000), ("tables", 8000)])
def test_dispatch(exe, part, at_least):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, part], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    word, checks = r.stdout.split()
    assert word == "ok" and int(checks) >= at_least                  # (the checks ran: none was compiled away)


def test_the_headers_include_nothing_from_hip():
    for name in ("netcsum_dispatch.h", "netcsum_tables.h"):
        src = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in src and "netcsum_kernels.h" not in src and "netcsum_host.h" not in src


def test_no_define_builds_an_instantiation_list():
    """No macro in a kernel file's launcher end: the .hip files define none at all."""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(".hip"):
            src = open(os.path.join(CSRC, name)).read()
            assert "#define" not in src, name
