"""The launch decisions of the batch ABI stay what they were: every case of tools/launch_matrix.py —
segment, packet, chain, host-burst and CRC batches on each side of every threshold the host-side policy
has — leaves the NetUtil_MI355X_LastLaunch() string recorded in tests/golden/launch_names.json (kernel
form, run length, plan). The fixture was recorded once from a known-good library; a string that
differs is a changed launch decision, never a reason to re-record."""
import json
import os
import sys

import pytest

import netcsum

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(netcsum.REPO, "tools"))
import launch_matrix  # noqa: E402

with open(launch_matrix.GOLDEN_NAMES) as _f:
    GOLDEN = json.load(_f)
CASES = launch_matrix.cases()


@pytest.fixture(scope="module")
def matrix():
    m = launch_matrix.Matrix()
    yield m
    del m
    torch.cuda.empty_cache()


def test_fixture_covers_the_matrix():
    assert sorted(GOLDEN) == sorted(c["id"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_launch_name(matrix, case):
    assert matrix.run(case) == GOLDEN[case["id"]]
