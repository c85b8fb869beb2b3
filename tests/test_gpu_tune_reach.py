"""A launch option set through NetUtil_MI355X_Tune reaches the launcher that reads it.

Twelve of the thirteen options of netcsum::KernelTune (csrc/netcsum_tune.h) are set to non-default values,
with the results checked against the oracle, by the tests beside their kernels: STREAM_WAVES / _TOUCH /
_XCD and STORE_GATHER in test_gpu_parity.py (and _pktstream, _hdrstream, _chains), VARLEN_RUN_BYTES in
test_gpu_parity.py, HDR_BURST in test_gpu_hdrstream.py, TX_FLUSH in test_gpu_pktstream.py, CHAIN_GRID in
test_gpu_chains.py and the four CRC options in test_gpu_crc.py. LIVE_COMPACT has two readers: the chain
batches' one-record pass 1 (test_gpu_chains.py sets it) and the offset/length pool's live-sector stream
(launch_live_varlen), which no other test runs with it off. That reader is the case here.

Run in a thread of its own (options are per thread), so the main thread keeps its defaults.
"""
import threading

import numpy as np
import pytest

import netcsum
import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"


def _in_thread(fn):
    box = []

    def body():
        try:
            torch.cuda.set_device(0)
            fn()
        except BaseException as e:                                  # noqa: BLE001 (re-raised in the caller)
            box.append(e)
        finally:
            netcsum.thread_release()

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if box:
        raise box[0]


@pytest.mark.parametrize("compact", [0, 1])
def test_live_compact_reaches_the_pool_stream(compact):
    """300 segments of 20 / 556 / 1480 B, one per 2-KiB buffer at +84, random bytes between them, 12-B
    pseudo-headers: from the second batch on the same descriptors the plan runs them in the live-sector
    stream, whose sectors are read compacted (1) or as the live pieces of the span (0)."""
    rng = np.random.default_rng(300 + compact)
    n = 300 + compact                                               # (plans are keyed on addresses and the count)
    lens = np.array([20, 556, 1480])[rng.choice(3, size=n, p=[7 / 12, 4 / 12, 1 / 12])].astype(np.uint16)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(2048) + np.uint64(84)
    buf = rng.integers(0, 256, size=n * 2048 + 64, dtype=np.uint8)
    ph = rng.integers(0, 256, size=n * 12, dtype=np.uint8)
    want = {op: oracle.batch_varlen(buf, offs, lens, ph, 12, 12, op) for op in (netcsum.OP_DATA_CALC, netcsum.OP_DATA_VERIFY)}

    def body():
        netcsum.tune(netcsum.TUNE_LIVE_COMPACT, compact)
        b = torch.from_numpy(buf).to(DEV)
        o = torch.from_numpy(offs.view(np.int64)).to(DEV)
        ln = torch.from_numpy(lens.view(np.int16)).to(DEV)
        p = torch.from_numpy(ph).to(DEV)
        launches = []
        for op in (netcsum.OP_DATA_CALC, netcsum.OP_DATA_VERIFY, netcsum.OP_DATA_CALC):
            out = torch.zeros(n * (2 if op == netcsum.OP_DATA_CALC else 1), dtype=torch.uint8, device=DEV)
            netcsum.batch_varlen(b, o, ln, p, 12, 12, n, out, op)
            torch.cuda.synchronize()
            launches.append(netcsum.last_launch())
            got = out.cpu().numpy().view(np.uint16) if op == netcsum.OP_DATA_CALC else out.cpu().numpy()
            bad = np.nonzero(got != want[op])[0]
            assert bad.size == 0, (op, launches[-1], [(int(i), int(got[i]), int(want[op][i])) for i in bad[:6]])
        for last in launches[1:]:
            assert last.startswith("seg_live_varlen_kernel") and "plan=pool(live)" in last, launches

    _in_thread(body)
