// netcsum_tune.h — the launch options the kernel files' launchers read (NetUtil_MI355X_Tune), and the
// rules that resolve them. No HIP: a launcher takes these by const reference from its caller, the host
// layer keeps them in the calling thread's nchost::Tune (netcsum_host.h), and a plain C++ program can
// include this file alone.
#pragma once

#include <stdint.h>

namespace netcsum {

struct KernelTune {
    // NETCSUM_TUNE_STREAM_WAVES: residency cap of the run-stream kernels, w waves per SIMD (3..8); 0 no
    // cap; -1 each kernel's default
    int stream_waves = -1;
    // NETCSUM_TUNE_STREAM_TOUCH: row-touch prologue of the run-stream kernels: -1 each kernel's default,
    // 0 off, 1 on
    int stream_touch = -1;
    // NETCSUM_TUNE_STREAM_XCD: XCD-aware block order of the segment / varlen / header stream kernels: -1
    // each kernel's default, 0 off, 1 on (C >= 2: chunks of C blocks, stream_xcd_mode). Measured
    // (profiles/r2w_*, r2x_*): C5 shard 3.614 -> 3.561 ms, C2 0.2186 -> 0.2181, C4 0.6777 -> 0.6747 (on);
    // C3 0.0579-0.0584 -> 0.0589 (off).
    int stream_xcd = -1;
    // NETCSUM_TUNE_TX_FLUSH: Tx finalize write-back of the dirty field lines: -1 / 0 none, 1 scatter
    // stores at system scope, 2 release at the end of every scatter wave, 3 / 4 a write-back launch of
    // 8 / 256 workgroups after the Tx launch(es)
    int tx_flush = -1;
    int crc_kernel = 0;             // NETCSUM_TUNE_CRC_KERNEL (netcsum_mi355x.h)
    int crc_nt = 0;                 // NETCSUM_TUNE_CRC_NT: non-temporal chunk loads (interleaved form)
    int crc_lanes = 0;              // NETCSUM_TUNE_CRC_LANES: interleaved lanes per segment, 0 auto
    int crc_wide = 1;               // NETCSUM_TUNE_CRC_WIDE: 0 byte, 1 11-bit, 2 lane-replicated 6-bit tables
    // NETCSUM_TUNE_HDR_BURST: header stream results written per run (1) or per piece (0); -1 default
    // (kHdrBurstDefault)
    int hdr_burst = -1;
    int varlen_run_bytes = -1;      // NETCSUM_TUNE_VARLEN_RUN_BYTES: -1 default (16384), 0 fixed runs of 8
    // NETCSUM_TUNE_LIVE_COMPACT: the live-sector streams read their live sectors compacted, 16 per
    // wave-instruction (-1 default / 1), or as the live 1-KiB pieces of their span (0)
    int live_compact = -1;
    // NETCSUM_TUNE_STORE_GATHER: the dense segment stream kernel's results, per block of 4 runs, gathered
    // in LDS and stored whole by the block's last wave (-1 default / 1), or per wave (0)
    int store_gather = -1;
    // NETCSUM_TUNE_CHAIN_GRID: 0 / -1 chain pass 1 in tiles of 64 pieces, one per block; k >= 1 a grid of
    // k x the resident blocks, each owning an equal contiguous share of the pieces
    int chain_grid = -1;
};

// LDS bytes each 256-thread workgroup of a run-stream kernel reserves so that at most w of them (w waves
// per SIMD) fit a CU's 160 KiB: the largest 512-B multiple of which w fit and w + 1 do not; 0 = no cap.
// auto_waves: the kernel's default.
inline uint32_t stream_lds_bytes(const KernelTune& k, int auto_waves) {
    const int w = k.stream_waves >= 0 ? k.stream_waves : auto_waves;
    return (w >= 3 && w <= 8) ? ((163840u / (uint32_t)w) & ~511u) : 0u;
}
inline bool stream_waves_tuned(const KernelTune& k) { return k.stream_waves >= 0; }
inline bool stream_touch(const KernelTune& k, bool auto_on) { return k.stream_touch < 0 ? auto_on : k.stream_touch != 0; }
inline bool stream_xcd(const KernelTune& k, bool auto_on) { return k.stream_xcd < 0 ? auto_on : k.stream_xcd != 0; }
// the block-order mode for xcd_block (netcsum_stream.h): 0 dispatch order, 1 one slice per XCD, C >= 2
// chunks of C blocks per XCD in turn; auto_mode when the knob is at its default
inline uint32_t stream_xcd_mode(const KernelTune& k, uint32_t auto_mode) {
    return k.stream_xcd < 0 ? auto_mode : (uint32_t)k.stream_xcd;
}
inline bool live_compact(const KernelTune& k) { return k.live_compact != 0; }
inline bool store_gather(const KernelTune& k) { return k.store_gather != 0; }
constexpr uint32_t kVarlenRunBytes = 16384u;
inline uint32_t varlen_run_bytes(const KernelTune& k) {
    return k.varlen_run_bytes < 0 ? kVarlenRunBytes : (uint32_t)k.varlen_run_bytes;
}
constexpr bool kHdrBurstDefault = true;     // C3 0.0584 -> 0.0571-0.0575 ms (profiles/r2zi_c3_burst_sweep.jsonl)
inline bool hdr_burst(const KernelTune& k) { return k.hdr_burst < 0 ? kHdrBurstDefault : k.hdr_burst > 0; }
inline int chain_grid(const KernelTune& k) { return k.chain_grid < 0 ? 0 : k.chain_grid; }
inline int tx_flush_mode(const KernelTune& k) { return k.tx_flush < 0 ? 0 : k.tx_flush; }

}  // namespace netcsum
