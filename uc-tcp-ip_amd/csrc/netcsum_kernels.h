// netcsum_kernels.h — internal interface between the C ABI (netcsum_abi.hip) and the kernels: the
// argument blocks several kernel files share, then each kernel file's declarations in a section of its
// own. A launcher that reads a launch option takes the caller's KernelTune (netcsum_tune.h) first.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "netcsum_tune.h"

namespace netcsum {

// ---- argument blocks shared by several kernel files

struct SegBatchArgs {
    const uint8_t*  base;          // strided: first segment; varlen: base of the offsets
    const uint64_t* seg_off;       // varlen only (nullptr => strided)
    const uint16_t* seg_len_v;     // varlen only
    uint64_t        seg_stride;    // strided only
    uint32_t        seg_len;       // strided only
    const uint8_t*  pseudo;        // nullptr => no pseudo-header
    uint32_t        pseudo_stride;
    uint32_t        pseudo_len;
    uint32_t        n_seg;
    uint32_t        verify;        // 0: u16 checksum out, 1: u8 DEF_OK/DEF_FAIL out
    uint32_t        tile;          // 0: grid-stride; J > 0: block b owns segments [b*gpb*J, (b+1)*gpb*J)
    void*           out;
    uint32_t        touch;         // run-stream kernels: row-touch prologue (set by the launcher)
    uint32_t        xcd;           // stream kernels: XCD-aware block order (set by the launcher)
    const uint32_t* run_dev;       // varlen stream kernel: run length chosen on the device (used when
                                   // larger than the launch's), nullptr = the launch's
    uint32_t*       plan_out;      // varlen live kernel: the batch's plan for the next batch on the same
    uint32_t        plan_tag;      // descriptors (an extra sampler block), nullptr = none
    uint32_t        gather;        // dense stream kernel: a block's results gathered in LDS and stored as
                                   // one line by its last wave (set by the launcher)
    const uint32_t* n_dev;         // chain pass 1 (live kernel, CH): the segment count on the device
                                   // (chain_first[n]); n_seg is then the records' capacity
};

struct LaunchCfg {
    int  grid;             // workgroups; <= 0: fill the chip exactly (resident blocks x CUs x grid_mult)
    int  grid_mult;        // residency multiple used when grid <= 0
    int  cus;              // compute units of the device
    uint64_t blocks_needed;  // upper bound: one group per segment
    int  block;            // threads per workgroup (multiple of 64)
    int  group_lanes;      // lanes per segment: 1, 4, 8, 16, 32, 64
    int  chunks_per_pass;  // 16-B chunks per lane per pass: 1..4
    bool nt;               // non-temporal segment loads
    int  kernel;           // 1: seg_batch_kernel (one segment in flight per group), 2: seg_pipe_kernel,
                           // 3: seg_lds_kernel, 4: seg_tile_kernel (strided only),
                           // 5: seg_small_kernel (small 4-B-aligned strided segments, no pseudo),
                           // 6: seg_stream_kernel (dense strided runs, one wave per run),
                           // 7: seg_hdr_kernel (small headers through LDS-image tiles)
                           // 8: seg_hdrstream_kernel (packed 16 / 20-B headers, one wave per run)
    int  tile;             // segments per group per block in tile mode (0 = grid-stride)
    int  tile_pieces;      // v4: KiB of LDS image per stage (P)
    uint32_t stream_spw;   // kernel 6: segments per wave (one contiguous run each)
    uint32_t run_bytes;    // kernel 6, varlen: runs of about this many bytes, sized on the device from
                           // sampled lengths (stream_spw is then the shortest run the grid allows)
};

struct PktBatchArgs {
    const uint8_t*  base;          // packet i starts at base + off[i] (varlen) or base + i*stride
    const uint64_t* off;           // nullptr => strided
    const uint16_t* len;           // varlen: bytes of packet i present in the buffer
    uint64_t        stride;
    uint32_t        len_u;         // strided: bytes present per packet
    uint32_t        n;
    uint8_t*        flags_out;     // NETCSUM_PKT_* per packet (optional for Tx)
    uint32_t        tile;          // segments (packets) per group per block tile (0 = grid-stride)
    uint32_t        udp_tx_csum;   // Tx UDP checksums: 1 = compute, 0 = transmit none (write 0), 2 = per
                                   // datagram: a field of 0 is left 0 (no checksum), any other computed
    uint32_t        touch;         // run-stream form: row-touch prologue (set by the launcher)
    uint8_t*        action_out;    // Rx: NETCSUM_RX_* action per packet (optional; rx_action)
    uint32_t        rx_cfg;        // Rx: NETCSUM_RXCFG_* bits for the actions
    uint32_t*       defer_word;    // IPv6 / mixed: set to defer_tag by a batch kernel that leaves a
    uint32_t        defer_tag;     // datagram EXT_HDR; the walk pass runs only when it holds the tag
    uint32_t        xcd;           // run-stream form: XCD-aware block order (set by the launcher)
    union {                        // (one slot: the kernels' argument block keeps its size)
    uint32_t*       fieldpos_out;  // Tx (optional): per packet, which checksum fields were written —
                                   // kFieldIP | kFieldL4 | transport field offset (host-memory forms)
    uint32_t*       sums_out;      // Rx, mixed batches (RxBurstSums; the SUMS instantiations): per packet
                                   // one NETCSUM_FRAG_SUM as a little-endian dword, sum | len << 16 — a
                                   // fragment's payload sum and length, 0 for every other packet
    };
    uint32_t        plan;          // run-stream strided form, the next batch's plan (pkt_plan_block):
                                   // bits 0-7 the whole-span run (0: form 0 not allowed, gaps > 64 B),
                                   // bits 8-15 the longest live-piece run allowed (the bitmap's reach,
                                   // the batch size), bits 16-30 the host's tag for the ring
    uint32_t*       plan_out;      // optional: an extra block samples the batch and stores 1 << 31 |
                                   // tag << 16 | run << 8 | waves << 4 | form here (coherent host
                                   // memory); offset/length batches: bits 0-7 of `plan` unused
    uint32_t        res_waves;     // launcher: waves per SIMD to keep resident (3..8; 0: as many as fit)
    uint32_t*       vl_list;       // offset/length runs not in address order within the reach: the
    uint32_t*       vl_ctr;        // stream kernel appends their indices (vl_ctr[0]: count, by atomic
                                   // add) and the deferred pass (pkt_vl_deferred_kernel) does them, then
                                   // leaves vl_ctr[0..1] zero; nullptr: done inline
    uint32_t        vl_wide;       // launcher: the deferred pass's grid, wide (1) or 8 blocks (0)
};
// sums_out while a datagram waits for the walk pass (lane-group form: an IPv6 fragment whose Fragment
// header lies past the group's window): no record has len 0 and sum != 0
constexpr uint32_t kFragSumWalk = 1u;
constexpr uint32_t kFieldIP = 1u << 31;    // fieldpos_out: the IPv4 header checksum field (+10) written
constexpr uint32_t kFieldL4 = 1u << 30;    // fieldpos_out: the transport field at (bits 0-15) written

// Tx UDP checksum policy of a datagram whose checksum field holds `field` (PktBatchArgs::udp_tx_csum).
__host__ __device__ __forceinline__ bool udp_tx_compute(uint32_t mode, uint32_t field) {
    return mode == 1u || (mode == 2u && field != 0u);
}

// Two-pass Tx (run-stream form): one record per packet between the checksum pass and the scatter pass,
// written and read as ONE little-endian uint64 (vals | l4_off << 32 | flags << 48 | store << 56).
struct PktTxRecord {
    uint32_t vals;         // IP checksum | transport checksum << 16 (host order)
    uint16_t l4_off;       // packet offset of the transport checksum field
    uint8_t  flags;        // NETCSUM_PKT_* verdict
    uint8_t  store;        // bit 0: write the IP field, bit 1: write the transport field
};

struct ChainBatchArgs {
    const uint8_t*  base;          // piece j starts at base + off[j]
    const uint64_t* off;
    const uint16_t* len;
    const uint32_t* first;         // chain i = pieces [first[i], first[i+1])
    const uint8_t*  pseudo;        // nullptr => no pseudo-header
    uint32_t        pseudo_stride;
    uint32_t        pseudo_len;
    uint32_t        n;
    uint32_t        verify;
    void*           out;
    uint32_t        xcd;           // pass 1: XCD-aware tile order (set by the launcher)
};

// ---- netcsum_kernels.hip: the lane-group segment kernels, the dispatch of a segment batch, the probes
bool tile_supported(int g, int p, int k);   // is (G, P, K) a compiled v4 instantiation
const char* last_launch();                  // description of this thread's last batch launch
void set_last_launch(const char* desc);
hipError_t launch_seg_batch(const KernelTune& k, const SegBatchArgs& a, const LaunchCfg& c, hipStream_t s);
hipError_t launch_stream_exact(const void* d_p, uint32_t n16, unsigned long long* d_sum, int grid,
                               hipStream_t s, uint32_t tag = 0u);   // tag != 0 (grid 1): completion word
hipError_t launch_fill(void* d_buf, uint64_t n_bytes, uint64_t first_byte, uint64_t seed, int pattern, int grid,
                       hipStream_t s);
hipError_t launch_read_stream(const void* d_p, uint64_t n16, unsigned long long* d_sink, int grid, bool nt,
                              hipStream_t s, int variant);

// ---- netcsum_small.hip
bool small_supported(const SegBatchArgs& a);  // strided, no pseudo, 1..64 B, base/stride 4-B aligned
hipError_t launch_small_batch(const SegBatchArgs& a, int grid, hipStream_t s);

// ---- netcsum_hdr.hip
bool hdr_supported(const SegBatchArgs& a);     // small_supported and stride <= 64: LDS-image header tiles
int hdr_lanes_h(const SegBatchArgs& a, int h);  // headers per lane kernel 7 uses for a request (auto: h <= 0)
uint32_t hdr_pieces(const SegBatchArgs& a, int h);   // 1-KiB LDS-DMA pieces per tile of 64*h headers
int hdr_occupancy(const SegBatchArgs& a, int stages, int h);
hipError_t launch_hdr_batch(const SegBatchArgs& a, int stages, int h, int grid, hipStream_t s);

// ---- netcsum_hdrstream.hip
bool hdrstream_supported(const SegBatchArgs& a);                  // kernel 8: packed 16 / 20-B headers
hipError_t launch_hdrstream(const KernelTune& k, const SegBatchArgs& a, int depth, uint32_t spw, bool nt, hipStream_t s);

// ---- netcsum_stream.hip
bool stream_supported(const SegBatchArgs& a);  // strided, stride in [len, len+64], len >= 256
bool stream_dense(const SegBatchArgs& a);      // strided, stride == len >= 1024: the default for kernel 6
uint32_t stream_spw(const SegBatchArgs& a, uint64_t waves);
int stream_occupancy(int depth, const SegBatchArgs& a, bool nt);   // resident 256-thread blocks per CU
hipError_t launch_stream_batch(const KernelTune& k, const SegBatchArgs& a, int depth, uint32_t spw, bool nt, hipStream_t s);
// Varlen run length from sampled lengths: *out = clamp(run_bytes / (mean length + extra), spw_min, 128);
// with plan_out, also the batch's plan there: 1 << 31 | tag << 16 | form (0 the stream kernel; 1 / 2
// the lane-group pipe at 16 x 6 / 8 x 8, for sparse pools; 3 the live-sector stream, run << 8, bit 2
// depth 8).
hipError_t launch_varlen_runlen(const uint64_t* offs, const uint16_t* lens, uint32_t n, uint32_t extra, uint32_t run_bytes,
                                uint32_t spw_min, uint32_t* out, uint32_t* plan_out, uint32_t tag, hipStream_t s);
// Segments one per pool buffer (plan 3): the live-sector stream (netcsum_stream.hip
// seg_live_varlen_kernel), runs of spw <= 64 segments, depth 4 or 8 pieces in flight; a.plan_out:
// one extra block samples the descriptors for the next batch's plan.
hipError_t launch_live_varlen(const KernelTune& k, const SegBatchArgs& a, int depth, uint32_t spw, hipStream_t s);
constexpr uint32_t kVarlenSpwMin = 3u;
// Chain pass 1 in the live-sector segment stream (seg_live_varlen_kernel<…, CH>): runs of spw (<= 64)
// consecutive pieces, depth (4 / 8) pieces in flight, compacted sectors when cmp; each piece's exact
// half-word sum (u32, absolute LE frame) into rec[j]. (With the combine pass over those records:
// launch_chain_two_pass_h, netcsum_chains.hip.)
hipError_t launch_chain_live_records(const KernelTune& k, const ChainBatchArgs& c, uint32_t* rec, uint32_t cap, int depth,
                                     uint32_t spw, bool cmp, hipStream_t s);
hipError_t launch_read_run(const KernelTune& k, const void* d_p, uint64_t n_bytes, unsigned long long* d_sink, hipStream_t s,
                           bool sleep);

// ---- netcsum_chains.hip
hipError_t launch_chain_batch(const ChainBatchArgs& a, int group, int grid, hipStream_t s);
// Two-pass form (default): per-piece even/odd sums into `eo` (cap records), then a combine pass per
// chain; batches of more than `cap` pieces fall back to the wave-per-chain form inside pass 2.
// live_spw != 0: pass 1 in the live-sector stream, runs of live_spw (<= 64) consecutive pieces,
// live_depth (4 / 8) pieces in flight.
hipError_t launch_chain_two_pass(const KernelTune& k, const ChainBatchArgs& a, uint64_t* eo, uint32_t cap, int cus, hipStream_t s,
                                 uint32_t live_spw = 0u, int live_depth = 8);
// launch_chain_live_records (netcsum_stream.hip), then the combine pass over its records
// (chain_combine_h_kernel); combine_lanes: 16 or 64 lanes per chain in the combine pass
hipError_t launch_chain_two_pass_h(const KernelTune& k, const ChainBatchArgs& a, uint32_t* rec, uint32_t cap, int cus,
                                   hipStream_t s, uint32_t spw, int depth, bool cmp, int combine_lanes);

// ---- netcsum_crc.hip: CRC-32 batches (net_util.c:485-636)
struct CrcBatchArgs {
    const uint8_t*  base;          // segment i at base + off[i] (varlen) or base + i * stride
    const uint64_t* off;           // nullptr => strided
    const uint32_t* lens;          // varlen lengths (nullptr => all `len`)
    uint64_t        stride;
    uint32_t        len;
    uint32_t        n;
    uint32_t        cpl;           // 0: NetUtil_32BitCRC_Calc, 1: NetUtil_32BitCRC_CalcCpl
    uint32_t*       out;
    uint32_t        xs[4];         // strided: x^(8 s 2^k) mod P of the 16-lane combine (set by the launcher)
    uint32_t        xl;            // strided: x^(8 len) mod P
};
constexpr uint32_t kCrcShortMax = 96u;     // strided segments up to this length: one lane each
hipError_t launch_crc_batch(const KernelTune& k, const CrcBatchArgs& a, uint32_t max_len, int cus, hipStream_t s);
const char* crc_launch_name(const KernelTune& k, uint32_t max_len, bool varlen);

// ---- netcsum_packets.hip
hipError_t launch_pkt_batch(const PktBatchArgs& a, const LaunchCfg& c, bool tx, int ip_ver,  // 4, 6, 0 = per packet
                            hipStream_t s);

// ---- netcsum_pktstream.hip
// One 8-B record per packet of a host-memory Tx batch (pkt_field_gather_kernel): the written field
// values as they lie in memory (IP | transport << 16), the transport offset << 32, and the
// kFieldIP / kFieldL4 bits << 32 (bits 62 / 63).
hipError_t launch_pkt_field_gather(const PktBatchArgs& a, uint64_t* rec_out, hipStream_t s);
bool pkt_stream_supported(const PktBatchArgs& a, int ip_ver, int bound);   // run-stream packet kernel's domain
// bound (NETCSUM_TUNE_PKT_BOUND): 0 every piece of the run's span, 1 / 2 / 3 the live pieces, with 0 / 1
// / depth pieces loaded during the parse (netcsum_pktstream.hip; depth 8: bounds 0, 2 and 3)
// rec: two-pass Tx (records + scatter); scatter = false: the records only (zero-copy host bursts, whose
// host applies them)
hipError_t launch_pkt_stream(const KernelTune& k, const PktBatchArgs& a, int ip_ver, int depth, uint32_t spw, bool nt, bool tx,
                             int bound, hipStream_t s, PktTxRecord* rec = nullptr, bool scatter = true);
// The ring plan's sampler alone (one block; a.plan, a.plan_out and the batch's descriptors / stride as
// for the batch): the plan word for the batch about to be launched, which the host waits for.
hipError_t launch_pkt_plan(const PktBatchArgs& a, int ip_ver, hipStream_t s);
// Test-only fault (NETCSUM_TUNE_FAULT_INJECT 1): the calling thread's next offset/length packet batch
// with a deferred pass enqueues its stream kernel, skips the deferred pass and fails with
// hipErrorLaunchFailure — the state a failed deferred launch leaves (the list counters not reset).
void set_fault_skip_deferred(bool on);
// Zero-copy host bursts: one wave copies n result bytes (flags, and actions if act != nullptr) from
// device memory into coherent pinned host memory, then stores `tag` into *word (system scope).
hipError_t launch_burst_done(const uint8_t* fl, const uint8_t* act, uint32_t n, uint8_t* h_fl, uint8_t* h_act,
                             unsigned long long* word, uint32_t tag, hipStream_t s);

// Resident burst server (NETCSUM_TUNE_BURST_ZERO_COPY 3; netcsum_pktstream.hip burst_server_kernel):
// the host posts a zero-copy burst as ONE 64-B line of coherent host memory, which the server's
// leader waves poll, instead of launching a kernel per burst.
// Live-piece runs (run-stream packet kernels, bounds 1-3) span at most 63 KiB from their first 128-B
// line: piece 63 is never live, and its bit is the pop's sentinel.
constexpr uint32_t kLiveReach = 63u << 10;

struct alignas(64) BurstPost {
    uint64_t seq;          // burst number, increasing; kBurstStop: exit
    uint64_t ring;         // device address of the ring (its pinned alias)
    uint32_t stride;       // strided forms
    uint32_t n;            // frames (<= 4096)
    uint32_t pkt_len;      // strided forms: bytes present per slot
    uint32_t spw;          // frames per wave run
    uint32_t form;         // bit 0 Tx; form >> 1: kBurstWhole / kBurstLive / kBurstOffLen, or kBurstEther
                           // with kBurstEtherOff / kBurstEtherLen for the descriptors that are staged;
                           // kBurstSums (Rx): one NETCSUM_FRAG_SUM per frame as well
    uint32_t udp_mode;     // Tx: PktBatchArgs::udp_tx_csum
    uint32_t rx_cfg;       // Rx: NETCSUM_RXCFG_* for the actions
    uint32_t check;        // burst_post_check of every other field: a read that tore the line fails it
    uint32_t eth_cfg;      // kBurstEther: the demux's configuration, as EtherDemuxArgs names it (below);
    uint32_t have_hw;      // 0 in every other post
    uint32_t hw_lo;
    uint32_t hw_hi;
};
static_assert(sizeof(BurstPost) == 64, "one line");
constexpr uint64_t kBurstStop = ~0ull;
constexpr uint32_t kBurstWhole = 0u, kBurstLive = 1u, kBurstOffLen = 2u;
// Bursts of whole Ethernet frames (RxBurstEtherHost; with bit 0 of the form, Tx: TxBurstEtherHost, the Tx
// rule and one PktTxRecord per frame): the wave that owns a run classifies its frames
// (netcsum_etherhead.h) and streams their datagrams from descriptors it keeps in registers. Frame starts
// are off[i] with kBurstEtherOff, else i * stride; received lengths len[i] with kBurstEtherLen, else pkt_len.
constexpr uint32_t kBurstEther = 3u, kBurstKindMask = 3u, kBurstEtherOff = 4u, kBurstEtherLen = 8u;
// Rx bursts with fragment payload sums (RxBurstSumsHost, RxBurstEtherSumsHost): a bit of the form beside
// the kind (the line has no spare dword; the check covers it with the form), posted only to the server's
// SUMS instantiation, whose waves run the SUMS forms of the same runs and store one record per frame
// (BurstServerSumsArgs::sums) beside its flag and action.
constexpr uint32_t kBurstSums = 16u;
constexpr int kBurstServerMaxBlocks = 16;
__host__ __device__ __forceinline__ uint32_t burst_post_check(const BurstPost& p) {
    const uint32_t d[15] = {(uint32_t)p.seq, (uint32_t)(p.seq >> 32), (uint32_t)p.ring, (uint32_t)(p.ring >> 32),
                            p.stride, p.n, p.pkt_len, p.spw, p.form, p.udp_mode, p.rx_cfg,
                            p.eth_cfg, p.have_hw, p.hw_lo, p.hw_hi};
    uint32_t h = 0x811C9DC5u;                               // FNV-1a over the dwords
    for (int i = 0; i < 15; ++i) h = (h ^ d[i]) * 0x01000193u;
    return h;
}
struct BurstServerArgs {
    const BurstPost*    post;      // device alias of the post line
    unsigned long long* closed;    // [blocks]: set by a block that stops serving (device-written)
    uint8_t*            flags;     // Rx results (device aliases of coherent host memory)
    uint8_t*            act;
    uint8_t*            l2;        // kBurstEther: the frames' NETCSUM_L2_* classes
    PktTxRecord*        rec;       // Tx records
    const uint64_t*     off;       // offset/length descriptors (staged in coherent host memory)
    const uint16_t*     len;
    uint64_t            seq0;      // the last burst number already served
    uint64_t            idle_ticks;   // wall-clock ticks without a post after which a block stops
    uint64_t            life_ticks;   // wall-clock ticks after the block's start after which it stops
                                      // even while bursts keep coming (bounds how long the server holds
                                      // the hardware queue its stream shares with other streams)
};
// The SUMS instantiation's arguments (a type of its own: the other instantiation's argument block, which
// it keeps in scratch for the leader's wait, stays as it was).
struct BurstServerSumsArgs : BurstServerArgs {
    uint32_t*           sums;      // kBurstSums: the frames' NETCSUM_FRAG_SUM records, sum | len << 16
};
// blocks x 256 threads on stream s (a stream of its own: the kernel runs until it is idle). sums (the
// records' device alias) non-null: the instantiation that also serves kBurstSums posts. A thread's server
// is the other one until the thread first asks for sums: that one's code and resources are those of a
// server without the feature.
hipError_t launch_burst_server(const BurstServerArgs& a, int blocks, hipStream_t s, uint32_t* sums = nullptr);

// ---- netcsum_v6walk.hip
// IPv6 extension-header chains past the batch kernels' window (flags EXT_HDR): walked to the end and
// finished in place (netcsum_v6walk.hip); a.flags_out holds the batch kernel's flags.
hipError_t launch_pkt_v6_walk(const PktBatchArgs& a, bool tx, int cus, hipStream_t s);

// ---- netcsum_ether.hip
// The 802.x demux ahead of an Rx burst of Ethernet frames (netcsum_ether.hip ether_demux_kernel; the
// rules: include/netcsum_ether.h): per frame its layer-2 class and the offset/length descriptor of the IP
// datagram the packet batch is to check ({frame start, 0} for a frame that carries none).
struct EtherDemuxArgs {
    const uint8_t*  base;
    const uint64_t* off;        // frame starts, or nullptr: i * stride
    const uint16_t* len;        // octets received per frame, or nullptr: len_u
    uint64_t        stride;
    uint32_t        len_u;
    uint32_t        n;
    uint32_t        eth_cfg;    // NETCSUM_ETHCFG_*
    uint32_t        have_hw;    // 0: promiscuous
    uint32_t        hw_lo;      // the interface's address: octets 0-3, little-endian
    uint32_t        hw_hi;      // octets 4-5
    uint8_t*        l2_out;     // [n] NETCSUM_L2_*
    uint64_t*       off_out;    // [n] descriptors for the packet batch
    uint16_t*       len_out;    // [n]
};
constexpr uint32_t kEtherDemuxBlock = 256u;
inline uint32_t ether_demux_blocks(uint32_t n) { return (n + kEtherDemuxBlock - 1u) / kEtherDemuxBlock; }
hipError_t launch_ether_demux(const EtherDemuxArgs& a, hipStream_t s);
// The demux ahead of a Tx burst of Ethernet frames (ether_tx_demux_kernel, NetCsum_L2TxClass): the same
// arguments and outputs; eth_cfg and the interface's address are not looked at.
hipError_t launch_ether_tx_demux(const EtherDemuxArgs& a, hipStream_t s);

}  // namespace netcsum
