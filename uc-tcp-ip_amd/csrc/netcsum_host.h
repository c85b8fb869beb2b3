// netcsum_host.h — internal declarations of the batch ABI's host layer, shared by its translation
// units: netcsum_policy.hip (launch policy: which kernel form, geometry and run length a batch gets —
// decisions only, no launches), netcsum_abi.hip (argument checks, tuning, scratch and plans, the
// device-resident entry points) and netcsum_hostmem.hip (host contexts, the one copy-pipeline driver and
// the slot layout and issue step each ...Host form gives it, zero-copy bursts and the burst server, the
// host-memory entry points). What that file decides without a device — chunk plans, slot layouts,
// descriptor staging, the Tx record appliers — is netcsum_hostplan.h, free of HIP. The kernels' own
// interface is netcsum_kernels.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/netcsum_mi355x.h"
#include "netcsum_kernels.h"

namespace nchost {

constexpr int kMaxDev = 64;

// There is no CPU fallback: a failed HIP call is reported on stderr (the first 8 per process) and the
// caller gets NET_UTIL_ERR_MI355X_DEV.
NET_ERR dev_fail(const char* what, hipError_t e);

#define NC_HIP(call)                                    \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return nchost::dev_fail(#call, e_); \
    } while (0)

int cu_count(int dev);                                  // compute units of the device (cached)

// The calling thread's launch options (NetUtil_MI355X_Tune, NetUtil_MI355X_PlanBind): one value per host
// thread, so one thread's tuning never changes another thread's launches; a new thread starts from
// these defaults. Only NetUtil_MI355X_Tune / _PlanBind store to it: every policy function takes it by
// const reference, and every launcher that reads an option takes its KernelTune part (netcsum_tune.h)
// the same way, so what a launch depends on can be read off its signature.
struct Tune : netcsum::KernelTune {
    int grid = 0;
    int group = 0;
    int nt = -1;                    // -1: auto (nt when groups share no chunks)
    int block = 256;
    int chain_combine = -1;         // NETCSUM_TUNE_CHAIN_COMBINE
    int kernel = 0;                 // 0 = auto (5 when small_supported, else 2)
    int chunks = 0;
    int probe = 1;                  // LDS-DMA read probe by default
    int grid_mult = 1;
    int tile = -1;                  // -1: auto (4 segments per group per block tile)
    int burst_zc = 3;               // host bursts: pinned rings read in place by the resident server
    int burst_idle = 500;           // resident burst server: idle microseconds before it stops
    int burst_life = 1000;          // resident burst server: microseconds of residency per launch
    int pkt_bound = -1;             // run-stream packets: -1 auto, 0..3, 4 ring plans
    int tx_passes = 0;              // run-stream Tx: 0 auto (2 passes), 1, 2
    // NETCSUM_TUNE_PLAN_AHEAD: -1 auto (a batch whose plan has no word yet samples its layout first, in a
    // one-block launch the host waits for, from kPlanAheadRing frames / kPlanAheadPool segments), 0 never
    // (the first batch runs unplanned and leaves the plan for the next), 1 always.
    int plan_ahead = -1;
    // NetUtil_MI355X_PlanBind: the caller's identity for the layout its next batches carry (0: none, the
    // plans are keyed on the batch's addresses alone). Part of every plan key, so two layouts placed at the
    // same addresses under different ids keep a plan each and never run in the other's form.
    uint32_t plan_id = 0;
};

const Tune& tune();                                    // the calling thread's (netcsum_abi.hip)
void host_release();                                    // frees the calling thread's host contexts (netcsum_hostmem.hip)

// ---- segment batches (act: netcsum_abi.hip)
NET_ERR check_op(NETCSUM_OP op, const void* d_pseudo, CPU_INT16U pseudo_len);
netcsum::SegBatchArgs seg_args(const void* base, const uint64_t* seg_off, const uint16_t* seg_len_v, uint64_t seg_stride,
                               uint32_t seg_len, const void* pseudo, uint32_t pseudo_stride, uint32_t pseudo_len,
                               uint32_t n_seg, NETCSUM_OP op, void* out);
NET_ERR launch_batch(const Tune& t, const netcsum::SegBatchArgs& a0, uint32_t len_hint, hipStream_t s);
netcsum::LaunchCfg choose_cfg(const Tune& t, int dev, const netcsum::SegBatchArgs& a, uint32_t len_hint);

// ---- packet batches
// One packet batch on device-visible memory, as its entry point (a public wrapper, a chunk of a
// host-memory batch, a zero-copy burst) hands it to pkt_batch.
struct PktJob {
    const void*           base = nullptr;
    const uint64_t*       off = nullptr;       // offset/length form (with len), else strided
    const uint16_t*       len = nullptr;
    uint64_t              stride = 0;
    CPU_INT16U            pkt_len = 0;
    uint32_t              n = 0;
    uint8_t*              flags = nullptr;
    uint32_t              udp_mode = 1u;       // PktBatchArgs::udp_tx_csum (Tx)
    bool                  tx = false;
    int                   ip_ver = 0;          // 4, 6, or 0: per packet by the version nibble
    hipStream_t           stream = nullptr;
    uint8_t*              action = nullptr;    // Rx: the burst actions (optional), under rx_cfg
    uint32_t              rx_cfg = 0u;
    NETCSUM_FRAG_SUM*     sums = nullptr;      // Rx, mixed (RxBurstSums): per-frame fragment payload sums
    uint32_t*             fieldpos = nullptr;  // Tx: which fields each packet had written (the host-memory
                                               // forms' records, optional)
    netcsum::PktTxRecord* rec_only = nullptr;  // zero-copy Tx burst: the records alone, no scatter pass
    int                   bound_pref = -1;     // a burst read in place from host memory: its preferred form
};

// What pkt_decide chose for a PktJob; the ring's plan (netcsum_abi.hip pkt_ring_plan) may replace the
// form and run length, pkt_settle then fits the run to the live-piece reach and names the launch.
struct PktPlan {
    netcsum::PktBatchArgs a{};
    netcsum::LaunchCfg    c{};                 // the lane-group kernel's geometry
    bool                  stream = false;      // the run-stream form (netcsum_pktstream.hip), else lane groups
    bool                  walk = false, own_flags = false;
    int                   d = 4, bound = 0;    // pieces in flight; which bytes of each slot are read
    uint32_t              spw = 0u;            // datagrams per wave run
    bool                  snt = true, two = false;
    bool                  bound_default = true, dense = false;
    bool                  plan_ring = false;   // the batch takes (and leaves) a ring plan
    uint32_t              run0 = 0u;           // the whole-span form's run, where the plan may choose it
    uint64_t              cap = 0u;            // the longest run a plan may ask for
    bool                  vl_wide = true;      // the deferred pass's grid: wide unless the plan found the
    bool                  vl_inline = false;   // ring's descriptors in order; a dense ring in order: the
                                               // inline form (pkt_stream_kernel DEF)
    const char*           plan_note = "";
    const char*           ahead_note = "";
    char                  desc[208];
};

// NET_UTIL_ERR_MI355X_INVALID_ARG for a stride the lane-group stores cannot address, else the plan.
NET_ERR pkt_decide(const Tune& t, const PktJob& j, PktPlan& p);
void pkt_settle(const Tune& t, const PktJob& j, PktPlan& p);
// (act: netcsum_abi.hip) the job of the arguments the packet entry points share, and its launches
PktJob pkt_job(const void* base, const uint64_t* off, const uint16_t* len, uint64_t stride, CPU_INT16U pkt_len, uint32_t n,
               uint8_t* flags, void* hip_stream);
NET_ERR pkt_batch(const Tune& t, const PktJob& j);

// ---- Ether bursts
// The argument checks the four Rx Ether entry points share (device and host memory, with and without
// fragment sums), each returning the first failing code in the entry points' order: check_rx_ether, then —
// for a sums form — check_frag_sums, then n_frame 0 succeeds, then n_frame > 0x7FFFFFFF is invalid.
NET_ERR check_rx_ether(const void* base, const uint8_t* action, const uint8_t* l2, uint32_t n_frame, uint32_t rx_cfg,
                       uint32_t eth_cfg);
NET_ERR check_frag_sums(const NETCSUM_FRAG_SUM* sums, uint32_t n_frame);

// The interface's six address octets as the demux kernel and the burst post carry them (hw_addr nullptr:
// promiscuous, everything left 0): octets 0-3 and 4-5, little-endian.
inline void pack_hw_addr(const uint8_t* hw_addr, uint32_t* have_hw, uint32_t* hw_lo, uint32_t* hw_hi) {
    if (hw_addr == nullptr) return;
    *have_hw = 1u;
    *hw_lo = (uint32_t)hw_addr[0] | ((uint32_t)hw_addr[1] << 8) | ((uint32_t)hw_addr[2] << 16) | ((uint32_t)hw_addr[3] << 24);
    *hw_hi = (uint32_t)hw_addr[4] | ((uint32_t)hw_addr[5] << 8);
}

// TxBurstEther on device-visible memory (netcsum_abi.hip): the public entry point, and — with d_fieldpos
// (zeroed by the caller) and d_rec — a chunk of the host-memory form, whose written fields come back as
// one 8-B record per frame (launch_pkt_field_gather over the datagrams' descriptors: positions count
// from frame + 14).
NET_ERR tx_burst_ether(const Tune& t, void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                       CPU_INT16U frame_len, uint32_t n_frame, uint8_t* d_flags, uint8_t* d_l2, hipStream_t hs,
                       uint32_t* d_fieldpos, uint64_t* d_rec);

// 16 blocks x 4 waves: a block's leader polls the post line (16 64-B reads per poll round); 4 blocks
// of 16 waves were slower from 10 frames up (tools/burst_latency.c, 64 frames 14.8 us against 13.1 us
// for a launch per burst: 16 waves on one CU queue their PCIe reads)
constexpr int kServerBlocks = 16;

// The resident burst server's form for a burst (BurstPost::form >> 1 and its run length), or false
// when the burst is outside the run-stream kernel's domain (the launch path takes it).
bool server_form(const uint64_t* h_off, uint64_t stride, CPU_INT16U pkt_len, uint32_t n_pkt, uint32_t* form, uint32_t* spw);
// Its run length for the offset/length form, which the Ether form (BurstPost::form kBurstEther) shares.
uint32_t server_run(uint32_t n_pkt);

}  // namespace nchost
