// netcsum_hostmem.hip — the batch ABI's paths that start and end in host memory: the per-thread host
// context (one per host thread and device: its streams, pinned staging and device buffers), the
// drop-in's stream sum and CRC, the three-slot copy pipeline of the ...Host batches, the zero-copy
// bursts over a pinned ring and the resident burst server. Each is its device form (netcsum_abi.hip)
// run on a copy or an alias of the caller's memory.
//
// There is deliberately NO CPU fallback anywhere in this library: if the HIP runtime or device
// fails, the caller gets NET_UTIL_ERR_MI355X_DEV and a message on stderr.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/netcsum_ether.h"
#include "netcsum_device.h"
#include "netcsum_host.h"
#include "netcsum_hostplan.h"

using namespace nchost;

namespace {

constexpr size_t kZeroCopyMax = 16u * 1024u;      // streams up to 16 KiB: zero-copy single-block path

// ----------------------------------------------------------- per-thread host-path contexts
// One context per (host thread, device): its own stream, pinned staging, completion word and
// device buffers, so one host thread per device needs no lock (SURVEY §8(b) threading). The
// context is released when its thread exits (thread_local destructor) or on request
// (NetUtil_MI355X_ThreadRelease); a partially failed initialisation is rolled back.
struct HostCtx {
    bool                 ready = false;
    int                  dev = -1;
    hipStream_t          stream = nullptr;
    uint8_t*             h_stage = nullptr;   // pinned
    uint8_t*             d_stage = nullptr;
    size_t               cap = 0;
    unsigned long long*  d_sum = nullptr;
    unsigned long long*  h_sum = nullptr;     // pinned, mapped
    unsigned long long*  h_sum_dev = nullptr; // device alias of h_sum
    uint8_t*             h_stage_dev = nullptr;  // device alias of h_stage (zero-copy reads)
    uint32_t             seq = 0;                 // completion tags of the single-block launches
    // pipelined host batch
    hipStream_t          pstream[3] = {nullptr, nullptr, nullptr};
    uint8_t*             d_pipe[3] = {nullptr, nullptr, nullptr};
    size_t               pipe_cap = 0;
    uint8_t*             h_pipe[3] = {nullptr, nullptr, nullptr};   // pinned descriptor staging per slot
    size_t               hpipe_cap = 0;
    // zero-copy bursts (burst_zero_copy): device results, and coherent pinned memory holding the
    // completion word, the results the completion kernel copies out, and the burst's descriptors
    uint8_t*             d_burst = nullptr;
    uint8_t*             h_burst = nullptr;
    uint8_t*             h_burst_dev = nullptr;
    // resident burst server (TUNE_BURST_ZERO_COPY 3): its stream, whether it may be serving, the last
    // burst number posted
    hipStream_t          sstream = nullptr;
    bool                 server_live = false;
    bool                 want_sums = false;       // a sums burst was posted: every launch from then on is the
                                                  // server's SUMS instantiation (burst_server_run)
    uint64_t             post_seq = 0;

    bool empty() const {
        if (stream || h_stage || d_stage || d_sum || h_sum || d_burst || h_burst || sstream) return false;
        for (int j = 0; j < 3; ++j) {
            if (pstream[j] || d_pipe[j] || h_pipe[j]) return false;
        }
        return true;
    }
    // Frees everything this context holds (on its own device), leaving it reusable.
    void release() {
        if (empty()) {
            ready = false;
            return;
        }
        int cur = -1;
        const bool have_cur = hipGetDevice(&cur) == hipSuccess;
        if (dev >= 0) (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
        for (int j = 0; j < 3; ++j) {
            if (pstream[j]) (void)hipStreamSynchronize(pstream[j]);
        }
        (void)stop_server(0);                     // (no limit: the server reads h_burst, freed below)
        if (sstream) (void)hipStreamDestroy(sstream);
        if (stream) (void)hipStreamDestroy(stream);
        if (h_stage) (void)hipHostFree(h_stage);
        if (d_stage) (void)hipFree(d_stage);
        if (d_sum) (void)hipFree(d_sum);
        if (h_sum) (void)hipHostFree(h_sum);
        if (d_burst) (void)hipFree(d_burst);
        if (h_burst) (void)hipHostFree(h_burst);
        for (int j = 0; j < 3; ++j) {
            if (pstream[j]) (void)hipStreamDestroy(pstream[j]);
            if (d_pipe[j]) (void)hipFree(d_pipe[j]);
            if (h_pipe[j]) (void)hipHostFree(h_pipe[j]);
        }
        if (have_cur && cur != dev && cur >= 0) (void)hipSetDevice(cur);
        *this = HostCtx{};
    }
    ~HostCtx() { release(); }
    bool stop_server(int limit_ms);
};

thread_local HostCtx tls_ctx[kMaxDev];

NET_ERR host_ctx(HostCtx** out) {
    int dev = 0;
    NC_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDev) return dev_fail("device index", hipErrorInvalidDevice);
    HostCtx& c = tls_ctx[dev];
    if (!c.ready) {
        c.release();                               // roll back a previous partial initialisation
        c.dev = dev;
        hipError_t e = hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMalloc(&c.d_sum, 16);
        // coherent: the single-block kernel's system-scope completion store is visible while it runs
        if (e == hipSuccess) e = hipHostMalloc(&c.h_sum, 16, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&c.h_sum_dev), c.h_sum, 0);
        if (e != hipSuccess) {
            c.release();
            return dev_fail("host context init", e);
        }
        c.ready = true;
    }
    *out = &c;
    return NET_UTIL_ERR_NONE;
}

NET_ERR ensure_stage(HostCtx& c, size_t bytes) {
    if (bytes <= c.cap) return NET_UTIL_ERR_NONE;
    size_t cap = std::max<size_t>(bytes, 64u * 1024u);
    cap = (cap + 4095u) & ~(size_t)4095u;
    if (c.h_stage) { (void)hipHostFree(c.h_stage); c.h_stage = nullptr; }
    if (c.d_stage) { (void)hipFree(c.d_stage); c.d_stage = nullptr; }
    c.cap = 0;
    NC_HIP(hipHostMalloc(&c.h_stage, cap, hipHostMallocMapped));
    NC_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&c.h_stage_dev), c.h_stage, 0));
    NC_HIP(hipMalloc(&c.d_stage, cap));
    c.cap = cap;
    return NET_UTIL_ERR_NONE;
}

// The three pipeline slots of a host-memory batch: streams, device buffers of >= dev_bytes and pinned
// descriptor staging of >= host_bytes (grown on demand; the previous call has drained them).
NET_ERR ensure_pipe(HostCtx& c, size_t dev_bytes, size_t host_bytes) {
    for (int j = 0; j < 3; ++j) {
        if (!c.pstream[j]) NC_HIP(hipStreamCreateWithFlags(&c.pstream[j], hipStreamNonBlocking));
    }
    if (dev_bytes > c.pipe_cap) {
        for (int j = 0; j < 3; ++j) {
            if (c.d_pipe[j]) { (void)hipFree(c.d_pipe[j]); c.d_pipe[j] = nullptr; }
        }
        c.pipe_cap = 0;
        for (int j = 0; j < 3; ++j) NC_HIP(hipMalloc(&c.d_pipe[j], dev_bytes));
        c.pipe_cap = dev_bytes;
    }
    if (host_bytes > c.hpipe_cap) {
        for (int j = 0; j < 3; ++j) {
            if (c.h_pipe[j]) { (void)hipHostFree(c.h_pipe[j]); c.h_pipe[j] = nullptr; }
        }
        c.hpipe_cap = 0;
        for (int j = 0; j < 3; ++j) NC_HIP(hipHostMalloc(&c.h_pipe[j], host_bytes, 0));
        c.hpipe_cap = host_bytes;
    }
    return NET_UTIL_ERR_NONE;
}

// A host-memory batch that returns early (any error) first waits for its three pipeline streams, so
// no copy into the caller's memory is still in flight when the call returns. (A Tx batch that fails
// may leave the caller's buffer with some chunks finalized and others not.)
struct PipeDrainOnExit {
    HostCtx& c;
    bool     done = false;
    ~PipeDrainOnExit() {
        if (done) return;
        for (int j = 0; j < 3; ++j) {
            if (c.pstream[j]) (void)hipStreamSynchronize(c.pstream[j]);
        }
    }
};

static_assert(kRecFieldIP == netcsum::kFieldIP && kRecFieldL4 == netcsum::kFieldL4, "apply_field_records reads the gather's bits");

// ----------------------------------------------------------- the three-slot copy pipeline
// Every ...Host batch is its device form run over chunks (netcsum_hostplan.h plan_chunks) on the three
// pipeline streams of the calling thread's context: chunk k's bytes [lo, hi) go H2D into slot k mod 3
// (with its descriptors rebased to lo, staged in the slot's pinned memory), the device form runs on the
// copy and its results come D2H, while chunks k +- 1 copy and compute on the other streams. Host buffers
// should be pinned (hipHostMalloc / hipHostRegister) for the copies to overlap; the call returns when
// every output is in host memory.
struct PipeSlot {
    hipStream_t st;
    uint8_t*    d;      // the slot's device buffer (SlotLayout dev)
    uint8_t*    h;      // its pinned staging (SlotLayout host)
};

struct NoRetire { void operator()(const HostChunk&, const PipeSlot&) const {} };

// Runs the chunks through the slots. issue(chunk, slot) enqueues the chunk's H2D copies, memsets, launches
// and D2H copies on slot.st; retire(chunk, slot), where a form has one, runs on the host once that stream
// has finished the chunk (Tx: the returned records are applied to the caller's buffer).
// The one rule for reusing a slot: the device side of slot k mod 3 is reused in its stream's order, which
// needs no host wait; its pinned staging is written by the host, so a form that stages anything there, or
// retires, first waits for chunk k - 3 (synchronise, retire). At the end the last three chunks are
// waited for and retired in order — every stream in use then is idle.
template <class Issue, class Retire = NoRetire>
NET_ERR run_pipe(HostCtx& c, const ChunkPlan& plan, const SlotLayout& dev, const SlotLayout& host, Issue issue,
                 Retire retire = Retire{}) {
    const bool host_wait = host.total() != 0u || !std::is_same<Retire, NoRetire>::value;
    NET_ERR e = ensure_pipe(c, dev.total(), host.total());
    if (e != NET_UTIL_ERR_NONE) return e;
    PipeDrainOnExit guard{c};
    const size_t n = plan.ch.size();
    auto slot = [&](size_t k) { return PipeSlot{c.pstream[k % 3u], c.d_pipe[k % 3u], c.h_pipe[k % 3u]}; };
    auto finish = [&](size_t k) -> NET_ERR {                 // chunk k's stream has finished: retire it
        NC_HIP(hipStreamSynchronize(slot(k).st));
        retire(plan.ch[k], slot(k));
        return NET_UTIL_ERR_NONE;
    };
    for (size_t k = 0; k < n; ++k) {
        if (k >= 3 && host_wait) {                           // slot k mod 3's staging is free again
            e = finish(k - 3u);
            if (e != NET_UTIL_ERR_NONE) return e;
        }
        e = issue(plan.ch[k], slot(k));
        if (e != NET_UTIL_ERR_NONE) return e;
    }
    for (size_t k = n > 3 ? n - 3 : 0; k < n; ++k) {
        e = finish(k);
        if (e != NET_UTIL_ERR_NONE) return e;
    }
    guard.done = true;
    return NET_UTIL_ERR_NONE;
}

// A chunk's bytes [lo, hi) of the caller's buffer to the start of its slot.
NET_ERR copy_chunk_bytes(const void* h_base, const HostChunk& q, const PipeSlot& s) {
    if (q.hi > q.lo) {
        NC_HIP(hipMemcpyAsync(s.d, static_cast<const uint8_t*>(h_base) + q.lo, q.hi - q.lo, hipMemcpyHostToDevice, s.st));
    }
    return NET_UTIL_ERR_NONE;
}

// A chunk's descriptors, staged in the slot's pinned memory (stage_descriptors: offsets rebased to lo) and
// copied to the slot: where present, offsets at hs_off -> o_off and lengths at hs_len -> o_len.
NET_ERR copy_chunk_descriptors(const uint64_t* h_off, const uint16_t* h_len, const HostChunk& q, const PipeSlot& s,
                               size_t hs_off, size_t o_off, size_t hs_len, size_t o_len) {
    uint64_t* h_o = reinterpret_cast<uint64_t*>(s.h + hs_off);
    uint16_t* h_l = reinterpret_cast<uint16_t*>(s.h + hs_len);
    stage_descriptors(h_off, h_len, q, h_o, h_l);
    if (h_off) NC_HIP(hipMemcpyAsync(s.d + o_off, h_o, (size_t)q.ns * 8u, hipMemcpyHostToDevice, s.st));
    if (h_len) NC_HIP(hipMemcpyAsync(s.d + o_len, h_l, (size_t)q.ns * 2u, hipMemcpyHostToDevice, s.st));
    return NET_UTIL_ERR_NONE;
}

// A segment batch's pseudo-headers of items [s0, s0 + ns) to o_ph of the slot.
NET_ERR copy_chunk_pseudo(const void* h_pseudo, uint32_t pseudo_stride, uint32_t pseudo_len, const HostChunk& q,
                          const PipeSlot& s, size_t o_ph) {
    NC_HIP(hipMemcpyAsync(s.d + o_ph, static_cast<const uint8_t*>(h_pseudo) + (size_t)q.s0 * pseudo_stride,
                          (size_t)(q.ns - 1u) * pseudo_stride + pseudo_len, hipMemcpyHostToDevice, s.st));
    return NET_UTIL_ERR_NONE;
}

// Polls done() — a read of coherent pinned memory that a kernel on c.stream stores to — back to back
// instead of synchronising the stream (C1 and burst latency); every 1024 polls it looks at the clock,
// and after 2 s it falls back to the stream synchronisation, which reports a failed launch, and one
// last look: `what` names the failure when done() still does not hold.
template <class Done>
NET_ERR spin_until(HostCtx& c, const char* what, Done done) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0; !done(); ++spin) {
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            NC_HIP(hipStreamSynchronize(c.stream));
            return done() ? NET_UTIL_ERR_NONE : dev_fail(what, hipErrorUnknown);
        }
    }
    return NET_UTIL_ERR_NONE;
}

}  // namespace

void nchost::host_release() {
    for (int d = 0; d < kMaxDev; ++d) {
        tls_ctx[d].release();
    }
}

extern "C" {

NET_ERR NetUtil_MI355X_StreamSum32(const NETCSUM_SPAN* spans, uint32_t n_spans, uint32_t* p_sum32) {
    if (p_sum32 == nullptr || (spans == nullptr && n_spans != 0)) return NET_ERR_FAULT_NULL_PTR;
    HostCtx* cp = nullptr;
    NET_ERR e = host_ctx(&cp);                 // the device must exist even for an empty stream
    if (e != NET_UTIL_ERR_NONE) return e;
    HostCtx& c = *cp;
    size_t total = 0;
    for (uint32_t i = 0; i < n_spans; ++i) total += spans[i].len;
    *p_sum32 = 0u;
    if (total == 0) return NET_UTIL_ERR_NONE;
    const size_t padded = (total + 15u) & ~(size_t)15u;
    if (padded / 16u > 0xFFFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    e = ensure_stage(c, padded);
    if (e != NET_UTIL_ERR_NONE) return e;
    size_t pos = 0;
    for (uint32_t i = 0; i < n_spans; ++i) {
        if (spans[i].len) {
            std::memcpy(c.h_stage + pos, spans[i].p, spans[i].len);
            pos += spans[i].len;
        }
    }
    std::memset(c.h_stage + pos, 0, padded - pos);
    const uint32_t n16 = (uint32_t)(padded / 16u);
    if (padded <= kZeroCopyMax) {
        // one packet (the drop-in's common case): the kernel reads the pinned staging buffer over
        // the bus and stores its single-block total into pinned memory — one launch, one sync
        // the host polls the kernel's tagged completion word instead of synchronising the stream
        // (C1 latency); after 2 s without it, it falls back to the stream sync and its error check
        if (++c.seq == 0u) c.seq = 1u;
        const uint32_t tag = c.seq;
        volatile unsigned long long* w = c.h_sum;
        *w = 0ull;                             // no stale word (e.g. a multi-block sum) can carry the tag
        NC_HIP(netcsum::launch_stream_exact(c.h_stage_dev, n16, c.h_sum_dev, 1, c.stream, tag));
        unsigned long long v = 0ull;
        e = spin_until(c, "completion word", [&] { return (uint32_t)((v = *w) >> 32) == tag; });
        if (e == NET_UTIL_ERR_NONE) *p_sum32 = (uint32_t)v;
        return e;
    } else {
        const int grid = (int)std::min<uint32_t>(256u, (n16 + 1023u) / 1024u);
        NC_HIP(hipMemcpyAsync(c.d_stage, c.h_stage, padded, hipMemcpyHostToDevice, c.stream));
        NC_HIP(hipMemsetAsync(c.d_sum, 0, sizeof(unsigned long long), c.stream));
        NC_HIP(netcsum::launch_stream_exact(c.d_stage, n16, c.d_sum, std::max(grid, 2), c.stream));
        NC_HIP(hipMemcpyAsync(c.h_sum, c.d_sum, sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
        NC_HIP(hipStreamSynchronize(c.stream));
    }
    *p_sum32 = (uint32_t)(*(volatile unsigned long long*)c.h_sum);           // the reference's u32 accumulator wraps mod 2^32
    return NET_UTIL_ERR_NONE;
}

// One CRC-32 (the NetUtil_32BitCRC_Calc register value) of a host buffer: staged into this thread's
// pinned buffer, read from there by the kernel (zero-copy), result copied back.
NET_ERR NetUtil_MI355X_CRC32Host(const void* h_data, uint32_t len, uint32_t* p_crc) {
    if (p_crc == nullptr || (h_data == nullptr && len != 0)) return NET_ERR_FAULT_NULL_PTR;
    HostCtx* cp = nullptr;
    NET_ERR e = host_ctx(&cp);
    if (e != NET_UTIL_ERR_NONE) return e;
    HostCtx& c = *cp;
    *p_crc = 0u;
    if (len == 0) return NET_UTIL_ERR_NONE;
    e = ensure_stage(c, len);
    if (e != NET_UTIL_ERR_NONE) return e;
    std::memcpy(c.h_stage, h_data, len);
    netcsum::CrcBatchArgs a{};
    a.base = c.h_stage_dev;
    a.len = len;
    a.n = 1;
    a.out = reinterpret_cast<uint32_t*>(c.d_sum);
    NC_HIP(netcsum::launch_crc_batch(tune(), a, len, cu_count(c.dev), c.stream));
    NC_HIP(hipMemcpyAsync(c.h_sum, c.d_sum, sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
    NC_HIP(hipStreamSynchronize(c.stream));
    *p_crc = *reinterpret_cast<volatile uint32_t*>(c.h_sum);
    return NET_UTIL_ERR_NONE;
}

NET_ERR NetUtil_MI355X_ChkSumBatchStridedHost(const void* h_seg, uint64_t seg_stride, CPU_INT16U seg_len,
                                              const void* h_pseudo, uint32_t pseudo_stride, CPU_INT16U pseudo_len,
                                              uint32_t n_seg, void* h_out, NETCSUM_OP op, uint32_t n_chunks) {
    NET_ERR e = check_op(op, h_pseudo, pseudo_len);
    if (e != NET_UTIL_ERR_NONE) return e;
    if (n_seg == 0) return NET_UTIL_ERR_NONE;
    if (h_out == nullptr || (h_seg == nullptr && seg_len != 0)) return NET_ERR_FAULT_NULL_PTR;
    HostCtx* cp = nullptr;
    e = host_ctx(&cp);
    if (e != NET_UTIL_ERR_NONE) return e;
    HostCtx& c = *cp;
    const size_t out_elt = (op == NETCSUM_OP_DATA_VERIFY || op == NETCSUM_OP_HDR_VERIFY) ? 1u : 2u;
    const bool has_ph = (h_pseudo != nullptr && pseudo_len != 0);
    const ChunkPlan plan = plan_chunks(nullptr, nullptr, seg_stride, seg_len, n_seg, n_chunks);
    const uint32_t per = plan.per;
    // device slot: [segment bytes | pseudo-headers | outputs]; host slot: [] — nothing is staged on the host,
    // so a slot is reused in its stream's order, without a host wait
    SlotLayout dev, host;
    dev.take(plan.max_span);
    const size_t o_ph = dev.take(has_ph ? (size_t)(per - 1u) * pseudo_stride + pseudo_len : 0u);
    const size_t o_out = dev.take((size_t)per * out_elt);
    int dev_id = 0;
    NC_HIP(hipGetDevice(&dev_id));
    const Tune& t = tune();
    return run_pipe(c, plan, dev, host, [&](const HostChunk& q, const PipeSlot& s) -> NET_ERR {
        NET_ERR e = copy_chunk_bytes(h_seg, q, s);
        if (e == NET_UTIL_ERR_NONE && has_ph) e = copy_chunk_pseudo(h_pseudo, pseudo_stride, pseudo_len, q, s, o_ph);
        if (e != NET_UTIL_ERR_NONE) return e;
        const netcsum::SegBatchArgs a = seg_args(s.d, nullptr, nullptr, seg_stride, seg_len, has_ph ? s.d + o_ph : nullptr,
                                                 pseudo_stride, has_ph ? pseudo_len : 0u, q.ns, op, s.d + o_out);
        // Parity of each segment's start is derived in-kernel from the DEVICE address it reads,
        // so re-basing the chunk at a 256-B aligned device buffer is transparent.
        NC_HIP(netcsum::launch_seg_batch(t, a, choose_cfg(t, dev_id, a, seg_len), s.st));
        NC_HIP(hipMemcpyAsync(static_cast<uint8_t*>(h_out) + (size_t)q.s0 * out_elt, s.d + o_out, (size_t)q.ns * out_elt,
                              hipMemcpyDeviceToHost, s.st));
        return NET_UTIL_ERR_NONE;
    });
}

// ----------------------------------------------------------- host-memory batches (PCIe-inclusive)
// The path starts and ends in host memory (NIC Rx buffers, IF/net_if.c:6593; socket Tx buffers,
// Source/net_sock.c:5531). Each entry point below is a slot layout and an issue step for run_pipe (above).

NET_ERR NetUtil_MI355X_ChkSumBatchVarLenHost(const void* h_base, const uint64_t* h_seg_off, const uint16_t* h_seg_len,
                                             const void* h_pseudo, uint32_t pseudo_stride, CPU_INT16U pseudo_len,
                                             uint32_t n_seg, void* h_out, NETCSUM_OP op, uint32_t n_chunks) {
    NET_ERR e = check_op(op, h_pseudo, pseudo_len);
    if (e != NET_UTIL_ERR_NONE) return e;
    if (n_seg == 0) return NET_UTIL_ERR_NONE;
    if (n_seg > 0x7FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (h_out == nullptr || h_base == nullptr || h_seg_off == nullptr || h_seg_len == nullptr) return NET_ERR_FAULT_NULL_PTR;
    HostCtx* cp = nullptr;
    e = host_ctx(&cp);
    if (e != NET_UTIL_ERR_NONE) return e;
    HostCtx& c = *cp;
    const size_t elt = (op == NETCSUM_OP_DATA_VERIFY || op == NETCSUM_OP_HDR_VERIFY) ? 1u : 2u;
    const bool has_ph = h_pseudo != nullptr && pseudo_len != 0;
    const ChunkPlan plan = plan_chunks(h_seg_off, h_seg_len, 0, 0, n_seg, n_chunks);
    const uint32_t per = plan.per;
    // device slot: [bytes | offsets | lengths | pseudo-headers | outputs]; host slot: [offsets | lengths]
    SlotLayout dev, host;
    dev.take(plan.max_span);
    const size_t o_off = dev.take((size_t)per * 8u), o_len = dev.take((size_t)per * 2u);
    const size_t o_ph = dev.take(has_ph ? (size_t)(per - 1u) * pseudo_stride + pseudo_len : 0u);
    const size_t o_out = dev.take((size_t)per * elt);
    const size_t hs_off = host.take((size_t)per * 8u), hs_len = host.take((size_t)per * 2u);
    return run_pipe(c, plan, dev, host, [&](const HostChunk& q, const PipeSlot& s) -> NET_ERR {
        NET_ERR e = copy_chunk_bytes(h_base, q, s);
        if (e == NET_UTIL_ERR_NONE) e = copy_chunk_descriptors(h_seg_off, h_seg_len, q, s, hs_off, o_off, hs_len, o_len);
        if (e == NET_UTIL_ERR_NONE && has_ph) e = copy_chunk_pseudo(h_pseudo, pseudo_stride, pseudo_len, q, s, o_ph);
        if (e != NET_UTIL_ERR_NONE) return e;
        // (a segment's byte parity is taken from the device address it is read at, so the copy's new
        // alignment changes nothing)
        e = launch_batch(tune(),
                         seg_args(s.d, reinterpret_cast<const uint64_t*>(s.d + o_off),
                                  reinterpret_cast<const uint16_t*>(s.d + o_len), 0, 0, has_ph ? s.d + o_ph : nullptr,
                                  pseudo_stride, has_ph ? pseudo_len : 0u, q.ns, op, s.d + o_out),
                         0u, s.st);
        if (e != NET_UTIL_ERR_NONE) return e;
        NC_HIP(hipMemcpyAsync(static_cast<uint8_t*>(h_out) + (size_t)q.s0 * elt, s.d + o_out, (size_t)q.ns * elt,
                              hipMemcpyDeviceToHost, s.st));
        return NET_UTIL_ERR_NONE;
    });
}

// ---- zero-copy bursts (NetUtil_MI355X_RxBurstHost / RxValidateIPHost up to kBurstZC frames)
// A driver's burst is a few to a few hundred frames (the template's Rx ring holds 10 buffers,
// Cfg/Template/net_dev_cfg.c:147), so its cost is fixed, not bandwidth: an H2D copy, a launch, a D2H
// copy and a stream synchronisation took 19.3 us for one frame (profiles/r3x_burst_latency.jsonl).
// When the caller's ring is pinned (device-accessible host memory) the kernel reads it in place over
// PCIe, and its flags and actions (Tx: 8-B field records) go straight into coherent pinned memory that
// the host set to a sentinel no result can take (0xFF); the host polls them until every one has
// arrived — each is written once, so no completion protocol is needed — instead of synchronising a
// stream. By default (TUNE_BURST_ZERO_COPY 3) the kernel is this thread's resident burst server
// (burst_server_run below), which takes each burst from a posted line: no launch per burst.
// TUNE_BURST_ZERO_COPY 2: a launch per burst; 1: the results go to device memory and a one-wave
// completion kernel copies them into coherent memory, then stores a tagged completion word
// (system-scope release after the wave's own stores) that the host polls. tools/burst_latency.c zc,
// profiles/r4k_burst_zc.jsonl: 1 / 64 frames 6.9 / 11.2 us (3), 10.8 / 12.9 us (2), 12.7 / 15.1 us
// (1). A pageable ring takes the copy path.
constexpr uint32_t kBurstZC = 4096u;                    // frames
// Over PCIe a burst is latency-bound: the whole-slot stream (bound 0) issues the pieces with the
// parse's loads (one round trip) where the live-piece forms parse first (two); it applies to
// strided rings with gaps <= 64 B, the others keep the default (tools/burst_latency.c zc,
// profiles/r4k_burst_zc.jsonl: a launch per burst, 64 frames 12.9 us against 13.9 us in form 2)
constexpr int kBurstBound = 0;
constexpr uint64_t kBurstZCSpan = 64ull << 20;          // ring bytes the kernel may read in place
constexpr size_t kBurstWord = 0, kBurstPost = 64, kBurstClosed = 128, kBurstFlags = 256, kBurstAct = kBurstFlags + kBurstZC,
                 kBurstOff = kBurstAct + kBurstZC, kBurstLen = kBurstOff + 8u * kBurstZC,
                 kBurstRec = kBurstLen + 2u * kBurstZC, kBurstL2 = kBurstRec + 8u * kBurstZC,
                 kBurstSums = kBurstL2 + kBurstZC, kBurstHostBytes = kBurstSums + 4u * kBurstZC;
// (kBurstSums: one NETCSUM_FRAG_SUM per frame, sentinel 0xFFFFFFFF — no fragment payload has 65 535 octets:
// IPv4 at most 65 515, IPv6 at most 65 527 after the Fragment header; {0, 0} is a real record)
// device side: [flags | actions | Tx records]
constexpr size_t kBurstDevRec = 2u * kBurstZC, kBurstDevBytes = kBurstDevRec + 8u * kBurstZC;

// The device address of host bytes [h, h + span) when they are one pinned (device-mapped) host
// allocation, else nullptr.
static const uint8_t* pinned_alias(const void* h, uint64_t span) {
    if (h == nullptr || span == 0) return nullptr;
    hipPointerAttribute_t a0{}, a1{};
    const uint8_t* last = static_cast<const uint8_t*>(h) + (span - 1u);
    if (hipPointerGetAttributes(&a0, h) != hipSuccess || hipPointerGetAttributes(&a1, last) != hipSuccess) {
        (void)hipGetLastError();                        // pageable memory: not an error of this call
        return nullptr;
    }
    if (a0.type != hipMemoryTypeHost || a1.type != hipMemoryTypeHost || a0.devicePointer == nullptr ||
        static_cast<const uint8_t*>(a1.devicePointer) != static_cast<const uint8_t*>(a0.devicePointer) + (span - 1u)) {
        return nullptr;
    }
    return static_cast<const uint8_t*>(a0.devicePointer);
}

static NET_ERR ensure_burst(HostCtx& c) {
    if (c.h_burst != nullptr) return NET_UTIL_ERR_NONE;
    NC_HIP(hipMalloc(&c.d_burst, kBurstDevBytes));
    NC_HIP(hipHostMalloc(&c.h_burst, kBurstHostBytes, hipHostMallocMapped | hipHostMallocCoherent));
    NC_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&c.h_burst_dev), c.h_burst, 0));
    return NET_UTIL_ERR_NONE;
}

extern "C++" {
// ---- resident burst server (TUNE_BURST_ZERO_COPY 3; netcsum_pktstream.hip burst_server_kernel)
// A launch per burst is most of a small burst's cost (launch, dispatch, then the kernel's PCIe round
// trips). This context's server is launched on a stream of its own and serves every burst posted to
// it until it has been idle for TUNE_BURST_SERVER_IDLE_US (default 500 us: a device-wide
// synchronisation waits at most that long for it after the last burst) or resident for
// TUNE_BURST_SERVER_LIFE_US (default 1000 us) even while bursts keep coming: HIP maps the process's
// streams onto GPU_MAX_HW_QUEUES hardware queues, and kernels of a stream sharing the server's queue
// wait behind it, so each launch is bounded and the next burst relaunches it (one launch per ms of
// continuous service). Posting: the line's fields,
// then its burst number (a read that sees the new number with stale fields fails the check), a
// full fence, then the blocks' closed marks — a block that closed may have missed the post
// (Dekker's handshake, see the kernel), so the host waits the server out and relaunches it if the
// burst is not served. A server that stopped unnoticed is found by a stream query after 200 us
// without results.
static_assert(kServerBlocks <= netcsum::kBurstServerMaxBlocks && kBurstClosed + 8u * kServerBlocks <= kBurstFlags,
              "closed marks");

static void write_post(HostCtx& c, const netcsum::BurstPost& p) {
    volatile uint32_t* l = reinterpret_cast<volatile uint32_t*>(c.h_burst + kBurstPost);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(&p);
    for (int i = 2; i < 16; ++i) l[i] = q[i];            // fields, check
    std::atomic_thread_fence(std::memory_order_release);
    *reinterpret_cast<volatile uint64_t*>(c.h_burst + kBurstPost) = p.seq;
    std::atomic_thread_fence(std::memory_order_seq_cst); // the post before the closed marks are read
}

static NET_ERR launch_server(const Tune& t, HostCtx& c, uint64_t seq0) {
    volatile unsigned long long* closed = reinterpret_cast<volatile unsigned long long*>(c.h_burst + kBurstClosed);
    for (int b = 0; b < kServerBlocks; ++b) closed[b] = 0ull;
    int khz = 0;
    NC_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c.dev));
    netcsum::BurstServerArgs a{};
    a.post = reinterpret_cast<const netcsum::BurstPost*>(c.h_burst_dev + kBurstPost);
    a.closed = reinterpret_cast<unsigned long long*>(c.h_burst_dev + kBurstClosed);
    a.flags = c.h_burst_dev + kBurstFlags;
    a.act = c.h_burst_dev + kBurstAct;
    a.l2 = c.h_burst_dev + kBurstL2;
    a.rec =reinterpret_cast<netcsum::PktTxRecord*>(c.h_burst_dev + kBurstRec);
    a.off = reinterpret_cast<const uint64_t*>(c.h_burst_dev + kBurstOff);
    a.len = reinterpret_cast<const uint16_t*>(c.h_burst_dev + kBurstLen);
    a.seq0 = seq0;
    a.idle_ticks = (uint64_t)std::max(1, t.burst_idle) * (uint64_t)std::max(khz, 1) / 1000u;
    a.life_ticks = (uint64_t)std::max(1, t.burst_life) * (uint64_t)std::max(khz, 1) / 1000u;
    NC_HIP(netcsum::launch_burst_server(a, kServerBlocks, c.sstream,
                                        c.want_sums ? reinterpret_cast<uint32_t*>(c.h_burst_dev + kBurstSums) : nullptr));
    c.server_live = true;
    return NET_UTIL_ERR_NONE;
}

// Waits for the server's stream for at most limit_ms (a stream query loop, never a blocking
// synchronisation): a server launch queued behind other work on its hardware queue still ends, since
// every launch of every server is bounded by its residency limit, but the caller's wait must not
// depend on that. hipErrorNotReady when the stream is still busy at the deadline: a burst whose server
// is still queued 2 s after its post (burst_server_run's wait_out) fails with NET_UTIL_ERR_MI355X_DEV,
// and the server stays marked live (it still serves or stops). The first 20 us poll back to back (a
// server leaves within one burst of its stop), after that each poll yields the host core.
static hipError_t server_stream_wait(hipStream_t s, int limit_ms) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        const auto el = std::chrono::steady_clock::now() - t0;
        if (e != hipErrorNotReady || el > std::chrono::milliseconds(limit_ms)) {
            return e;
        }
        if (el > std::chrono::microseconds(20)) std::this_thread::yield();
    }
}

// Posts the stop line and waits for the server: limit_ms 0 without limit (release(), which frees the
// memory the server reads), else at most limit_ms; false if the server is still queued or running
// then (server_live stays set: it will serve whatever is posted next, or stop).
bool HostCtx::stop_server(int limit_ms) {
    if (server_live && sstream && h_burst) {
        netcsum::BurstPost p{};
        p.seq = netcsum::kBurstStop;
        p.check = netcsum::burst_post_check(p);
        write_post(*this, p);
        if (limit_ms <= 0) {
            (void)hipStreamSynchronize(sstream);
        } else if (server_stream_wait(sstream, limit_ms) == hipErrorNotReady) {
            return false;
        }
    }
    server_live = false;
    return true;
}

template <class Ready>
static NET_ERR burst_server_run(const Tune& t, HostCtx& c, netcsum::BurstPost p, Ready ready, uint32_t n) {
    if (c.sstream == nullptr) NC_HIP(hipStreamCreateWithFlags(&c.sstream, hipStreamNonBlocking));
    auto all_ready = [&](uint32_t from) {
        for (uint32_t i = from; i < n; ++i) {
            if (!ready(i)) return false;
        }
        return true;
    };
    auto wait_out = [&](uint32_t from) -> NET_ERR {     // the server has stopped, or is stopping
        NC_HIP(server_stream_wait(c.sstream, 2000));    // (its blocks stop together, after one burst at most)
        c.server_live = false;
        return all_ready(from) ? NET_UTIL_ERR_NONE : launch_server(t, c, p.seq - 1u);
    };
    // A post with fragment sums goes to the SUMS instantiation only. The thread's server is the other one
    // until its first such burst: that one is stopped and waited out here, before the post (it must never
    // read it), and every launch from then on is the SUMS one, which serves posts of both kinds — a driver
    // that alternates relaunches nothing.
    if (((p.form >> 1) & netcsum::kBurstSums) != 0u && !c.want_sums) {
        c.want_sums = true;
        if (c.server_live && !c.stop_server(2000)) return dev_fail("burst server still queued or running", hipErrorNotReady);
    }
    p.seq = ++c.post_seq;
    p.check = netcsum::burst_post_check(p);
    write_post(c, p);
    NET_ERR e = NET_UTIL_ERR_NONE;
    if (!c.server_live) {
        e = launch_server(t, c, p.seq - 1u);
    } else {
        const volatile unsigned long long* closed =
            reinterpret_cast<const volatile unsigned long long*>(c.h_burst + kBurstClosed);
        bool any = false;
        for (int b = 0; b < kServerBlocks; ++b) any = any || closed[b] != 0ull;
        if (any) e = wait_out(0u);
    }
    if (e != NET_UTIL_ERR_NONE) return e;
    const auto t0 = std::chrono::steady_clock::now();
    auto t_check = t0 + std::chrono::microseconds(200);
    uint32_t i = 0, spin = 0;
    while (i < n) {
        if (ready(i)) {
            ++i;
            continue;
        }
        if ((++spin & 255u) != 0u) continue;
        const auto t = std::chrono::steady_clock::now();
        if (t < t_check) continue;
        t_check = t + std::chrono::microseconds(200);
        if (c.server_live && hipStreamQuery(c.sstream) == hipSuccess) {   // stopped without serving it
            e = wait_out(i);
            if (e != NET_UTIL_ERR_NONE) return e;
        } else if (t - t0 > std::chrono::seconds(2)) {
            if (!c.stop_server(2000)) return dev_fail("burst server still queued or running", hipErrorNotReady);
            if (!all_ready(i)) return dev_fail("burst server results", hipErrorUnknown);
        }
    }
    return NET_UTIL_ERR_NONE;
}

// NetUtil_MI355X_LastLaunch after a zero-copy burst: which path served it (the tests check that the
// zero-copy path, not the copy pipeline, was taken)
// (an Ether burst: "ether_demux b=<blocks> | " — Tx: "ether_tx_demux b=<blocks> | " — in front, the
// device forms' shape, with the server's blocks, whose waves did the demux)
// (a burst with fragment sums: ",sums" after the direction — "burst_server_kernel rx,sums form=…")
static void server_launch_name(uint32_t form, uint32_t spw, bool tx) {
    char d[128];
    const bool ether = (form & netcsum::kBurstKindMask) == netcsum::kBurstEther;
    const bool sums = (form & netcsum::kBurstSums) != 0u;
    form &= ~netcsum::kBurstSums;
    int k = ether ? snprintf(d, sizeof d, "%s b=%d | ", tx ? "ether_tx_demux" : "ether_demux", kServerBlocks) : 0;
    snprintf(d + k, sizeof d - (size_t)k, "burst_server_kernel %s%s form=%s pkts_per_wave=%u zero-copy", tx ? "tx" : "rx",
             sums ? ",sums" : "",
             ether ? "ether" : form == netcsum::kBurstWhole ? "whole" : form == netcsum::kBurstLive ? "live" : "offlen", spw);
    netcsum::set_last_launch(d);
}

static void mark_zero_copy_launch(int zc) {
    char d[200];
    snprintf(d, sizeof d, "%s zero-copy%s", NetUtil_MI355X_LastLaunch(), zc == 1 ? " +burst_done_kernel" : "");
    netcsum::set_last_launch(d);
}

}  // extern "C++"

// A burst that qualifies for the zero-copy path — at most kBurstZC frames in one pinned allocation of at
// most kBurstZCSpan bytes — as the job of its launch: the ring's device alias and, for the
// offset/length form, the descriptors staged in the context's coherent pinned memory. *taken = false:
// it does not qualify (the caller takes the copy path); else the call's result.
static NET_ERR burst_job(HostCtx& c, const PktJob& h, PktJob* j, bool* taken) {
    *taken = false;
    if (h.n > kBurstZC) return NET_UTIL_ERR_NONE;
    uint64_t span = 0;
    if (h.off == nullptr) {
        span = (uint64_t)(h.n - 1u) * h.stride + h.pkt_len;
    } else {
        for (uint32_t i = 0; i < h.n; ++i) span = std::max<uint64_t>(span, h.off[i] + h.len[i]);
    }
    if (span > kBurstZCSpan) return NET_UTIL_ERR_NONE;
    const uint8_t* d_ring = pinned_alias(h.base, span);
    if (d_ring == nullptr) return NET_UTIL_ERR_NONE;
    *taken = true;
    NET_ERR e = ensure_burst(c);
    if (e != NET_UTIL_ERR_NONE) return e;
    *j = h;                                             // direction and policy fields; the pointers follow
    j->base = d_ring;
    j->flags = j->action = nullptr;
    if (h.off != nullptr) {                             // descriptors: staged in coherent pinned memory
        std::memcpy(c.h_burst + kBurstOff, h.off, (size_t)h.n * 8u);
        std::memcpy(c.h_burst + kBurstLen, h.len, (size_t)h.n * 2u);
        j->off = reinterpret_cast<const uint64_t*>(c.h_burst_dev + kBurstOff);
        j->len = reinterpret_cast<const uint16_t*>(c.h_burst_dev + kBurstLen);
    }
    j->stream = c.stream;
    j->bound_pref = kBurstBound;
    return NET_UTIL_ERR_NONE;
}

// What a burst waits on in the context's coherent host memory. Each result is written once, over a sentinel
// no result can take, so no completion protocol is needed: up to three byte arrays (flags, actions, classes:
// none of them is ever 0xFF), the 8-B Tx records (byte 7, the store mask, is 0..3) and the 4-B fragment
// records (0xFFFFFFFF, see kBurstSums above). arm(n) sets the sentinels of n results, before the burst is
// posted or launched; poll()(i) holds once result i has arrived in every array listed.
extern "C++" struct BurstWait {
    uint8_t* bytes[3] = {nullptr, nullptr, nullptr};
    uint8_t* rec = nullptr;
    uint8_t* sums = nullptr;

    void arm(uint32_t n) const {
        for (uint8_t* p : bytes) {
            if (p) std::memset(p, 0xFF, n);
        }
        if (rec) std::memset(rec, 0xFF, (size_t)n * 8u);
        if (sums) std::memset(sums, 0xFF, (size_t)n * 4u);
    }
    // The predicate of a burst that listed the first NB byte arrays, the records (REC) and the fragment
    // records (SUMS). Which arrays it reads is fixed at compile time, as in the lambdas it replaces: the host
    // calls it once per result and per poll, and testing at run time which arrays are listed cost an in-place
    // Rx burst of 1024 frames 1 us of its 38 (tools/burst_latency.c, profiles/hostpipe_latency.jsonl).
    template <int NB, bool REC, bool SUMS>
    auto poll() const {
        const BurstWait w = *this;
        return [w](uint32_t i) {
            for (int k = 0; k < NB; ++k) {
                if (*(volatile const uint8_t*)(w.bytes[k] + i) == 0xFFu) return false;
            }
            if (REC && *(volatile const uint8_t*)(w.rec + 8u * i + 7u) == 0xFFu) return false;
            return !SUMS || *(volatile const uint32_t*)(w.sums + 4u * i) != 0xFFFFFFFFu;
        };
    }
};

// Runs a qualified burst and returns when its results are in coherent host memory, in the mode
// TUNE_BURST_ZERO_COPY asks for: 3 the resident server (where the burst is in its domain, else as 2),
// 2 a launch whose results go straight into coherent memory, polled with ready(i) (wait.poll), 1 a launch into
// device memory and a one-wave completion kernel that copies them out and stores a tagged word.
// point(j, r0, r1) directs the job's outputs at the arrays — Tx: the records (wait.rec) alone; Rx: flags and
// actions (wait.bytes[0], [1]), which the done-kernel mode writes to device memory first, the actions only
// when the caller wants them (dev_r1) —; `post` carries the direction's own fields.
extern "C++" {
template <class Ready, class Point>
static NET_ERR burst_deliver(const Tune& t, HostCtx& c, PktJob j, const uint64_t* h_off, netcsum::BurstPost post,
                             const BurstWait& wait, bool dev_r1, Ready ready, Point point) {
    auto dev_alias = [&](uint8_t* h) { return h ? c.h_burst_dev + (h - c.h_burst) : nullptr; };
    uint8_t* h0_dev = dev_alias(wait.rec ? wait.rec : wait.bytes[0]);
    uint8_t* h1_dev = dev_alias(wait.rec ? nullptr : wait.bytes[1]);
    const int zc = t.burst_zc;
    if (zc >= 2) wait.arm(j.n);
    uint32_t form = 0, spw = 0;
    if (zc == 3 && server_form(h_off, j.stride, j.pkt_len, j.n, &form, &spw)) {   // the resident server
        post.ring = reinterpret_cast<uint64_t>(j.base);
        post.stride = (uint32_t)j.stride;
        post.n = j.n;
        post.pkt_len = j.pkt_len;
        post.spw = spw;
        if (!j.tx && j.sums != nullptr) form |= netcsum::kBurstSums;   // (the records: wait.sums)
        post.form = (form << 1) | (j.tx ? 1u : 0u);
        server_launch_name(form, spw, j.tx);
        return burst_server_run(t, c, post, ready, j.n);
    }
    if (zc >= 2) {                                      // results straight into coherent memory, polled
        point(j, h0_dev, h1_dev);
        const NET_ERR e = pkt_batch(t, j);
        if (e != NET_UTIL_ERR_NONE) return e;
        mark_zero_copy_launch(2);
        uint32_t i = 0;                                 // (each result is written once: scan forward)
        return spin_until(c, "burst results", [&] {
            while (i < j.n && ready(i)) ++i;
            return i == j.n;
        });
    }
    uint8_t* d0 = c.d_burst + (wait.rec ? kBurstDevRec : 0u);   // (device side: [flags | actions | Tx records])
    uint8_t* d1 = dev_r1 ? c.d_burst + kBurstZC : nullptr;
    point(j, d0, d1);
    const NET_ERR e = pkt_batch(t, j);
    if (e != NET_UTIL_ERR_NONE) return e;
    mark_zero_copy_launch(1);
    if (++c.seq == 0u) c.seq = 1u;
    const uint32_t tag = c.seq;
    *reinterpret_cast<volatile unsigned long long*>(c.h_burst + kBurstWord) = 0ull;
    NC_HIP(netcsum::launch_burst_done(d0, d1, wait.rec ? 8u * j.n : j.n, h0_dev, h1_dev,
                                      reinterpret_cast<unsigned long long*>(c.h_burst_dev + kBurstWord), tag, c.stream));
    volatile unsigned long long* w = reinterpret_cast<volatile unsigned long long*>(c.h_burst + kBurstWord);
    return spin_until(c, "burst completion word", [&] { return (uint32_t)*w == tag; });
}
}  // extern "C++"

// Rx over a pinned ring in place; *taken as burst_job's.
// With fragment sums (h.sums, RxBurstSumsHost): by the resident server only — TUNE_BURST_ZERO_COPY 3 and a
// layout the server takes (server_form); the launch-per-burst modes' kernels write a record twice where a
// datagram waits for the walk (kFragSumWalk), which a polled sentinel cannot tell from the result. The
// records arrive behind a sentinel of their own (0xFFFFFFFF, kBurstSums).
static NET_ERR rx_burst_zero_copy(const Tune& t, HostCtx& c, const PktJob& h, bool* taken) {
    *taken = false;
    NETCSUM_FRAG_SUM* h_sums = h.sums;
    if (h_sums != nullptr) {
        uint32_t form = 0, spw = 0;
        if (t.burst_zc != 3 || h.n > kBurstZC || !server_form(h.off, h.stride, h.pkt_len, h.n, &form, &spw)) {
            return NET_UTIL_ERR_NONE;
        }
    }
    PktJob j;
    NET_ERR e = burst_job(c, h, &j, taken);
    if (e != NET_UTIL_ERR_NONE || !*taken) return e;
    netcsum::BurstPost post{};
    post.rx_cfg = h.rx_cfg;
    BurstWait wait;
    wait.bytes[0] = c.h_burst + kBurstFlags;
    wait.bytes[1] = c.h_burst + kBurstAct;
    if (h_sums) wait.sums = c.h_burst + kBurstSums;
    auto point = [](PktJob& q, uint8_t* r0, uint8_t* r1) { q.flags = r0; q.action = r1; };
    // (the predicate's set of arrays is a compile-time choice, see BurstWait::poll: one call per set)
    e = h_sums ? burst_deliver(t, c, j, h.off, post, wait, h.action != nullptr, wait.poll<2, false, true>(), point)
               : burst_deliver(t, c, j, h.off, post, wait, h.action != nullptr, wait.poll<2, false, false>(), point);
    if (e != NET_UTIL_ERR_NONE) return e;
    if (h.flags) std::memcpy(h.flags, wait.bytes[0], h.n);
    if (h.action) std::memcpy(h.action, wait.bytes[1], h.n);
    if (h_sums) std::memcpy(h_sums, wait.sums, (size_t)h.n * 4u);
    return NET_UTIL_ERR_NONE;
}

// Packet batches from host memory: RxValidateIP / TxFinalizeIP / RxBurst / TxBurst over the chunks.
// Tx: the device form runs on the chunk's copy and records which checksum fields it wrote
// (fieldpos); a gather pass packs them into 8-B records, only those return D2H, and the host writes
// the fields into its own buffer once the chunk's stream has drained (run_pipe's retire step) — 8 B per
// datagram over PCIe instead of the chunk's bytes.
static NET_ERR pkt_host_copy(const Tune& t, const PktJob& h, uint32_t n_chunks) {
    const uint64_t* h_off = h.off;
    const uint16_t* h_len = h.len;
    const uint64_t stride = h.stride;
    const uint32_t n_pkt = h.n;
    uint8_t* h_flags = h.flags;
    uint8_t* h_action = h.action;
    NETCSUM_FRAG_SUM* h_sums = h.sums;                       // (RxBurstSumsHost: 4 B more per frame D2H)
    const bool tx = h.tx;
    HostCtx* cp = nullptr;
    NET_ERR e = host_ctx(&cp);
    if (e != NET_UTIL_ERR_NONE) return e;
    // n_chunks 0 = the library's choice (tools/burst_latency.c, profiles/r3x_burst_latency.jsonl): each
    // chunk adds 15-20 us per call and PCIe stays the bound, so one chunk, except Tx from 32 Ki
    // datagrams, whose host-side field write-back overlaps the later chunks' copies (262 144 frames:
    // 16 chunks 7.4 ms, one 8.4 ms)
    if (n_chunks == 0) n_chunks = tx ? std::min(16u, std::max(1u, n_pkt / 16384u)) : 1u;
    if (n_pkt / n_chunks > (1u << 28)) n_chunks = (n_pkt >> 28) + 1u;   // records: 32-bit offsets
    const ChunkPlan plan = plan_chunks(h_off, h_len, stride, h.pkt_len, n_pkt, n_chunks);
    const bool varlen = h_off != nullptr;
    const size_t per = plan.per;
    // device slot: [bytes | offsets | lengths | flags | actions | field positions | records | fragment sums];
    // host slot: [offsets | lengths | records]
    SlotLayout dev, host;
    dev.take(plan.max_span);
    const size_t o_off = dev.take(varlen ? per * 8u : 0u), o_len = dev.take(varlen ? per * 2u : 0u);
    const size_t o_fl = dev.take(per), o_act = dev.take(per);
    const size_t o_fp = dev.take(tx ? per * 4u : 0u), o_rec = dev.take(tx ? per * 8u : 0u);
    const size_t o_sum = dev.take(h_sums ? per * sizeof(NETCSUM_FRAG_SUM) : 0u);
    const size_t hs_off = host.take(varlen ? per * 8u : 0u), hs_len = host.take(varlen ? per * 2u : 0u);
    const size_t hs_rec = host.take(tx ? per * 8u : 0u);
    uint8_t* hb = static_cast<uint8_t*>(const_cast<void*>(h.base));
    auto issue = [&](const HostChunk& q, const PipeSlot& s) -> NET_ERR {
        uint8_t* d = s.d;
        NET_ERR e = copy_chunk_bytes(hb, q, s);
        if (e == NET_UTIL_ERR_NONE) e = copy_chunk_descriptors(h_off, h_len, q, s, hs_off, o_off, hs_len, o_len);
        if (e != NET_UTIL_ERR_NONE) return e;
        uint32_t* d_fp = tx ? reinterpret_cast<uint32_t*>(d + o_fp) : nullptr;
        if (tx) NC_HIP(hipMemsetAsync(d_fp, 0, (size_t)q.ns * 4u, s.st));   // a packet no kernel wrote: no fields
        const uint64_t* d_o = varlen ? reinterpret_cast<const uint64_t*>(d + o_off) : nullptr;
        PktJob job = h;                                      // the chunk's copy on the device
        job.base = d;
        job.off = d_o;
        job.len = varlen ? reinterpret_cast<const uint16_t*>(d + o_len) : nullptr;
        job.n = q.ns;
        job.flags = h_flags ? d + o_fl : nullptr;
        job.action = h_action ? d + o_act : nullptr;
        job.fieldpos = d_fp;
        job.sums = h_sums ? reinterpret_cast<NETCSUM_FRAG_SUM*>(d + o_sum) : nullptr;
        job.stream = s.st;
        e = pkt_batch(t, job);
        if (e != NET_UTIL_ERR_NONE) return e;
        if (h_flags) NC_HIP(hipMemcpyAsync(h_flags + q.s0, d + o_fl, q.ns, hipMemcpyDeviceToHost, s.st));
        if (h_action) NC_HIP(hipMemcpyAsync(h_action + q.s0, d + o_act, q.ns, hipMemcpyDeviceToHost, s.st));
        if (h_sums) {
            NC_HIP(hipMemcpyAsync(h_sums + q.s0, d + o_sum, (size_t)q.ns * sizeof(NETCSUM_FRAG_SUM), hipMemcpyDeviceToHost, s.st));
        }
        if (tx) {
            netcsum::PktBatchArgs g{};
            g.base = d;
            g.off = d_o;
            g.stride = stride;
            g.n = q.ns;
            g.fieldpos_out = d_fp;
            uint64_t* d_rec = reinterpret_cast<uint64_t*>(d + o_rec);
            NC_HIP(netcsum::launch_pkt_field_gather(g, d_rec, s.st));
            NC_HIP(hipMemcpyAsync(s.h + hs_rec, d_rec, (size_t)q.ns * 8u, hipMemcpyDeviceToHost, s.st));
        }
        return NET_UTIL_ERR_NONE;
    };
    if (!tx) return run_pipe(*cp, plan, dev, host, issue);   // (fixed-length Rx stages nothing: no host wait)
    return run_pipe(*cp, plan, dev, host, issue, [&](const HostChunk& q, const PipeSlot& s) {
        apply_field_records(hb, h_off, stride, q.s0, q.ns, reinterpret_cast<const uint64_t*>(s.h + hs_rec));
    });
}

// The datagrams an in-place Tx burst left alone (apply_tx_records: flag EXT_HDR, the rare IPv6 chains that
// run past the kernel's window and are walked by a later pass in the device forms), finished by the copy
// path as an offset/length batch of just those under the burst's UDP policy; their flags go to their
// places, and LastLaunch names both paths.
static NET_ERR tx_finish_skipped(const Tune& t, const void* h_base, const TxSkipped& skip, uint32_t udp_mode,
                                 uint8_t* h_flags) {
    if (skip.idx.empty()) return NET_UTIL_ERR_NONE;
    const uint32_t m = (uint32_t)skip.idx.size();
    std::vector<uint8_t> fl(m);
    char zc_name[256];
    snprintf(zc_name, sizeof zc_name, "%s", NetUtil_MI355X_LastLaunch());
    PktJob rest = pkt_job(h_base, skip.off.data(), skip.len.data(), 0, 0, m, h_flags ? fl.data() : nullptr, nullptr);
    rest.tx = true;
    rest.udp_mode = udp_mode;
    const NET_ERR e = pkt_host_copy(t, rest, 1u);
    if (e != NET_UTIL_ERR_NONE) return e;
    char d[256];
    snprintf(d, sizeof d, "%.180s +copy path for %u EXT_HDR datagrams", zc_name, m);
    netcsum::set_last_launch(d);
    if (h_flags) {
        for (uint32_t k = 0; k < m; ++k) h_flags[skip.idx[k]] = fl[k];
    }
    return NET_UTIL_ERR_NONE;
}

// Tx over a pinned ring: the checksum pass reads the ring in place and writes one 8-B
// record per datagram (PktTxRecord) to device memory — never into the ring —, the completion kernel
// copies the records into coherent pinned memory, and the host writes the fields into its ring
// (apply_tx_records; datagrams flagged EXT_HDR: tx_finish_skipped). *taken as for Rx.
static NET_ERR tx_burst_zero_copy(const Tune& t, HostCtx& c, const PktJob& h, bool* taken) {
    *taken = false;
    if (h.n > kBurstZC || t.kernel == 2) return NET_UTIL_ERR_NONE;
    netcsum::PktBatchArgs a{};
    a.stride = h.stride;
    a.len_u = h.pkt_len;
    a.n = h.n;
    a.off = h.off;                                      // (only tested against nullptr here)
    a.len = h.len;
    // the records come from the run-stream kernel only: the burst qualifies where pkt_batch picks it
    // (the tuned bound, else the whole-span form 0 or the live-piece form 2), and the server's form
    // where the server serves it (server_form: strided dense, sparse and offset/length rings)
    const int tb = t.pkt_bound;
    if (!((tb >= 0 && tb <= 3) ? netcsum::pkt_stream_supported(a, 0, tb)
                  : netcsum::pkt_stream_supported(a, 0, kBurstBound) || netcsum::pkt_stream_supported(a, 0, 2))) {
        return NET_UTIL_ERR_NONE;
    }
    PktJob j;
    NET_ERR e = burst_job(c, h, &j, taken);
    if (e != NET_UTIL_ERR_NONE || !*taken) return e;
    netcsum::BurstPost post{};
    post.udp_mode = h.udp_mode;
    BurstWait wait;
    wait.rec = c.h_burst + kBurstRec;
    e = burst_deliver(t, c, j, h.off, post, wait, false, wait.poll<0, true, false>(), [](PktJob& q, uint8_t* r0, uint8_t*) { q.rec_only = reinterpret_cast<netcsum::PktTxRecord*>(r0); });
    if (e != NET_UTIL_ERR_NONE) return e;
    const TxSkipped skip = apply_tx_records(reinterpret_cast<const uint64_t*>(wait.rec), static_cast<uint8_t*>(const_cast<void*>(h.base)),
                                            h.off, h.len, h.stride, h.pkt_len, 0u, h.n, h.flags);
    return tx_finish_skipped(t, h.base, skip, h.udp_mode, h.flags);
}

// h: the batch with HOST pointers.
static NET_ERR pkt_host(const PktJob& h, uint32_t n_chunks) {
    if (h.n == 0) return NET_UTIL_ERR_NONE;
    if (h.n > 0x7FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (h.base == nullptr || (h.off != nullptr) != (h.len != nullptr) || (!h.tx && h.flags == nullptr && h.action == nullptr)) {
        return NET_ERR_FAULT_NULL_PTR;
    }
    const Tune& t = tune();
    if (n_chunks == 0 && t.burst_zc != 0) {                  // a burst from a pinned ring: in place
        HostCtx* cp = nullptr;
        NET_ERR e = host_ctx(&cp);
        if (e != NET_UTIL_ERR_NONE) return e;
        bool taken = false;
        e = h.tx ? tx_burst_zero_copy(t, *cp, h, &taken) : rx_burst_zero_copy(t, *cp, h, &taken);
        if (taken) return e;
    }
    return pkt_host_copy(t, h, n_chunks);
}

NET_ERR NetUtil_MI355X_RxValidateIPHost(const void* h_base, const uint64_t* h_off, const uint16_t* h_len, uint64_t stride,
                                        CPU_INT16U pkt_len, uint32_t n_pkt, uint8_t* h_flags, uint32_t n_chunks) {
    if (n_pkt != 0 && h_flags == nullptr) return NET_ERR_FAULT_NULL_PTR;
    return pkt_host(pkt_job(h_base, h_off, h_len, stride, pkt_len, n_pkt, h_flags, nullptr), n_chunks);
}

NET_ERR NetUtil_MI355X_TxFinalizeIPHost(void* h_base, const uint64_t* h_off, const uint16_t* h_len, uint64_t stride,
                                        CPU_INT16U pkt_len, uint32_t n_pkt, uint8_t* h_flags, int udp_tx_csum,
                                        uint32_t n_chunks) {
    PktJob h = pkt_job(h_base, h_off, h_len, stride, pkt_len, n_pkt, h_flags, nullptr);
    h.tx = true;
    h.udp_mode = udp_tx_csum ? 1u : 0u;
    return pkt_host(h, n_chunks);
}

NET_ERR NetUtil_MI355X_RxBurstHost(const void* h_base, const uint64_t* h_off, const uint16_t* h_len, uint64_t stride,
                                   CPU_INT16U pkt_len, uint32_t n_pkt, uint32_t rx_cfg, uint8_t* h_action,
                                   uint8_t* h_flags, uint32_t n_chunks) {
    if (n_pkt != 0 && h_action == nullptr) return NET_ERR_FAULT_NULL_PTR;
    if (rx_cfg & ~(uint32_t)NETCSUM_RXCFG_UDP_DISCARD_NO_CHK_SUM) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    PktJob h = pkt_job(h_base, h_off, h_len, stride, pkt_len, n_pkt, h_flags, nullptr);
    h.action = h_action;
    h.rx_cfg = rx_cfg;
    return pkt_host(h, n_chunks);
}

NET_ERR NetUtil_MI355X_RxBurstSumsHost(const void* h_base, const uint64_t* h_off, const uint16_t* h_len, uint64_t stride,
                                       CPU_INT16U pkt_len, uint32_t n_pkt, uint32_t rx_cfg, uint8_t* h_action,
                                       uint8_t* h_flags, NETCSUM_FRAG_SUM* h_sums, uint32_t n_chunks) {
    if (n_pkt != 0 && h_action == nullptr) return NET_ERR_FAULT_NULL_PTR;
    if (rx_cfg & ~(uint32_t)NETCSUM_RXCFG_UDP_DISCARD_NO_CHK_SUM) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (n_pkt != 0 && h_sums == nullptr) return NET_ERR_FAULT_NULL_PTR;
    if (n_pkt > 0x3FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    PktJob h = pkt_job(h_base, h_off, h_len, stride, pkt_len, n_pkt, h_flags, nullptr);
    h.action = h_action;
    h.rx_cfg = rx_cfg;
    h.sums = h_sums;
    return pkt_host(h, n_chunks);
}

// ---- Ether bursts (RxBurstEtherHost, TxBurstEtherHost and the sums form)
// The front of an Ether burst over a pinned ring in place, by the resident server's Ether forms
// (netcsum_pktstream.hip pkt_ether_run: the wave that owns a run classifies its frames and streams their
// datagrams). Taken under rx_burst_zero_copy's conditions — at most kBurstZC frames whose span is one pinned
// allocation of at most kBurstZCSpan bytes —; the callers ask in the server's mode only
// (TUNE_BURST_ZERO_COPY 3: the launch-per-burst experiments are not extended to frames). *taken = false: the
// caller takes the copy pipeline. Else the descriptors the burst gives are staged in the context's coherent
// memory, and b holds the form (with kBurstEtherOff / kBurstEtherLen), the run length and a post with the
// ring and its geometry filled; the direction adds its own fields and the form's direction and sums bits.
struct EtherBurst {
    uint32_t           form = netcsum::kBurstEther;
    uint32_t           spw = 0;
    netcsum::BurstPost post{};                              // (every field a form does not use: 0)
};

static NET_ERR ether_burst_setup(HostCtx& c, const void* h_base, const uint64_t* h_off, const uint16_t* h_len,
                                 uint64_t stride, CPU_INT16U frame_len, uint32_t n, EtherBurst* b, bool* taken) {
    *taken = false;
    if (n > kBurstZC) return NET_UTIL_ERR_NONE;
    const HostChunk all = chunk_span(h_off, h_len, stride, frame_len, 0u, n);
    if (all.hi <= all.lo || all.hi - all.lo > kBurstZCSpan) return NET_UTIL_ERR_NONE;
    const uint8_t* d_lo = pinned_alias(static_cast<const uint8_t*>(h_base) + all.lo, all.hi - all.lo);
    if (d_lo == nullptr) return NET_UTIL_ERR_NONE;
    *taken = true;
    NET_ERR e = ensure_burst(c);
    if (e != NET_UTIL_ERR_NONE) return e;
    b->spw = server_run(n);                                 // (as the offset/length form)
    if (h_off) {
        std::memcpy(c.h_burst + kBurstOff, h_off, (size_t)n * 8u);
        b->form |= netcsum::kBurstEtherOff;
    }
    if (h_len) {
        std::memcpy(c.h_burst + kBurstLen, h_len, (size_t)n * 2u);
        b->form |= netcsum::kBurstEtherLen;
    }
    b->post.ring = reinterpret_cast<uint64_t>(d_lo - all.lo);   // the base's alias: offsets count from it
    b->post.stride = (uint32_t)stride;
    b->post.n = n;
    b->post.pkt_len = frame_len;
    b->post.spw = b->spw;
    return NET_UTIL_ERR_NONE;
}

// Rx: flags, actions and classes arrive in coherent memory behind 0xFF sentinels (no class is >= 16), and the
// host polls all three. h_sums (RxBurstEtherSumsHost): the post carries kBurstSums, and the frames' records
// arrive behind their own sentinel (0xFFFFFFFF, kBurstSums) and are polled with the rest.
static NET_ERR rx_burst_ether_zero_copy(const Tune& t, HostCtx& c, const void* h_base, const uint64_t* h_off,
                                        const uint16_t* h_len, uint64_t stride, CPU_INT16U frame_len, uint32_t n,
                                        uint32_t rx_cfg, uint32_t eth_cfg, const uint8_t* hw_addr, uint8_t* h_action,
                                        uint8_t* h_flags, uint8_t* h_l2, NETCSUM_FRAG_SUM* h_sums, bool* taken) {
    EtherBurst b;
    NET_ERR e = ether_burst_setup(c, h_base, h_off, h_len, stride, frame_len, n, &b, taken);
    if (e != NET_UTIL_ERR_NONE || !*taken) return e;
    BurstWait wait;
    wait.bytes[0] = c.h_burst + kBurstFlags;
    wait.bytes[1] = c.h_burst + kBurstAct;
    wait.bytes[2] = c.h_burst + kBurstL2;
    if (h_sums) {
        wait.sums = c.h_burst + kBurstSums;
        b.form |= netcsum::kBurstSums;
    }
    wait.arm(n);
    b.post.form = b.form << 1;
    b.post.rx_cfg = rx_cfg;
    b.post.eth_cfg = eth_cfg;
    pack_hw_addr(hw_addr, &b.post.have_hw, &b.post.hw_lo, &b.post.hw_hi);
    server_launch_name(b.form, b.spw, false);
    e = h_sums ? burst_server_run(t, c, b.post, wait.poll<3, false, true>(), n)
               : burst_server_run(t, c, b.post, wait.poll<3, false, false>(), n);
    if (e != NET_UTIL_ERR_NONE) return e;
    if (h_flags) std::memcpy(h_flags, wait.bytes[0], n);
    std::memcpy(h_action, wait.bytes[1], n);
    std::memcpy(h_l2, wait.bytes[2], n);
    if (h_sums) std::memcpy(h_sums, wait.sums, (size_t)n * 4u);
    return NET_UTIL_ERR_NONE;
}

// RxBurstEther over frames in host memory. A burst from a pinned ring (n_chunks 0, at most 4096 frames in
// one pinned allocation, TUNE_BURST_ZERO_COPY 3) is served in place by the resident burst server
// (rx_burst_ether_zero_copy). Every other call: the copy pipeline with the frame-level descriptors
// (per-frame lengths also without offsets: a ring of slots) and the classes as a third result. Per chunk:
// H2D of the frames' span and descriptors, the device form (demux, packet batch) on the chunk's stream,
// D2H of actions, flags and classes.
// sums (RxBurstEtherSumsHost): both stages also return one NETCSUM_FRAG_SUM per frame — the copy pipeline
// through a fourth result region and the device form RxBurstEtherSums.
static NET_ERR rx_burst_ether_host(const void* h_base, const uint64_t* h_off, const uint16_t* h_len, uint64_t stride,
                                   CPU_INT16U frame_len, uint32_t n_frame, uint32_t rx_cfg, uint32_t eth_cfg,
                                   const uint8_t* hw_addr, uint8_t* h_action, uint8_t* h_flags, uint8_t* h_l2, bool sums,
                                   NETCSUM_FRAG_SUM* h_sums, uint32_t n_chunks) {
    NET_ERR e = check_rx_ether(h_base, h_action, h_l2, n_frame, rx_cfg, eth_cfg);
    if (e == NET_UTIL_ERR_NONE && sums) e = check_frag_sums(h_sums, n_frame);
    if (e != NET_UTIL_ERR_NONE) return e;
    if (n_frame == 0) return NET_UTIL_ERR_NONE;
    if (n_frame > 0x7FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    HostCtx* cp = nullptr;
    e = host_ctx(&cp);
    if (e != NET_UTIL_ERR_NONE) return e;
    const Tune& t = tune();
    if (n_chunks == 0 && t.burst_zc == 3) {                  // a burst from a pinned ring: in place
        bool taken = false;
        e = rx_burst_ether_zero_copy(t, *cp, h_base, h_off, h_len, stride, frame_len, n_frame, rx_cfg, eth_cfg, hw_addr,
                                     h_action, h_flags, h_l2, h_sums, &taken);
        if (taken) return e;
    }
    const ChunkPlan plan = plan_chunks(h_off, h_len, stride, frame_len, n_frame, n_chunks);   // (0: one chunk)
    const size_t per = plan.per;
    // device slot: [bytes | offsets | lengths | flags | actions | classes | fragment sums]; host slot:
    // [offsets | lengths]
    SlotLayout dev, host;
    dev.take(plan.max_span);
    const size_t o_off = dev.take(h_off ? per * 8u : 0u), o_len = dev.take(h_len ? per * 2u : 0u);
    const size_t o_fl = dev.take(per), o_act = dev.take(per), o_l2 = dev.take(per);
    const size_t o_sum = dev.take(h_sums ? per * sizeof(NETCSUM_FRAG_SUM) : 0u);
    const size_t hs_off = host.take(h_off ? per * 8u : 0u), hs_len = host.take(h_len ? per * 2u : 0u);
    return run_pipe(*cp, plan, dev, host, [&](const HostChunk& q, const PipeSlot& s) -> NET_ERR {
        uint8_t* d = s.d;
        NET_ERR e = copy_chunk_bytes(h_base, q, s);
        if (e == NET_UTIL_ERR_NONE) e = copy_chunk_descriptors(h_off, h_len, q, s, hs_off, o_off, hs_len, o_len);
        if (e != NET_UTIL_ERR_NONE) return e;
        const uint64_t* d_o = h_off ? reinterpret_cast<const uint64_t*>(d + o_off) : nullptr;
        const uint16_t* d_l = h_len ? reinterpret_cast<const uint16_t*>(d + o_len) : nullptr;
        if (h_sums) {
            e = NetUtil_MI355X_RxBurstEtherSums(d, d_o, d_l, stride, frame_len, q.ns, rx_cfg, eth_cfg, hw_addr, d + o_act,
                                                h_flags ? d + o_fl : nullptr, d + o_l2,
                                                reinterpret_cast<NETCSUM_FRAG_SUM*>(d + o_sum), s.st);
        } else {
            e = NetUtil_MI355X_RxBurstEther(d, d_o, d_l, stride, frame_len, q.ns, rx_cfg, eth_cfg, hw_addr, d + o_act,
                                            h_flags ? d + o_fl : nullptr, d + o_l2, s.st);
        }
        if (e != NET_UTIL_ERR_NONE) return e;
        if (h_flags) NC_HIP(hipMemcpyAsync(h_flags + q.s0, d + o_fl, q.ns, hipMemcpyDeviceToHost, s.st));
        NC_HIP(hipMemcpyAsync(h_action + q.s0, d + o_act, q.ns, hipMemcpyDeviceToHost, s.st));
        NC_HIP(hipMemcpyAsync(h_l2 + q.s0, d + o_l2, q.ns, hipMemcpyDeviceToHost, s.st));
        if (h_sums) {
            NC_HIP(hipMemcpyAsync(h_sums + q.s0, d + o_sum, (size_t)q.ns * sizeof(NETCSUM_FRAG_SUM), hipMemcpyDeviceToHost, s.st));
        }
        return NET_UTIL_ERR_NONE;
    });
}

NET_ERR NetUtil_MI355X_RxBurstEtherHost(const void* h_base, const uint64_t* h_off, const uint16_t* h_len, uint64_t stride,
                                        CPU_INT16U frame_len, uint32_t n_frame, uint32_t rx_cfg, uint32_t eth_cfg,
                                        const uint8_t* hw_addr, uint8_t* h_action, uint8_t* h_flags, uint8_t* h_l2,
                                        uint32_t n_chunks) {
    return rx_burst_ether_host(h_base, h_off, h_len, stride, frame_len, n_frame, rx_cfg, eth_cfg, hw_addr, h_action, h_flags,
                               h_l2, false, nullptr, n_chunks);
}

NET_ERR NetUtil_MI355X_RxBurstEtherSumsHost(const void* h_base, const uint64_t* h_off, const uint16_t* h_len, uint64_t stride,
                                            CPU_INT16U frame_len, uint32_t n_frame, uint32_t rx_cfg, uint32_t eth_cfg,
                                            const uint8_t* hw_addr, uint8_t* h_action, uint8_t* h_flags, uint8_t* h_l2,
                                            NETCSUM_FRAG_SUM* h_sums, uint32_t n_chunks) {
    return rx_burst_ether_host(h_base, h_off, h_len, stride, frame_len, n_frame, rx_cfg, eth_cfg, hw_addr, h_action, h_flags,
                               h_l2, true, h_sums, n_chunks);
}

// A Tx Ether burst over a pinned ring in place, by the resident server's Tx Ether form
// (netcsum_pktstream.hip pkt_ether_run<TX, REC>): the wave that owns a run classifies its frames by the Tx
// rule, stores the classes and streams the datagrams in the record-producing Tx instantiation; classes
// and records arrive in coherent memory behind 0xFF sentinels (no class is >= 16, a record's store byte is
// 0..3), the host polls both and applies each record at the frame's start + 14, exactly as
// tx_burst_zero_copy does for datagrams. Nothing on the device writes the ring. Taken under
// ether_burst_setup's conditions, for a burst tx_burst_zero_copy would accept as an offset/length one (the
// records come from the run-stream kernel only). *taken = false: the caller takes the copy pipeline.
static NET_ERR tx_burst_ether_zero_copy(const Tune& t, HostCtx& c, void* h_base, const uint64_t* h_off, const uint16_t* h_len,
                                        uint64_t stride, CPU_INT16U frame_len, uint32_t n, uint8_t* h_flags, uint8_t* h_l2,
                                        bool* taken) {
    *taken = false;
    if (t.kernel == 2) return NET_UTIL_ERR_NONE;
    const int tb = t.pkt_bound;
    if (tb == 0 || tb == 3) return NET_UTIL_ERR_NONE;        // (offset/length runs: the live-piece forms only)
    EtherBurst b;
    NET_ERR e = ether_burst_setup(c, h_base, h_off, h_len, stride, frame_len, n, &b, taken);
    if (e != NET_UTIL_ERR_NONE || !*taken) return e;
    BurstWait wait;
    wait.bytes[0] = c.h_burst + kBurstL2;
    wait.rec = c.h_burst + kBurstRec;
    wait.arm(n);
    b.post.form = (b.form << 1) | 1u;
    b.post.udp_mode = 2u;
    server_launch_name(b.form, b.spw, true);
    e = burst_server_run(t, c, b.post, wait.poll<1, true, false>(), n);
    if (e != NET_UTIL_ERR_NONE) return e;
    std::memcpy(h_l2, wait.bytes[0], n);
    const TxSkipped skip = apply_tx_records(reinterpret_cast<const uint64_t*>(wait.rec), static_cast<uint8_t*>(h_base), h_off,
                                            h_len, stride, frame_len, NETCSUM_L2_HDR_ETHER, n, h_flags);
    return tx_finish_skipped(t, h_base, skip, 2u, h_flags);
}

// The copy pipeline of TxBurstEtherHost (below): for run_pipe, a slot layout over frame-level descriptors that
// ends in field positions and records, an issue step and a retire step that applies the records. Per chunk: H2D of the frames' span and descriptors, the device form on the chunk's
// copy (Tx demux, the offset/length Tx batch, the field gather over the datagrams' descriptors), D2H of the
// flags, the classes and one 8-B record per frame; once the chunk's stream has drained the host writes the
// recorded fields into its own ring at frame + 14 + position. Nothing else of the ring is written.
static NET_ERR tx_burst_ether_copy(const Tune& t, HostCtx& c, void* h_base, const uint64_t* h_off, const uint16_t* h_len,
                                   uint64_t stride, CPU_INT16U frame_len, uint32_t n_frame, uint8_t* h_flags, uint8_t* h_l2,
                                   uint32_t n_chunks) {
    // chunks: TxBurstHost's choice (the host's field write-back overlaps the later chunks' copies)
    if (n_chunks == 0) n_chunks = std::min(16u, std::max(1u, n_frame / 16384u));
    if (n_frame / n_chunks > (1u << 28)) n_chunks = (n_frame >> 28) + 1u;
    const ChunkPlan plan = plan_chunks(h_off, h_len, stride, frame_len, n_frame, n_chunks);
    const size_t per = plan.per;
    // device slot: [bytes | offsets | lengths | flags | classes | field positions | records];
    // host slot: [offsets | lengths | records]
    SlotLayout dev, host;
    dev.take(plan.max_span);
    const size_t o_off = dev.take(h_off ? per * 8u : 0u), o_len = dev.take(h_len ? per * 2u : 0u);
    const size_t o_fl = dev.take(per), o_l2 = dev.take(per);
    const size_t o_fp = dev.take(per * 4u), o_rec = dev.take(per * 8u);
    const size_t hs_off = host.take(h_off ? per * 8u : 0u), hs_len = host.take(h_len ? per * 2u : 0u);
    const size_t hs_rec = host.take(per * 8u);
    uint8_t* hb = static_cast<uint8_t*>(h_base);
    return run_pipe(
        c, plan, dev, host,
        [&](const HostChunk& q, const PipeSlot& s) -> NET_ERR {
            uint8_t* d = s.d;
            NET_ERR e = copy_chunk_bytes(hb, q, s);
            if (e == NET_UTIL_ERR_NONE) e = copy_chunk_descriptors(h_off, h_len, q, s, hs_off, o_off, hs_len, o_len);
            if (e != NET_UTIL_ERR_NONE) return e;
            uint32_t* d_fp = reinterpret_cast<uint32_t*>(d + o_fp);
            uint64_t* d_rec = reinterpret_cast<uint64_t*>(d + o_rec);
            NC_HIP(hipMemsetAsync(d_fp, 0, (size_t)q.ns * 4u, s.st));   // a frame no kernel wrote: no fields
            // (a strided chunk's copy starts at its first slot: q.lo = s0 * stride, so slot i of the chunk is at i * stride)
            e = tx_burst_ether(t, d, h_off ? reinterpret_cast<const uint64_t*>(d + o_off) : nullptr,
                               h_len ? reinterpret_cast<const uint16_t*>(d + o_len) : nullptr, stride, frame_len, q.ns,
                               h_flags ? d + o_fl : nullptr, d + o_l2, s.st, d_fp, d_rec);
            if (e != NET_UTIL_ERR_NONE) return e;
            if (h_flags) NC_HIP(hipMemcpyAsync(h_flags + q.s0, d + o_fl, q.ns, hipMemcpyDeviceToHost, s.st));
            NC_HIP(hipMemcpyAsync(h_l2 + q.s0, d + o_l2, q.ns, hipMemcpyDeviceToHost, s.st));
            NC_HIP(hipMemcpyAsync(s.h + hs_rec, d_rec, (size_t)q.ns * 8u, hipMemcpyDeviceToHost, s.st));
            return NET_UTIL_ERR_NONE;
        },
        [&](const HostChunk& q, const PipeSlot& s) {
            apply_field_records(hb + NETCSUM_L2_HDR_ETHER, h_off, stride, q.s0, q.ns,
                                reinterpret_cast<const uint64_t*>(s.h + hs_rec));
        });
}

// TxBurstEther over frames in host memory. A burst from a pinned ring (n_chunks 0, at most 4096 frames in one
// pinned allocation, TUNE_BURST_ZERO_COPY 3) is served in place by the resident burst server
// (tx_burst_ether_zero_copy), every other call by the copy pipeline (tx_burst_ether_copy). Checks, their
// order, error codes and the resulting bytes do not depend on the path.
NET_ERR NetUtil_MI355X_TxBurstEtherHost(void* h_base, const uint64_t* h_off, const uint16_t* h_len, uint64_t stride,
                                        CPU_INT16U frame_len, uint32_t n_frame, uint8_t* h_flags, uint8_t* h_l2,
                                        uint32_t n_chunks) {
    if (n_frame != 0 && (h_l2 == nullptr || h_base == nullptr)) return NET_ERR_FAULT_NULL_PTR;
    if (n_frame > 0x7FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (n_frame == 0) return NET_UTIL_ERR_NONE;
    HostCtx* cp = nullptr;
    NET_ERR e = host_ctx(&cp);
    if (e != NET_UTIL_ERR_NONE) return e;
    const Tune& t = tune();
    if (n_chunks == 0 && t.burst_zc == 3) {                  // a burst from a pinned ring: in place
        bool taken = false;
        e = tx_burst_ether_zero_copy(t, *cp, h_base, h_off, h_len, stride, frame_len, n_frame, h_flags, h_l2, &taken);
        if (taken) return e;
    }
    return tx_burst_ether_copy(t, *cp, h_base, h_off, h_len, stride, frame_len, n_frame, h_flags, h_l2, n_chunks);
}

NET_ERR NetUtil_MI355X_TxBurstHost(void* h_base, const uint64_t* h_off, const uint16_t* h_len, uint64_t stride,
                                   CPU_INT16U pkt_len, uint32_t n_pkt, uint8_t* h_flags, uint32_t n_chunks) {
    PktJob h = pkt_job(h_base, h_off, h_len, stride, pkt_len, n_pkt, h_flags, nullptr);
    h.tx = true;
    h.udp_mode = 2u;
    return pkt_host(h, n_chunks);
}

}  // extern "C"
