// netcsum_abi.hip — extern "C" entry points of include/netcsum_mi355x.h groups (2) and (3) for
// device-resident data: argument checks, the calling thread's tuning (NetUtil_MI355X_Tune), its scratch
// leases and ring / pool plans, and the launches of what netcsum_policy.hip decided. The host-memory
// forms are in netcsum_hostmem.hip. Group (1) — the reference's four signatures — lives in
// ../host/net_util_mi355x.c (plain C) and reaches the GPU through NetUtil_MI355X_StreamSum32 there.
//
// There is deliberately NO CPU fallback anywhere in this library: if the HIP runtime or device
// fails, the caller gets NET_UTIL_ERR_MI355X_DEV and a message on stderr.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/netcsum_mi355x.h"
#include "netcsum_device.h"
#include "netcsum_host.h"
#include "netcsum_kernels.h"

using namespace nchost;

namespace {

thread_local Tune tls_tune;
std::atomic<int> g_err_reports{0};

}  // namespace

NET_ERR nchost::dev_fail(const char* what, hipError_t e) {
    if (g_err_reports.fetch_add(1) < 8) {
        std::fprintf(stderr, "[netcsum-mi355x] %s failed: %s (%d) — no CPU fallback, returning "
                             "NET_UTIL_ERR_MI355X_DEV\n", what, hipGetErrorString(e), (int)e);
    }
    return (NET_ERR)NET_UTIL_ERR_MI355X_DEV;
}

int nchost::cu_count(int dev) {
    static std::atomic<int> cache[kMaxDev];
    if (dev < 0 || dev >= kMaxDev) return 256;
    int v = cache[dev].load();
    if (v <= 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
            v = 256;
        }
        cache[dev].store(v);
    }
    return v;
}

const Tune& nchost::tune() { return tls_tune; }

NET_ERR nchost::check_op(NETCSUM_OP op, const void* d_pseudo, CPU_INT16U pseudo_len) {
    if ((int)op < 0 || (int)op > 3) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if ((op == NETCSUM_OP_HDR_CALC || op == NETCSUM_OP_HDR_VERIFY) && d_pseudo != nullptr && pseudo_len != 0) {
        return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;     // header checksums take no pseudo-header
    }
    return NET_UTIL_ERR_NONE;
}

NET_ERR nchost::check_rx_ether(const void* base, const uint8_t* action, const uint8_t* l2, uint32_t n_frame, uint32_t rx_cfg,
                               uint32_t eth_cfg) {
    if (n_frame != 0 && (action == nullptr || l2 == nullptr || base == nullptr)) return NET_ERR_FAULT_NULL_PTR;
    if (rx_cfg & ~(uint32_t)NETCSUM_RXCFG_UDP_DISCARD_NO_CHK_SUM) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (eth_cfg & ~(uint32_t)NETCSUM_ETHCFG_MCAST_RX) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    return NET_UTIL_ERR_NONE;
}

NET_ERR nchost::check_frag_sums(const NETCSUM_FRAG_SUM* sums, uint32_t n_frame) {
    if (n_frame != 0 && sums == nullptr) return NET_ERR_FAULT_NULL_PTR;
    // one record is one 4-B store (offsets of the lane-group form's buffer stores: 32 bits)
    if (((uintptr_t)sums & 3u) != 0u || n_frame > 0x3FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    return NET_UTIL_ERR_NONE;
}

namespace {

// Device scratch of the packet batches (two-pass Tx records, the walk pass's flags when the caller
// passes none) and of the varlen run word: plain hipMalloc memory (memory from the stream-ordered
// allocator measured ~70 us slower for the record stores on 1 M packets, profiles/r2tx_*), one buffer
// per (device, stream), kept PER HOST THREAD: only the calling thread hands a buffer out, launches on
// it and evicts it, so no other thread can free it between the hand-out and the launches that use it.
// A lease records an event on the stream after the launches that use its buffer; evicting (least
// recently used, beyond kScratchSlots) or growing a buffer waits for that event — never for the whole
// device — and a new lease whose earlier launches are still pending makes the stream wait for it, so
// a stream created with the handle of a destroyed one whose work is still running cannot overtake it.
// Under stream capture no event is recorded and the slot is pinned (the captured graph keeps its
// address): capture needs one uncaptured call first. Later uncaptured calls on that stream get a slot
// of their own. A graph's replays share its pinned buffer with each other, so replays of one graph
// must be ordered (one stream, or events) — as for any graph that writes a buffer.
constexpr int kScratchSlots = 16;
struct ScratchSlot {
    int                dev = -1;
    hipStream_t        stream = nullptr;
    void*              p = nullptr;
    size_t             cap = 0;
    uint64_t           used = 0;
    hipEvent_t         ev = nullptr;  // recorded after the last launches that used p
    bool               ev_live = false;
    bool               pinned = false;  // used under stream capture: never freed while the thread runs
    bool               unordered = false;  // used by a lease with no event since the last record
    bool               tail_dirty = false; // tail words handed out by a call that did not confirm the
                                           // launch of the pass that resets them (ScratchLease::tail_words)
    uint32_t           seq = 0;         // last tag handed out (ScratchLease::next_tag)
};

hipError_t slot_wait(ScratchSlot& sl) {                // all launches that used sl.p have finished
    hipError_t e = hipSuccess;
    if (sl.unordered) {
        e = hipDeviceSynchronize();                    // (the caller has made sl.dev current)
        sl.unordered = false;
    } else if (sl.ev_live) {
        e = hipEventSynchronize(sl.ev);
    }
    sl.ev_live = false;
    return e;
}

struct ScratchCache {
    ScratchSlot slots[kScratchSlots];
    uint64_t    tick = 0;

    void drop(ScratchSlot& sl) {                       // free a slot's buffer and event (its device)
        int cur = -1;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        if (sl.dev >= 0) (void)hipSetDevice(sl.dev);
        (void)slot_wait(sl);
        if (sl.p) (void)hipFree(sl.p);
        if (sl.ev) (void)hipEventDestroy(sl.ev);
        if (have && cur >= 0 && cur != sl.dev) (void)hipSetDevice(cur);
        sl = ScratchSlot{};
    }
    void release_all() {
        for (ScratchSlot& sl : slots) {
            if (sl.p || sl.ev) drop(sl);
        }
    }
    ~ScratchCache() { release_all(); }
};

thread_local ScratchCache tls_scratch;

// A buffer of >= `bytes` for launches on stream `st` of device `dev`; end() (or the destructor) after
// the last launch that uses it records the slot's event. An UNORDERED lease (ordered = false) is for
// contents any interleaving leaves correct (the varlen run word: any value is a valid run length):
// it records no event (an event record costs ~3 us of GPU time per call, profiles/r3d_event_probe)
// and its slot is freed after a device synchronisation instead.
constexpr size_t kTailBytes = 64;

class ScratchLease {
public:
    hipError_t acquire(int dev, hipStream_t st, size_t bytes, bool ordered = true) {
        stream_ = st;
        ordered_ = ordered;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (st != nullptr && hipStreamIsCapturing(st, &cs) != hipSuccess) cs = hipStreamCaptureStatusNone;
        capturing_ = cs != hipStreamCaptureStatusNone;
        ScratchCache& c = tls_scratch;
        ScratchSlot* hit = nullptr;
        ScratchSlot* lru = nullptr;
        for (ScratchSlot& sl : c.slots) {
            // a slot pinned by a capture belongs to its graph: a direct (uncaptured) call on the same
            // stream takes a slot of its own, so it can grow it and never shares the graph's buffer
            if (sl.p != nullptr && sl.dev == dev && sl.stream == st && (capturing_ || !sl.pinned)) {
                hit = &sl;
                break;
            }
            if (sl.pinned) continue;
            if (lru == nullptr || sl.p == nullptr || (lru->p != nullptr && sl.used < lru->used)) lru = &sl;
        }
        if (hit == nullptr) {
            if (lru == nullptr) return hipErrorOutOfMemory;           // every slot pinned by captures
            if (lru->p != nullptr || lru->ev != nullptr) c.drop(*lru);  // evict: waits for its event
            hit = lru;
            hit->dev = dev;
            hit->stream = st;
        }
        if (hit->cap < bytes + kTailBytes) {
            if (capturing_ || hit->pinned) return hipErrorStreamCaptureUnsupported;   // no allocation under capture
            hipError_t e = slot_wait(*hit);                // the stream's earlier launches may use it
            if (e != hipSuccess) return e;
            if (hit->p) (void)hipFree(hit->p);
            hit->p = nullptr;
            hit->cap = 0;
            const size_t cap = std::max<size_t>(bytes + kTailBytes, (size_t)1 << 20);
            e = hipMalloc(&hit->p, cap);
            if (e != hipSuccess) {
                hit->p = nullptr;
                return e;
            }
            // the tail words start at zero (tail_words: counters that their users reset themselves)
            e = hipMemsetAsync(static_cast<uint8_t*>(hit->p) + cap - kTailBytes, 0, kTailBytes, st);
            if (e != hipSuccess) {
                (void)hipFree(hit->p);
                hit->p = nullptr;
                return e;
            }
            hit->cap = cap;
            hit->tail_dirty = false;
        }
        if (hit->tail_dirty) {
            // the last call that used the tail words (the offset/length deferral counters) failed
            // between the kernel that counts up and the pass that resets them: zero them in stream
            // order before this call's launches (a stale count re-ran stale list entries)
            hipError_t e = hipMemsetAsync(static_cast<uint8_t*>(hit->p) + hit->cap - kTailBytes, 0, kTailBytes, st);
            if (e != hipSuccess) return e;
            hit->tail_dirty = false;
        }
        if (ordered && hit->ev_live && !capturing_ && hipEventQuery(hit->ev) == hipErrorNotReady) {
            hipError_t e = hipStreamWaitEvent(st, hit->ev, 0);
            if (e != hipSuccess) return e;
        }
        if (hit->ev == nullptr && !capturing_ && ordered) {
            hipError_t e = hipEventCreateWithFlags(&hit->ev, hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        hit->used = ++c.tick;
        if (capturing_) hit->pinned = true;
        if (!ordered) hit->unordered = true;
        slot_ = hit;
        return hipSuccess;
    }
    void* ptr() const { return slot_ ? slot_->p : nullptr; }
    // The slot's last kTailBytes, past every request (zeroed when the slot is allocated): words that
    // outlive a call — the offset/length deferral counter, which the deferred pass resets to zero.
    // Handing them out marks the slot dirty until tail_reset_enqueued(): a call that fails before its
    // resetting pass is enqueued leaves them to be zeroed by the next acquire() of the slot.
    uint32_t* tail_words() const {
        if (slot_ == nullptr) return nullptr;
        slot_->tail_dirty = true;
        return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(slot_->p) + slot_->cap - kTailBytes);
    }
    void tail_reset_enqueued() {
        if (slot_) slot_->tail_dirty = false;
    }
    // A tag no earlier call on this slot used (a deferral word holding it was written by this call;
    // after 2^32 calls a stale word may match once, which only repeats an idempotent pass).
    uint32_t next_tag() {
        if (++slot_->seq == 0u) slot_->seq = 1u;
        return slot_->seq;
    }
    hipError_t end() {
        ScratchSlot* sl = slot_;
        slot_ = nullptr;
        if (sl == nullptr || capturing_ || !ordered_) return hipSuccess;
        const hipError_t e = hipEventRecord(sl->ev, stream_);
        sl->ev_live = e == hipSuccess;
        return e;
    }
    ~ScratchLease() { (void)end(); }

private:
    ScratchSlot* slot_ = nullptr;
    hipStream_t  stream_ = nullptr;
    bool         capturing_ = false;
    bool         ordered_ = true;
};

// ---- ring plans (netcsum_pktstream.hip pkt_plan_block): the form and run length the last batch on a
// ring sampled for the next one. The words live in one pinned, coherent, device-mapped allocation per
// device that is never freed (a launch still in flight may store into its word after its thread has
// gone); each thread keeps a small table of its rings, each with a word and a tag (a word reused for
// another ring, or a late store of an evicted one, carries another tag and is ignored).
constexpr uint32_t kPlanWords = 4096u;
struct PlanPool {
    std::once_flag once;
    uint32_t* h = nullptr;
    uint32_t* d = nullptr;
};
PlanPool g_plan_pool[kMaxDev];
std::atomic<uint32_t> g_plan_next{0};
struct RingPlan {
    int dev = -1;
    const void* base = nullptr;
    uint64_t stride = 0;
    uint32_t pkt_len = 0, n = 0, slot = 0, tag = 0, plan = 0, use = 0, calls = 0;
    int ip_ver = -1;
    uint32_t plan_id = 0;
};
constexpr int kRingPlans = 16;
thread_local RingPlan tls_ring_plans[kRingPlans];
thread_local uint32_t tls_ring_clock = 0;
constexpr uint32_t kPlanAheadRing = 1u << 22;
constexpr uint32_t kPlanAheadPool = 1u << 19;

// The plan the ring's previous batch left (0: none yet), its word (host and device addresses) and tag
// for this batch's plan block; *d_word = nullptr when no pool could be had (the batch then runs
// without a plan block).
static uint32_t ring_plan(uint32_t plan_id, int dev, const void* base, uint64_t stride, uint32_t pkt_len, uint32_t n,
                          int ip_ver, uint32_t** h_word, uint32_t** d_word, uint32_t* tag, uint32_t* calls) {
    *h_word = *d_word = nullptr;
    if (dev < 0 || dev >= kMaxDev) return 0u;
    PlanPool& pool = g_plan_pool[dev];
    std::call_once(pool.once, [&]() {
        void* h = nullptr;
        void* dp = nullptr;
        if (hipHostMalloc(&h, kPlanWords * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        if (hipHostGetDevicePointer(&dp, h, 0) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        std::memset(h, 0, kPlanWords * sizeof(uint32_t));
        pool.h = static_cast<uint32_t*>(h);
        pool.d = static_cast<uint32_t*>(dp);
    });
    if (pool.h == nullptr) return 0u;
    RingPlan* e = nullptr;
    RingPlan* lru = &tls_ring_plans[0];
    for (RingPlan& r : tls_ring_plans) {
        if (r.dev == dev && r.base == base && r.stride == stride && r.pkt_len == pkt_len && r.n == n && r.ip_ver == ip_ver &&
            r.plan_id == plan_id) {
            e = &r;
            break;
        }
        if (r.use < lru->use) lru = &r;
    }
    if (e == nullptr) {                                     // a new ring: a fresh word and tag
        e = lru;
        const uint32_t k = g_plan_next.fetch_add(1u);
        *e = RingPlan{};
        e->dev = dev;
        e->base = base;
        e->stride = stride;
        e->pkt_len = pkt_len;
        e->n = n;
        e->ip_ver = ip_ver;
        e->plan_id = plan_id;
        e->slot = k % kPlanWords;
        e->tag = (k / kPlanWords * 2654435761u + k) & 0x7FFFu;
    }
    e->use = ++tls_ring_clock;
    if (calls != nullptr) *calls = e->calls++;
    const uint32_t w = *reinterpret_cast<volatile uint32_t*>(pool.h + e->slot);
    if ((w >> 31) != 0u && ((w >> 16) & 0x7FFFu) == e->tag) e->plan = w & 0xFFFFu;
    *h_word = pool.h + e->slot;
    *d_word = pool.d + e->slot;
    *tag = e->tag;
    return e->plan;
}

// Sample a plan ahead of this batch (NETCSUM_TUNE_PLAN_AHEAD): for a plan entry that has never had a
// word (its first batch), of at least `nmin` items, on a stream that is not being captured.
static bool plan_ahead(const Tune& t, hipStream_t s, uint32_t n, uint32_t nmin) {
    const int v = t.plan_ahead;
    if (v == 0 || (v < 0 && n < nmin)) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (s != nullptr && hipStreamIsCapturing(s, &cs) != hipSuccess) return false;
    return cs == hipStreamCaptureStatusNone;
}

// The plan word a sampler launch stores for `tag` (coherent host memory, system-scope store), polled:
// the plan (bits 0-15), or 0 when none arrived within limit_ms (the batch then runs unplanned).
static uint32_t wait_plan_word(uint32_t* h_word, uint32_t tag, int limit_ms = 2000) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const uint32_t w = *reinterpret_cast<volatile uint32_t*>(h_word);
        if ((w >> 31) != 0u && ((w >> 16) & 0x7FFFu) == tag) return w & 0xFFFFu;
        const auto el = std::chrono::steady_clock::now() - t0;
        if (el > std::chrono::milliseconds(limit_ms)) return 0u;
        if (el > std::chrono::microseconds(20)) std::this_thread::yield();
    }
}

}  // namespace

NET_ERR nchost::launch_batch(const Tune& t, const netcsum::SegBatchArgs& a0, uint32_t len_hint, hipStream_t s) {
    int dev = 0;
    NC_HIP(hipGetDevice(&dev));
    netcsum::LaunchCfg c = choose_cfg(t, dev, a0, len_hint);
    netcsum::SegBatchArgs a = a0;
    const int tile_k = t.tile;
    const bool fixed = c.run_bytes == 0u && tile_k >= 1 && tile_k <= 64;    // TUNE_TILE: fixed runs, both forms
    if (c.kernel == 6 && a.seg_off != nullptr && (c.run_bytes != 0u || fixed)) {
        // The batch's plan (varlen_runlen_kernel / the live kernel's sampler block, keyed on its
        // descriptor arrays like the packet rings' plans). Segments with gaps between them — one per
        // pool buffer — in address order take the live-sector stream (plan 3: seg_live_varlen_kernel,
        // the plan's run length and depth; TUNE_TILE 1..64 / TUNE_CHUNKS 4 or 8 override them), which
        // samples the descriptors again in one extra block, so the plan follows the descriptors from
        // batch to batch. Pools too sparse for it take the lane-group pipe form (16 lanes x 6 chunks
        // for >= 1 KiB segments, 8 x 8 for shorter ones), every 4th batch the stream form with the
        // sampler again (a plan left by other descriptors at the same addresses lasts at most 3
        // batches; the sampler costs a 1-block launch, ≈ 5 µs).
        uint32_t* h_word = nullptr;
        uint32_t* d_word = nullptr;
        uint32_t tag = 0u, calls = 0u;
        uint32_t plan = ring_plan(t.plan_id, dev, a.base, reinterpret_cast<uint64_t>(a.seg_off), 0xFFFFFFFEu, a.n_seg,
                                  -2, &h_word, &d_word, &tag, &calls);
        const char* ahead = "";
        if (plan == 0u && calls == 0u && d_word != nullptr && !fixed && plan_ahead(t, s, a.n_seg, kPlanAheadPool)) {
            // the first batch on these descriptors: the sampler alone, waited for, so that this batch
            // already runs in its plan (a one-block launch and a poll of the word)
            ScratchLease word;
            NC_HIP(word.acquire(dev, s, 256u, false));
            uint32_t* run = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(word.ptr()) + 128);
            *reinterpret_cast<volatile uint32_t*>(h_word) = 0u;
            NC_HIP(netcsum::launch_varlen_runlen(a.seg_off, a.seg_len_v, a.n_seg, a.pseudo ? a.pseudo_len : 0u, c.run_bytes,
                                                 c.stream_spw, run, d_word, tag, s));
            NC_HIP(word.end());
            plan = wait_plan_word(h_word, tag);
            ahead = " ahead";
            calls = 1u;                                   // (the pipe form below may use its plan at once)
        }
        if ((plan & 3u) == 3u && d_word != nullptr && t.kernel == 0 && t.group == 0) {
            const int ch = t.chunks;
            const uint32_t spw = fixed ? (uint32_t)tile_k : std::min<uint32_t>(64u, std::max<uint32_t>(1u, (plan >> 8) & 0xFFu));
            const int depth = (ch == 4 || ch == 8) ? ch : ((plan & 4u) ? 8 : 4);
            a.plan_out = d_word;
            a.plan_tag = tag;
            NC_HIP(netcsum::launch_live_varlen(t, a, depth, spw, s));
            char d[192];
            snprintf(d, sizeof d, "seg_live_varlen_kernel<D=%d%s,nt> block=256 segs_per_wave=%u plan=pool(live)%s", depth,
                     (a.pseudo && a.pseudo_len) ? ",pseudo" : "", spw, ahead);
            netcsum::set_last_launch(d);
            return NET_UTIL_ERR_NONE;
        }
        if (!fixed && (plan & 3u) != 0u && (plan & 3u) != 3u && (calls & 3u) != 0u && t.kernel == 0 && t.group == 0 &&
            t.chunks == 0) {                 // (any of those tuned: the form asked for)
            Tune pipe = t;                                // the caller's options with the pipe form's geometry
            pipe.kernel = 2;
            pipe.group = (plan & 3u) == 1u ? 16 : 8;      // plan 1: >= 1 KiB segments, 2: shorter
            pipe.chunks = (plan & 3u) == 1u ? 6 : 8;
            const netcsum::LaunchCfg cp = choose_cfg(pipe, dev, a0, len_hint);
            NC_HIP(netcsum::launch_seg_batch(pipe, a, cp, s));
            char d[192];
            snprintf(d, sizeof d, "%s plan=pool(pipe)%s", NetUtil_MI355X_LastLaunch(), ahead);
            netcsum::set_last_launch(d);
            return NET_UTIL_ERR_NONE;
        }
        // adaptive varlen runs: a one-block kernel samples the lengths and leaves the run length in
        // this stream's scratch word, which the batch kernel reads (stream order; any value is safe:
        // the kernel never runs shorter runs than its grid covers), and the plan for the next batch
        // (at +128 of the slot's reserved 256-B header: the lane-group walk pass keeps its deferral word
        // at +0; the packet stream's Tx records and deferred-run list start at +256)
        ScratchLease word;
        NC_HIP(word.acquire(dev, s, 256u, false));
        uint32_t* run = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(word.ptr()) + 128);
        NC_HIP(netcsum::launch_varlen_runlen(a.seg_off, a.seg_len_v, a.n_seg, a.pseudo ? a.pseudo_len : 0u, c.run_bytes,
                                             c.stream_spw, run, d_word, tag, s));
        a.run_dev = fixed ? nullptr : run;                 // (fixed runs: the sampler for the plan only)
        NC_HIP(netcsum::launch_seg_batch(t, a, c, s));
        NC_HIP(word.end());
        return NET_UTIL_ERR_NONE;
    }
    NC_HIP(netcsum::launch_seg_batch(t, a, c, s));
    return NET_UTIL_ERR_NONE;
}

// The SegBatchArgs of a strided (seg_off == nullptr) or offset/length segment batch.
netcsum::SegBatchArgs nchost::seg_args(const void* base, const uint64_t* seg_off, const uint16_t* seg_len_v, uint64_t seg_stride,
                               uint32_t seg_len, const void* pseudo, uint32_t pseudo_stride, uint32_t pseudo_len,
                               uint32_t n_seg, NETCSUM_OP op, void* out) {
    netcsum::SegBatchArgs a{};
    a.base = static_cast<const uint8_t*>(base);
    a.seg_off = seg_off;
    a.seg_len_v = seg_len_v;
    a.seg_stride = seg_stride;
    a.seg_len = seg_len;
    a.pseudo = (pseudo_len != 0) ? static_cast<const uint8_t*>(pseudo) : nullptr;
    a.pseudo_stride = pseudo_stride;
    a.pseudo_len = pseudo_len;
    a.n_seg = n_seg;
    a.verify = (op == NETCSUM_OP_DATA_VERIFY || op == NETCSUM_OP_HDR_VERIFY) ? 1u : 0u;
    a.out = out;
    return a;
}

extern "C" {

NET_ERR NetUtil_MI355X_ChkSumBatchStrided(const void* d_seg, uint64_t seg_stride, CPU_INT16U seg_len,
                                          const void* d_pseudo, uint32_t pseudo_stride, CPU_INT16U pseudo_len,
                                          uint32_t n_seg, void* d_out, NETCSUM_OP op, void* hip_stream) {
    NET_ERR e = check_op(op, d_pseudo, pseudo_len);
    if (e != NET_UTIL_ERR_NONE) return e;
    if (n_seg == 0) return NET_UTIL_ERR_NONE;
    if (n_seg > 0x7FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (d_out == nullptr || (d_seg == nullptr && seg_len != 0)) return NET_ERR_FAULT_NULL_PTR;
    return launch_batch(tls_tune, seg_args(d_seg, nullptr, nullptr, seg_stride, seg_len, d_pseudo, pseudo_stride, pseudo_len,
                                           n_seg, op, d_out),
                        seg_len, static_cast<hipStream_t>(hip_stream));
}

NET_ERR NetUtil_MI355X_ChkSumBatchVarLen(const void* d_base, const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                         const void* d_pseudo, uint32_t pseudo_stride, CPU_INT16U pseudo_len,
                                         uint32_t n_seg, void* d_out, NETCSUM_OP op, void* hip_stream) {
    NET_ERR e = check_op(op, d_pseudo, pseudo_len);
    if (e != NET_UTIL_ERR_NONE) return e;
    if (n_seg == 0) return NET_UTIL_ERR_NONE;
    if (n_seg > 0x7FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (d_out == nullptr || d_base == nullptr || d_seg_off == nullptr || d_seg_len == nullptr) {
        return NET_ERR_FAULT_NULL_PTR;
    }
    return launch_batch(tls_tune, seg_args(d_base, d_seg_off, d_seg_len, 0, 0, d_pseudo, pseudo_stride, pseudo_len, n_seg, op,
                                           d_out),
                        0u, static_cast<hipStream_t>(hip_stream));
}

NET_ERR NetUtil_MI355X_ThreadRelease(void) {
    host_release();
    tls_scratch.release_all();
    return NET_UTIL_ERR_NONE;
}

NET_ERR NetUtil_MI355X_CRC32BatchStrided(const void* d_base, uint64_t stride, uint32_t len, uint32_t n,
                                         uint32_t* d_out, int cpl, void* hip_stream) {
    if (n == 0) return NET_UTIL_ERR_NONE;
    if (d_out == nullptr || (d_base == nullptr && len != 0)) return NET_ERR_FAULT_NULL_PTR;
    netcsum::CrcBatchArgs a{};
    a.base = static_cast<const uint8_t*>(d_base);
    a.stride = stride;
    a.len = len;
    a.n = n;
    a.cpl = cpl ? 1u : 0u;
    a.out = d_out;
    netcsum::set_last_launch(netcsum::crc_launch_name(tls_tune, len, false));
    int dev = 0;
    NC_HIP(hipGetDevice(&dev));
    NC_HIP(netcsum::launch_crc_batch(tls_tune, a, len, cu_count(dev), static_cast<hipStream_t>(hip_stream)));
    return NET_UTIL_ERR_NONE;
}

NET_ERR NetUtil_MI355X_CRC32BatchVarLen(const void* d_base, const uint64_t* d_off, const uint32_t* d_len, uint32_t n,
                                        uint32_t* d_out, int cpl, void* hip_stream) {
    if (n == 0) return NET_UTIL_ERR_NONE;
    if (d_out == nullptr || d_base == nullptr || d_off == nullptr || d_len == nullptr) return NET_ERR_FAULT_NULL_PTR;
    netcsum::CrcBatchArgs a{};
    a.base = static_cast<const uint8_t*>(d_base);
    a.off = d_off;
    a.lens = d_len;
    a.n = n;
    a.cpl = cpl ? 1u : 0u;
    a.out = d_out;
    netcsum::set_last_launch(netcsum::crc_launch_name(tls_tune, 0xFFFFFFFFu, true));
    int dev = 0;
    NC_HIP(hipGetDevice(&dev));
    NC_HIP(netcsum::launch_crc_batch(tls_tune, a, 0xFFFFFFFFu, cu_count(dev), static_cast<hipStream_t>(hip_stream)));
    return NET_UTIL_ERR_NONE;
}

// The ring's plan for a batch pkt_decide marked plan_ring: looks it up (sampling it ahead of the
// ring's first batch where NETCSUM_TUNE_PLAN_AHEAD says so), gives the launch its plan word, and where
// the plan is one this batch can run in, takes its form and run length.
static NET_ERR pkt_ring_plan(const Tune& t, const PktJob& j, int dev, PktPlan& p) {
    netcsum::PktBatchArgs& a = p.a;
    uint32_t* h_word = nullptr;
    uint32_t* d_word = nullptr;
    uint32_t tag = 0u, calls = 0u;
    uint32_t plan = j.off ? ring_plan(t.plan_id, dev, j.base, reinterpret_cast<uint64_t>(j.off), 0xFFFFFFFFu, j.n, j.ip_ver,
                                      &h_word, &d_word, &tag, &calls)
                          : ring_plan(t.plan_id, dev, j.base, j.stride, j.pkt_len, j.n, j.ip_ver, &h_word, &d_word, &tag,
                                      &calls);
    if (d_word == nullptr) return NET_UTIL_ERR_NONE;
    a.plan = p.run0 | ((uint32_t)p.cap << 8) | (tag << 16);
    a.plan_out = d_word;
    if (plan == 0u && calls == 0u && plan_ahead(t, j.stream, j.n, kPlanAheadRing)) {
        // the ring's first batch: its sampler alone, waited for
        *reinterpret_cast<volatile uint32_t*>(h_word) = 0u;
        NC_HIP(netcsum::launch_pkt_plan(a, j.ip_ver, j.stream));
        plan = wait_plan_word(h_word, tag);
        p.ahead_note = " ahead";
    }
    const uint32_t form = plan & 0x7u, pw = (plan >> 4) & 0xFu, prun = (plan >> 8) & 0xFFu;
    if (plan != 0u && j.off != nullptr) {
        p.vl_wide = (plan & 8u) != 0u;
        p.vl_inline = !p.vl_wide && ((plan >> 4) & 0xFu) != 0u;   // (the plan's reduced residency)
    }
    if (plan != 0u && form == 0u && p.run0 != 0u && prun == p.run0) {
        p.bound = 0;
        p.spw = p.run0;
        p.plan_note = " plan=ring(form0)";
    } else if (plan != 0u && form == 2u && prun >= 1u && prun <= p.cap && (pw == 0u || (pw >= 3u && pw <= 8u))) {
        p.bound = 2;
        p.spw = prun;
        a.res_waves = pw;
        p.plan_note = pw ? (pw == 5u ? " plan=ring(live,5 waves)" : pw == 6u ? " plan=ring(live,6 waves)"
                                                                   : " plan=ring(live,waves)")
                         : " plan=ring(live)";
    } else {
        p.plan_note = " plan=first";
    }
    return NET_UTIL_ERR_NONE;
}

extern "C++" {
NET_ERR nchost::pkt_batch(const Tune& t, const PktJob& j) {
    if (j.n == 0) return NET_UTIL_ERR_NONE;
    if (j.n > 0x7FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (j.base == nullptr || (j.off != nullptr) != (j.len != nullptr) || (!j.tx && j.flags == nullptr && j.action == nullptr)) {
        return NET_ERR_FAULT_NULL_PTR;
    }
    if (j.sums != nullptr && (j.tx || j.ip_ver != 0)) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;   // (Rx, mixed)
    int dev = 0;
    NC_HIP(hipGetDevice(&dev));
    PktPlan p;
    NET_ERR e = pkt_decide(t, j, p);
    if (e != NET_UTIL_ERR_NONE) return e;
    netcsum::PktBatchArgs& a = p.a;
    hipStream_t hs = j.stream;
    if (p.stream) {
        if (p.plan_ring) {
            e = pkt_ring_plan(t, j, dev, p);
            if (e != NET_UTIL_ERR_NONE) return e;
        }
        pkt_settle(t, j, p);
        netcsum::set_last_launch(p.desc);
        // scratch slot layout (one slot per (thread, device, stream), shared by every batch kind on the
        // stream, which stream order keeps apart): [0, 256) the words that must survive other calls'
        // data — +0 the lane-group walk pass's deferral word (tagged), +128 the varlen run word — then,
        // from +256, the records of two-pass Tx and, after them, offset/length batches' deferred-run list
        // (one index per run the stream kernel could not stream in order); the list's counters (count,
        // blocks done) are the slot's tail words, which the deferred pass leaves zero
        const size_t rec_bytes = (p.two && j.rec_only == nullptr) ? (size_t)j.n * sizeof(netcsum::PktTxRecord) : 0u;
        const size_t defer_bytes = (j.off && !p.vl_inline) ? (4u * (((size_t)j.n + p.spw - 1u) / p.spw) + 15u) & ~(size_t)15u : 0u;
        constexpr size_t kHdr = 256u;
        ScratchLease scratch;
        if (rec_bytes + defer_bytes) NC_HIP(scratch.acquire(dev, hs, kHdr + rec_bytes + defer_bytes));
        if (j.off && !p.vl_inline) {
            a.vl_list = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(scratch.ptr()) + kHdr + rec_bytes);
            a.vl_ctr = scratch.tail_words();
            a.vl_wide = p.vl_wide ? 1u : 0u;
        }
        netcsum::PktTxRecord* recs = rec_bytes ? reinterpret_cast<netcsum::PktTxRecord*>(static_cast<uint8_t*>(scratch.ptr()) + kHdr)
                                               : nullptr;
        if (j.rec_only != nullptr) {                      // zero-copy Tx burst: records only, no scatter
            NC_HIP(netcsum::launch_pkt_stream(t, a, j.ip_ver, p.d, p.spw, p.snt, j.tx, p.bound, hs, j.rec_only, false));
        } else {
            NC_HIP(netcsum::launch_pkt_stream(t, a, j.ip_ver, p.d, p.spw, p.snt, j.tx, p.bound, hs, p.two ? recs : nullptr));
        }
        if (a.vl_ctr != nullptr) scratch.tail_reset_enqueued();   // (launch_pkt_stream enqueued the deferred pass)
        NC_HIP(scratch.end());
        return NET_UTIL_ERR_NONE;
    }
    if (j.rec_only != nullptr) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;   // (callers check the domain)
    char desc[120];
    snprintf(desc, sizeof desc, "pkt_batch_kernel<G=%d,K=%d%s,%s,v%d%s> block=256 tile=%u%s", p.c.group_lanes,
             p.c.chunks_per_pass, p.c.nt ? ",nt" : "", j.tx ? "tx" : "rx", j.ip_ver, !j.tx && a.sums_out ? ",sums" : "", a.tile,
             p.walk ? " +pkt_v6_walk_kernel" : "");
    netcsum::set_last_launch(desc);
    ScratchLease scratch;                                 // [deferral word, 256 B | flags (own_flags)]
    if (p.walk) {
        NC_HIP(scratch.acquire(dev, hs, 256u + (p.own_flags ? j.n : 0u)));
        a.defer_word = static_cast<uint32_t*>(scratch.ptr());
        a.defer_tag = scratch.next_tag();
        if (p.own_flags) a.flags_out = static_cast<uint8_t*>(scratch.ptr()) + 256u;
    }
    NC_HIP(netcsum::launch_pkt_batch(a, p.c, j.tx, j.ip_ver, hs));
    if (p.walk) NC_HIP(netcsum::launch_pkt_v6_walk(a, j.tx, cu_count(dev), hs));
    NC_HIP(scratch.end());
    return NET_UTIL_ERR_NONE;
}

// The public packet entry points' job: the arguments they share.
PktJob nchost::pkt_job(const void* base, const uint64_t* off, const uint16_t* len, uint64_t stride, CPU_INT16U pkt_len,
                      uint32_t n, uint8_t* flags, void* hip_stream) {
    PktJob j;
    j.base = base;
    j.off = off;
    j.len = len;
    j.stride = stride;
    j.pkt_len = pkt_len;
    j.n = n;
    j.flags = flags;
    j.stream = static_cast<hipStream_t>(hip_stream);
    return j;
}
}  // extern "C++"

NET_ERR NetUtil_MI355X_ChkSumBatchChains(const void* d_base, const uint64_t* d_piece_off,
                                        const uint16_t* d_piece_len, const uint32_t* d_chain_first,
                                        const void* d_pseudo, uint32_t pseudo_stride, CPU_INT16U pseudo_len,
                                        uint32_t n_chains, void* d_out, NETCSUM_OP op, void* hip_stream) {
    if (op != NETCSUM_OP_DATA_CALC && op != NETCSUM_OP_DATA_VERIFY) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (n_chains == 0) return NET_UTIL_ERR_NONE;
    if (n_chains > 0x7FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (d_out == nullptr || d_chain_first == nullptr || d_piece_off == nullptr || d_piece_len == nullptr ||
        (d_pseudo == nullptr && pseudo_len != 0)) {
        return NET_ERR_FAULT_NULL_PTR;
    }
    const Tune& t = tls_tune;
    int dev = 0;
    NC_HIP(hipGetDevice(&dev));
    netcsum::ChainBatchArgs a{};
    a.base = static_cast<const uint8_t*>(d_base);
    a.off = d_piece_off;
    a.len = d_piece_len;
    a.first = d_chain_first;
    a.pseudo = (pseudo_len != 0) ? static_cast<const uint8_t*>(d_pseudo) : nullptr;
    a.pseudo_stride = pseudo_stride;
    a.pseudo_len = pseudo_len;
    a.n = n_chains;
    a.verify = (op == NETCSUM_OP_DATA_VERIFY) ? 1u : 0u;
    a.out = d_out;
    // GROUP_LANES 16/32/64: chain_batch_kernel with that many lanes per chain; KERNEL 1: the
    // wave-per-chain kernel (4 chains per 256-thread block); otherwise (auto) the two-pass form
    // (per-piece sums in piece order, then a combine pass per chain), its records in this thread's
    // scratch for this stream: room for max(2^20, 128 x chains) pieces (a batch with more pieces is
    // done by the wave-per-chain form inside the combine pass).
    int g = t.group;
    g = (g == 16 || g == 32 || g == 64) ? g : 0;
    // The records are capped at 2^24 pieces (128 MiB per thread and stream): a larger batch runs its
    // pieces past the cap in the wave-per-chain form inside pass 1, and a thread whose scratch cannot
    // be allocated (or is pinned by a stream capture) takes the wave-per-chain kernel instead.
    if (g == 0 && t.kernel != 1) {
        const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(1ull << 20, 128ull * n_chains), 1ull << 24);
        const int kern = t.kernel;
        // the default (0) and 5: one record per piece (4 B); 3 the round-5 live form, others the tiled
        // 16-lane groups (both 8 B per piece)
        const bool one_rec = kern == 0 || kern == 5;
        ScratchLease scratch;
        if (scratch.acquire(dev, static_cast<hipStream_t>(hip_stream), (size_t)cap * (one_rec ? 4u : 8u)) == hipSuccess) {
            // pass 1: tiled 16-lane groups, or with TUNE_KERNEL 3 the live-sector stream in runs of 16
            // pieces (TUNE_TILE 1..64 sets the run, TUNE_CHUNKS 4 the depth) — 0.1993-0.2046 ms on the
            // chain row against 0.1756-0.1803 for the groups (profiles/r5v_chains.log: two wave totals
            // per piece end, the byte and the half-word sums, cost more than the sectors save there)
            // Default / TUNE_KERNEL 5 (round 6): the segment live-sector stream with ONE wave total per piece
            // end, the piece's half-word sum, combined modulo 65535 (chain_combine_h_kernel)
            const int tk = t.tile, ch = t.chunks;
            // runs: TUNE_TILE, else 16 pieces (round 5's live form) / 12 (the one-record form: 0.1686-0.1691
            // ms on the chain row against 0.1709-0.1715 for 16, profiles/r6v_*, r6w_*)
            const uint32_t live = (kern != 3 && !one_rec) ? 0u : (tk >= 1 && tk <= 64) ? (uint32_t)tk : one_rec ? 12u : 16u;
            const int depth = ch == 4 ? 4 : 8;
            char d[128];
            if (one_rec) {
                const bool cmp = netcsum::live_compact(t);
                const int cl = t.chain_combine == 64 ? 64 : 16;
                snprintf(d, sizeof d, "seg_live_varlen_kernel<D=%d,chain,nt%s> pieces_per_wave=%u +chain_combine_h_kernel<%d>",
                         depth, cmp ? ",compact" : "", live, cl);
                netcsum::set_last_launch(d);
                NC_HIP(netcsum::launch_chain_two_pass_h(t, a, static_cast<uint32_t*>(scratch.ptr()), (uint32_t)cap, cu_count(dev),
                                                        static_cast<hipStream_t>(hip_stream), live, depth, cmp, cl));
                NC_HIP(scratch.end());
                return NET_UTIL_ERR_NONE;
            }
            if (live) {
                snprintf(d, sizeof d, "chain_live_piece_kernel<D=%d,nt> pieces_per_wave=%u +chain_combine_kernel", depth, live);
            } else {
                snprintf(d, sizeof d, "chain_piece_kernel<G=16,K=6,tile=64,nt> +chain_combine_kernel");
            }
            netcsum::set_last_launch(d);
            NC_HIP(netcsum::launch_chain_two_pass(t, a, static_cast<uint64_t*>(scratch.ptr()), (uint32_t)cap, cu_count(dev),
                                                  static_cast<hipStream_t>(hip_stream), live, depth));
            NC_HIP(scratch.end());
            return NET_UTIL_ERR_NONE;
        }
        (void)hipGetLastError();                          // a failed allocation is not this launch's error
    }
    netcsum::set_last_launch(g ? "chain_batch_kernel" : "chain_wave_kernel");
    const uint32_t gpb = g ? 256u / (uint32_t)g : 4u;
    const uint64_t need = ((uint64_t)n_chains + gpb - 1u) / gpb;
    int grid = t.grid;
    if (grid <= 0) grid = (int)std::min<uint64_t>(need, (uint64_t)cu_count(dev) * (g ? 16u : 64u));
    NC_HIP(netcsum::launch_chain_batch(a, g, grid, static_cast<hipStream_t>(hip_stream)));
    return NET_UTIL_ERR_NONE;
}

NET_ERR NetUtil_MI355X_RxValidateIPv4(const void* d_base, const uint64_t* d_off, const uint16_t* d_len,
                                      uint64_t stride, CPU_INT16U pkt_len, uint32_t n_pkt, uint8_t* d_flags,
                                      void* hip_stream) {
    PktJob j = pkt_job(d_base, d_off, d_len, stride, pkt_len, n_pkt, d_flags, hip_stream);
    j.ip_ver = 4;
    return pkt_batch(tls_tune, j);
}

NET_ERR NetUtil_MI355X_TxFinalizeIPv4(void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                                      CPU_INT16U pkt_len, uint32_t n_pkt, uint8_t* d_flags, int udp_tx_csum,
                                      void* hip_stream) {
    PktJob j = pkt_job(d_base, d_off, d_len, stride, pkt_len, n_pkt, d_flags, hip_stream);
    j.ip_ver = 4;
    j.tx = true;
    j.udp_mode = udp_tx_csum ? 1u : 0u;
    return pkt_batch(tls_tune, j);
}

NET_ERR NetUtil_MI355X_RxValidateIPv6(const void* d_base, const uint64_t* d_off, const uint16_t* d_len,
                                      uint64_t stride, CPU_INT16U pkt_len, uint32_t n_pkt, uint8_t* d_flags,
                                      void* hip_stream) {
    PktJob j = pkt_job(d_base, d_off, d_len, stride, pkt_len, n_pkt, d_flags, hip_stream);
    j.ip_ver = 6;
    return pkt_batch(tls_tune, j);
}

NET_ERR NetUtil_MI355X_RxValidateIP(const void* d_base, const uint64_t* d_off, const uint16_t* d_len,
                                    uint64_t stride, CPU_INT16U pkt_len, uint32_t n_pkt, uint8_t* d_flags,
                                    void* hip_stream) {
    return pkt_batch(tls_tune, pkt_job(d_base, d_off, d_len, stride, pkt_len, n_pkt, d_flags, hip_stream));
}

NET_ERR NetUtil_MI355X_TxFinalizeIPv6(void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                                      CPU_INT16U pkt_len, uint32_t n_pkt, uint8_t* d_flags, int udp_tx_csum,
                                      void* hip_stream) {
    PktJob j = pkt_job(d_base, d_off, d_len, stride, pkt_len, n_pkt, d_flags, hip_stream);
    j.ip_ver = 6;
    j.tx = true;
    j.udp_mode = udp_tx_csum ? 1u : 0u;
    return pkt_batch(tls_tune, j);
}

NET_ERR NetUtil_MI355X_TxFinalizeIP(void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                                    CPU_INT16U pkt_len, uint32_t n_pkt, uint8_t* d_flags, int udp_tx_csum,
                                    void* hip_stream) {
    PktJob j = pkt_job(d_base, d_off, d_len, stride, pkt_len, n_pkt, d_flags, hip_stream);
    j.tx = true;
    j.udp_mode = udp_tx_csum ? 1u : 0u;
    return pkt_batch(tls_tune, j);
}

// Burst adapters of the reference's checksum-offload seam (include/netcsum_mi355x.h (2b'')): the mixed
// IPv4 / IPv6 kernels with the action written beside each verdict (Rx) and the per-datagram UDP policy
// of the offload's 0xFFFF placeholder (Tx).
NET_ERR NetUtil_MI355X_RxBurst(const void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                               CPU_INT16U pkt_len, uint32_t n_pkt, uint32_t rx_cfg, uint8_t* d_action, uint8_t* d_flags,
                               void* hip_stream) {
    if (n_pkt != 0 && d_action == nullptr) return NET_ERR_FAULT_NULL_PTR;
    if (rx_cfg & ~(uint32_t)NETCSUM_RXCFG_UDP_DISCARD_NO_CHK_SUM) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    PktJob j = pkt_job(d_base, d_off, d_len, stride, pkt_len, n_pkt, d_flags, hip_stream);
    j.action = d_action;
    j.rx_cfg = rx_cfg;
    return pkt_batch(tls_tune, j);
}

// RxBurst with the per-frame fragment payload sums (the SUMS instantiations of the same kernels, in the
// launch RxBurst would have chosen): RxBurst's checks first, then d_sums.
NET_ERR NetUtil_MI355X_RxBurstSums(const void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                                   CPU_INT16U pkt_len, uint32_t n_pkt, uint32_t rx_cfg, uint8_t* d_action, uint8_t* d_flags,
                                   NETCSUM_FRAG_SUM* d_sums, void* hip_stream) {
    if (n_pkt != 0 && d_action == nullptr) return NET_ERR_FAULT_NULL_PTR;
    if (rx_cfg & ~(uint32_t)NETCSUM_RXCFG_UDP_DISCARD_NO_CHK_SUM) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    const NET_ERR e = check_frag_sums(d_sums, n_pkt);
    if (e != NET_UTIL_ERR_NONE) return e;
    PktJob j = pkt_job(d_base, d_off, d_len, stride, pkt_len, n_pkt, d_flags, hip_stream);
    j.action = d_action;
    j.rx_cfg = rx_cfg;
    j.sums = d_sums;
    return pkt_batch(tls_tune, j);
}

// The demux step both Ether device forms open with, and its end. begin(): one lease of the stream's scratch
// for the demux and the packet batch behind it — `below` bytes that pkt_batch leases in the same slot for
// its own layouts, then the datagrams' offsets and lengths — and the demux arguments with the frames and
// those outputs filled (the direction adds its own and launches). end(), after pkt_batch's launches: the
// lease ends and LastLaunch gets "<name> b=<blocks> | " in front.
struct EtherDemux {
    ScratchLease            scratch;
    netcsum::EtherDemuxArgs a{};

    NET_ERR begin(size_t below, const void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                  CPU_INT16U frame_len, uint32_t n_frame, uint8_t* d_l2, hipStream_t hs) {
        int dev = 0;
        NC_HIP(hipGetDevice(&dev));
        const size_t n = n_frame;
        const size_t o_off = (below + 255u) & ~(size_t)255u;
        const size_t o_len = (o_off + 8u * n + 255u) & ~(size_t)255u;
        NC_HIP(scratch.acquire(dev, hs, o_len + 2u * n));
        uint8_t* sp = static_cast<uint8_t*>(scratch.ptr());
        a.base = static_cast<const uint8_t*>(d_base);
        a.off = d_off;
        a.len = d_len;
        a.stride = stride;
        a.len_u = frame_len;
        a.n = n_frame;
        a.l2_out = d_l2;
        a.off_out = reinterpret_cast<uint64_t*>(sp + o_off);
        a.len_out = reinterpret_cast<uint16_t*>(sp + o_len);
        return NET_UTIL_ERR_NONE;
    }
    NET_ERR end(const char* name) {
        NC_HIP(scratch.end());
        char desc[256];
        snprintf(desc, sizeof desc, "%s b=%u | %.220s", name, netcsum::ether_demux_blocks(a.n), netcsum::last_launch());
        netcsum::set_last_launch(desc);
        return NET_UTIL_ERR_NONE;
    }
};

// Rx burst of Ethernet frames: the 802.x demux pass (netcsum_ether.hip) writes each frame's class and the
// offset/length descriptor of its IP datagram into this thread's scratch for the stream, then RxBurst's
// offset/length batch runs over the descriptors, unchanged. The lease is taken once, for both steps, and
// ends after the packet launches: pkt_batch leases the same slot for its own scratch (Rx offset/length:
// 256 B of words, then at most 4 B per frame of deferred-run list, or one flag byte per frame for the
// walk pass), which fits below the descriptors, so its lease never grows the buffer under them. Under
// stream capture the rule is the Tx records': the slot is pinned, and a capture needs one uncaptured
// call of at least its size first.
// d_sums (RxBurstEtherSums; checked by the entry point): the packet batch is RxBurstSums' — the SUMS
// instantiations of the same launch. It leases what RxBurst's does and nothing more: its deferred-run list is
// the same list, and a datagram that waits for the walk is marked in d_sums itself (kFragSumWalk), not in
// scratch; the lane-group form's own flags (one byte per frame) are the other case, below 4 B per frame too.
// So the descriptors lie above all of it, as they do without sums (pkt_batch's layouts: 256 + 4 n + 16 at most).
// sums: the call is RxBurstEtherSums, whose d_sums is checked after RxBurstEther's own arguments (RxBurstSums'
// checks); n_frame 0 succeeds without a launch.
static NET_ERR rx_burst_ether(const void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                              CPU_INT16U frame_len, uint32_t n_frame, uint32_t rx_cfg, uint32_t eth_cfg,
                              const uint8_t* hw_addr, uint8_t* d_action, uint8_t* d_flags, uint8_t* d_l2, bool sums,
                              NETCSUM_FRAG_SUM* d_sums, void* hip_stream) {
    NET_ERR e = check_rx_ether(d_base, d_action, d_l2, n_frame, rx_cfg, eth_cfg);
    if (e == NET_UTIL_ERR_NONE && sums) e = check_frag_sums(d_sums, n_frame);
    if (e != NET_UTIL_ERR_NONE) return e;
    if (n_frame == 0) return NET_UTIL_ERR_NONE;
    if (n_frame > 0x7FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    hipStream_t hs = static_cast<hipStream_t>(hip_stream);
    EtherDemux x;
    e = x.begin(256u + 4u * (size_t)n_frame + 16u, d_base, d_off, d_len, stride, frame_len, n_frame, d_l2, hs);   // past pkt_batch's own scratch
    if (e != NET_UTIL_ERR_NONE) return e;
    x.a.eth_cfg = eth_cfg;
    pack_hw_addr(hw_addr, &x.a.have_hw, &x.a.hw_lo, &x.a.hw_hi);
    NC_HIP(netcsum::launch_ether_demux(x.a, hs));
    PktJob j = pkt_job(d_base, x.a.off_out, x.a.len_out, 0, 0, n_frame, d_flags, hip_stream);
    j.action = d_action;
    j.rx_cfg = rx_cfg;
    j.sums = d_sums;
    e = pkt_batch(tls_tune, j);
    if (e != NET_UTIL_ERR_NONE) return e;
    return x.end("ether_demux");
}

NET_ERR NetUtil_MI355X_RxBurstEther(const void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                                    CPU_INT16U frame_len, uint32_t n_frame, uint32_t rx_cfg, uint32_t eth_cfg,
                                    const uint8_t* hw_addr, uint8_t* d_action, uint8_t* d_flags, uint8_t* d_l2,
                                    void* hip_stream) {
    return rx_burst_ether(d_base, d_off, d_len, stride, frame_len, n_frame, rx_cfg, eth_cfg, hw_addr, d_action, d_flags, d_l2,
                          false, nullptr, hip_stream);
}

NET_ERR NetUtil_MI355X_RxBurstEtherSums(const void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                                        CPU_INT16U frame_len, uint32_t n_frame, uint32_t rx_cfg, uint32_t eth_cfg,
                                        const uint8_t* hw_addr, uint8_t* d_action, uint8_t* d_flags, uint8_t* d_l2,
                                        NETCSUM_FRAG_SUM* d_sums, void* hip_stream) {
    return rx_burst_ether(d_base, d_off, d_len, stride, frame_len, n_frame, rx_cfg, eth_cfg, hw_addr, d_action, d_flags, d_l2,
                          true, d_sums, hip_stream);
}

// Tx burst of Ethernet frames: the Tx demux pass (netcsum_ether.hip ether_tx_demux_kernel) writes each
// frame's class and the offset/length descriptor of the datagram behind its Ethernet II header into this
// thread's scratch for the stream, then TxBurst's offset/length batch runs over the descriptors,
// unchanged. One lease for both steps, as RxBurstEther's, but the descriptors sit past everything
// pkt_batch leases in the same slot for a Tx batch: the 256-B header, the two-pass form's 8-B record per
// frame and the deferred-run list (at most 4 B per frame + 16). The capture rule is the Tx records'.
// d_fieldpos / d_rec (the host-memory form's chunks; both or neither, d_fieldpos zeroed by the caller):
// the fields each datagram had written, gathered into 8-B records while the descriptors are leased.
extern "C++" NET_ERR nchost::tx_burst_ether(const Tune& t, void* d_base, const uint64_t* d_off, const uint16_t* d_len,
                                            uint64_t stride, CPU_INT16U frame_len, uint32_t n_frame, uint8_t* d_flags,
                                            uint8_t* d_l2, hipStream_t hs, uint32_t* d_fieldpos, uint64_t* d_rec) {
    if (n_frame != 0 && (d_l2 == nullptr || d_base == nullptr)) return NET_ERR_FAULT_NULL_PTR;
    if (n_frame > 0x7FFFFFFFu) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    if (n_frame == 0) return NET_UTIL_ERR_NONE;
    EtherDemux x;
    NET_ERR e = x.begin(256u + 8u * (size_t)n_frame + 4u * (size_t)n_frame + 16u, d_base, d_off, d_len, stride, frame_len,
                        n_frame, d_l2, hs);                  // past pkt_batch's own Tx scratch
    if (e != NET_UTIL_ERR_NONE) return e;
    NC_HIP(netcsum::launch_ether_tx_demux(x.a, hs));
    PktJob j = pkt_job(d_base, x.a.off_out, x.a.len_out, 0, 0, n_frame, d_flags, hs);
    j.tx = true;
    j.udp_mode = 2u;
    j.fieldpos = d_fieldpos;
    e = pkt_batch(t, j);
    if (e != NET_UTIL_ERR_NONE) return e;
    if (d_rec != nullptr) {
        netcsum::PktBatchArgs g{};
        g.base = static_cast<const uint8_t*>(d_base);
        g.off = x.a.off_out;
        g.n = n_frame;
        g.fieldpos_out = d_fieldpos;
        NC_HIP(netcsum::launch_pkt_field_gather(g, d_rec, hs));
    }
    return x.end("ether_tx_demux");
}

NET_ERR NetUtil_MI355X_TxBurstEther(void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                                    CPU_INT16U frame_len, uint32_t n_frame, uint8_t* d_flags, uint8_t* d_l2,
                                    void* hip_stream) {
    return tx_burst_ether(tls_tune, d_base, d_off, d_len, stride, frame_len, n_frame, d_flags, d_l2,
                          static_cast<hipStream_t>(hip_stream), nullptr, nullptr);
}

uint8_t NetUtil_MI355X_RxAction(uint8_t flags, uint8_t proto, int ipv6, uint32_t rx_cfg) {
    return (uint8_t)netcsum::rx_action(flags, proto, ipv6 != 0, rx_cfg);
}

NET_ERR NetUtil_MI355X_TxBurst(void* d_base, const uint64_t* d_off, const uint16_t* d_len, uint64_t stride,
                               CPU_INT16U pkt_len, uint32_t n_pkt, uint8_t* d_flags, void* hip_stream) {
    PktJob j = pkt_job(d_base, d_off, d_len, stride, pkt_len, n_pkt, d_flags, hip_stream);
    j.tx = true;
    j.udp_mode = 2u;
    return pkt_batch(tls_tune, j);
}

NET_ERR NetUtil_MI355X_Fill(void* d_buf, uint64_t n_bytes, uint64_t first_byte, uint64_t seed, int pattern,
                            void* hip_stream) {
    if (n_bytes == 0) return NET_UTIL_ERR_NONE;
    if (d_buf == nullptr) return NET_ERR_FAULT_NULL_PTR;
    if (((uintptr_t)d_buf & 7u) != 0u || pattern < 0 || pattern > 3) {
        return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    }
    int dev = 0;
    NC_HIP(hipGetDevice(&dev));
    const uint64_t words = (n_bytes >> 3) + 1u;
    const uint64_t cap = (uint64_t)cu_count(dev) * 8u;
    const int grid = (int)std::max<uint64_t>(1u, std::min<uint64_t>((words + 255u) / 256u, cap));
    NC_HIP(netcsum::launch_fill(d_buf, n_bytes, first_byte, seed, pattern, grid, static_cast<hipStream_t>(hip_stream)));
    return NET_UTIL_ERR_NONE;
}

NET_ERR NetUtil_MI355X_ReadStream(const void* d_buf, uint64_t n_bytes, uint64_t* d_sink, void* hip_stream) {
    if (n_bytes == 0) return NET_UTIL_ERR_NONE;
    if (d_buf == nullptr || d_sink == nullptr) return NET_ERR_FAULT_NULL_PTR;
    if (((uintptr_t)d_buf & 15u) != 0u || (n_bytes & 15u) != 0u) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    const Tune& t = tls_tune;
    int dev = 0;
    NC_HIP(hipGetDevice(&dev));
    if (t.probe >= 2) {                     // run-stream form (netcsum_stream.hip); 3: with a pause per piece
        NC_HIP(netcsum::launch_read_run(t, d_buf, n_bytes, reinterpret_cast<unsigned long long*>(d_sink),
                                        static_cast<hipStream_t>(hip_stream), t.probe == 3));
        return NET_UTIL_ERR_NONE;
    }
    int grid = t.grid;
    if (grid <= 0) grid = cu_count(dev) * 32;
    NC_HIP(netcsum::launch_read_stream(d_buf, n_bytes / 16u, reinterpret_cast<unsigned long long*>(d_sink), grid,
                                       t.nt != 0, static_cast<hipStream_t>(hip_stream), t.probe));
    return NET_UTIL_ERR_NONE;
}

NET_ERR NetUtil_MI355X_PlanBind(uint32_t plan_id) {
    tls_tune.plan_id = plan_id;
    return NET_UTIL_ERR_NONE;
}

// NetUtil_MI355X_Tune as a table: per key the accepted values (a range, or a listed set), a
// normalisation of the accepted value where the key has one, and the field of the calling thread's Tune
// it is stored in.
namespace {
constexpr int kEnd = INT_MIN;                           // ends a row's value set
struct TuneRow {
    int key;
    int lo, hi;                                         // accepted range, unless
    int set[9];                                         // set[0] != kEnd: the accepted values, kEnd-terminated
    int Tune::*field;                                   // stored here
    int (*norm)(int);                                   // applied first to an accepted value (nullptr: as given)
};
const TuneRow kTuneRows[] = {
    {NETCSUM_TUNE_GRID_BLOCKS, 0, INT_MAX, {kEnd}, &Tune::grid, nullptr},
    {NETCSUM_TUNE_GROUP_LANES, 0, 0, {0, 1, 4, 8, 16, 32, 64, kEnd}, &Tune::group, nullptr},
    {NETCSUM_TUNE_NT_LOADS, INT_MIN, INT_MAX, {kEnd}, &Tune::nt, [](int v) { return v < 0 ? -1 : (int)(v != 0); }},
    {NETCSUM_TUNE_BLOCK_THREADS, 0, 0, {0, 64, 128, 256, kEnd}, &Tune::block,   // __launch_bounds__(256)
     [](int v) { return v == 0 ? 256 : v; }},
    {NETCSUM_TUNE_KERNEL, 0, 8, {kEnd}, &Tune::kernel, nullptr},
    {NETCSUM_TUNE_CHUNKS, 0, 0, {0, 1, 2, 3, 4, 6, 8, kEnd}, &Tune::chunks, nullptr},
    {NETCSUM_TUNE_PROBE, 0, 3, {kEnd}, &Tune::probe, nullptr},
    {NETCSUM_TUNE_GRID_MULT, 0, 64, {kEnd}, &Tune::grid_mult, [](int v) { return v == 0 ? 1 : v; }},
    {NETCSUM_TUNE_TILE, -1, 1 << 20, {kEnd}, &Tune::tile, nullptr},
    {NETCSUM_TUNE_TX_PASSES, 0, 2, {kEnd}, &Tune::tx_passes, nullptr},
    {NETCSUM_TUNE_STREAM_WAVES, 0, 0, {-1, 0, 3, 4, 5, 6, 7, 8, kEnd}, &Tune::stream_waves, nullptr},
    {NETCSUM_TUNE_STREAM_TOUCH, -1, 1, {kEnd}, &Tune::stream_touch, nullptr},
    {NETCSUM_TUNE_STREAM_XCD, -1, 4096, {kEnd}, &Tune::stream_xcd, nullptr},
    {NETCSUM_TUNE_TX_FLUSH, -1, 4, {kEnd}, &Tune::tx_flush, nullptr},
    {NETCSUM_TUNE_CRC_KERNEL, 0, 3, {kEnd}, &Tune::crc_kernel, nullptr},
    {NETCSUM_TUNE_CRC_NT, 0, 1, {kEnd}, &Tune::crc_nt, nullptr},
    {NETCSUM_TUNE_CRC_LANES, 0, 0, {0, 1, 2, 4, 8, 16, kEnd}, &Tune::crc_lanes, nullptr},
    {NETCSUM_TUNE_CRC_WIDE, 0, 2, {kEnd}, &Tune::crc_wide, nullptr},
    {NETCSUM_TUNE_HDR_BURST, -1, 1, {kEnd}, &Tune::hdr_burst, nullptr},
    {NETCSUM_TUNE_VARLEN_RUN_BYTES, -1, 1 << 20, {kEnd}, &Tune::varlen_run_bytes, nullptr},
    {NETCSUM_TUNE_PKT_BOUND, -1, 4, {kEnd}, &Tune::pkt_bound, nullptr},
    {NETCSUM_TUNE_BURST_ZERO_COPY, 0, 3, {kEnd}, &Tune::burst_zc, nullptr},
    {NETCSUM_TUNE_BURST_SERVER_IDLE_US, 1, 1000000, {kEnd}, &Tune::burst_idle, nullptr},
    {NETCSUM_TUNE_BURST_SERVER_LIFE_US, 1, 1000000, {kEnd}, &Tune::burst_life, nullptr},
    {NETCSUM_TUNE_PLAN_AHEAD, -1, 1, {kEnd}, &Tune::plan_ahead, nullptr},
    {NETCSUM_TUNE_LIVE_COMPACT, -1, 1, {kEnd}, &Tune::live_compact, nullptr},
    {NETCSUM_TUNE_STORE_GATHER, -1, 1, {kEnd}, &Tune::store_gather, nullptr},
    {NETCSUM_TUNE_CHAIN_GRID, -1, 16, {kEnd}, &Tune::chain_grid, nullptr},
    {NETCSUM_TUNE_CHAIN_COMBINE, 0, 0, {-1, 16, 64, kEnd}, &Tune::chain_combine, nullptr},
};
}  // namespace

NET_ERR NetUtil_MI355X_Tune(int key, int value) {
    // Not a setting, so not in Tune: a one-shot flag the test arms (1) or disarms (0) and the next deferred
    // pass consumes, kept beside that launcher (netcsum_pktstream.hip launch_vl_deferred).
    if (key == NETCSUM_TUNE_FAULT_INJECT) {
        if (value != 0 && value != 1) return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
        netcsum::set_fault_skip_deferred(value == 1);
        return NET_UTIL_ERR_NONE;
    }
    for (const TuneRow& r : kTuneRows) {
        if (r.key != key) continue;
        bool ok = r.set[0] == kEnd && value >= r.lo && value <= r.hi;
        for (int i = 0; !ok && r.set[0] != kEnd && r.set[i] != kEnd; ++i) ok = r.set[i] == value;
        if (!ok) break;
        tls_tune.*r.field = r.norm ? r.norm(value) : value;
        return NET_UTIL_ERR_NONE;
    }
    return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
}

const char* NetUtil_MI355X_LastLaunch(void) {
    return netcsum::last_launch();
}

const char* NetUtil_MI355X_Version(void) {
    return "netcsum-mi355x 0.1.0 gfx950";
}

}  // extern "C"
