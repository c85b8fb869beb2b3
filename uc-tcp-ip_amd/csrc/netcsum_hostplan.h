// netcsum_hostplan.h — the host-memory batches' planning, free of HIP (a plain C++ program can include it:
// tests/c_hostplan/hostplan_caller.cpp): how a batch is cut into chunks and which octets of the caller's
// buffer each chunk spans, where the regions of a pipeline slot lie, how a chunk's descriptors are staged,
// and how the records a Tx batch returns are written into the caller's ring. netcsum_hostmem.hip decides
// from these what is copied where; nothing here touches a device.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/netcsum_ether.h"

namespace nchost {

inline size_t al256(size_t x) { return (x + 255u) & ~(size_t)255u; }

// One chunk of a host-memory batch: items [s0, s0 + ns) whose bytes are [lo, hi) of the caller's buffer.
struct HostChunk {
    uint32_t s0, ns;
    uint64_t lo, hi;
};

// Items s0 .. s0 + ns - 1 (ns >= 1) with the octets [lo, hi) they occupy from the base: item i starts at
// off[i], or at i * stride without offsets, and has len[i] octets, or fixed_len without lengths (all four
// combinations occur: a ring of slots has lengths and no offsets).
inline HostChunk chunk_span(const uint64_t* off, const uint16_t* len, uint64_t stride, uint32_t fixed_len, uint32_t s0,
                            uint32_t ns) {
    HostChunk k{s0, ns, ~0ull, 0};
    if (off == nullptr && len == nullptr) {
        k.lo = (uint64_t)s0 * stride;
        k.hi = (uint64_t)(s0 + ns - 1u) * stride + fixed_len;
        return k;
    }
    for (uint32_t i = s0; i < s0 + ns; ++i) {
        const uint64_t o = off ? off[i] : (uint64_t)i * stride;
        k.lo = std::min<uint64_t>(k.lo, o);
        k.hi = std::max<uint64_t>(k.hi, o + (len ? len[i] : fixed_len));
    }
    return k;
}

// The chunks of a batch of n items, per = ceil(n / n_chunks) items each (n_chunks clamped to [1, n]; the
// last chunk takes what is left), and the largest chunk's byte span.
struct ChunkPlan {
    std::vector<HostChunk> ch;
    uint32_t               per = 0;
    uint64_t               max_span = 0;
};

inline ChunkPlan plan_chunks(const uint64_t* off, const uint16_t* len, uint64_t stride, uint32_t fixed_len, uint32_t n,
                             uint32_t n_chunks) {
    ChunkPlan p;
    if (n == 0) return p;
    n_chunks = std::min(std::max(n_chunks, 1u), n);
    p.per = (n + n_chunks - 1u) / n_chunks;
    for (uint32_t s0 = 0; s0 < n; s0 += p.per) {
        p.ch.push_back(chunk_span(off, len, stride, fixed_len, s0, std::min(p.per, n - s0)));
        p.max_span = std::max<uint64_t>(p.max_span, p.ch.back().hi - p.ch.back().lo);
    }
    return p;
}

// The regions of one pipeline slot (a device slot or its pinned host staging), handed out in order at
// 256-B aligned offsets; a region of 0 bytes takes no room. total(): what the slot must hold.
class SlotLayout {
public:
    size_t take(size_t bytes) {
        const size_t o = end_;
        end_ += al256(bytes);
        return o;
    }
    size_t total() const { return end_; }

private:
    size_t end_ = 0;
};

// A chunk's descriptors as its copy on the device needs them: offsets counted from the chunk's lo (where
// the copy starts), lengths as they are; either array may be absent (nullptr in, nothing written).
inline void stage_descriptors(const uint64_t* off, const uint16_t* len, const HostChunk& q, uint64_t* off_out,
                              uint16_t* len_out) {
    if (off != nullptr) {
        for (uint32_t i = 0; i < q.ns; ++i) off_out[i] = off[q.s0 + i] - q.lo;
    }
    if (len != nullptr) memcpy(len_out, len + q.s0, (size_t)q.ns * 2u);
}

// ---- Tx: the checksum fields a batch computed, written into the caller's buffer by the host (the device
// never writes it). A field is the 2 octets as the device would have stored them (memcpy of the value).

// Copy pipeline: the gather pass's record of item s0 + i is rec[i] = IP value | transport value << 16 |
// position word << 32; the position word (PktBatchArgs::fieldpos_out) says which fields were written —
// kRecFieldIP: the IPv4 header checksum at +10, kRecFieldL4: the transport field at +(bits 0-15).
constexpr uint32_t kRecFieldIP = 1u << 31, kRecFieldL4 = 1u << 30;

inline void apply_field_records(uint8_t* base, const uint64_t* off, uint64_t stride, uint32_t s0, uint32_t ns,
                                const uint64_t* rec) {
    for (uint32_t i = 0; i < ns; ++i) {
        const uint64_t r = rec[i];
        const uint32_t pos = (uint32_t)(r >> 32);
        if ((pos & (kRecFieldIP | kRecFieldL4)) == 0u) continue;
        uint8_t* p = base + (off ? off[s0 + i] : (uint64_t)(s0 + i) * stride);
        const uint16_t ip = (uint16_t)r, l4 = (uint16_t)(r >> 16);
        if (pos & kRecFieldIP) memcpy(p + 10, &ip, 2);
        if (pos & kRecFieldL4) memcpy(p + (pos & 0xFFFFu), &l4, 2);
    }
}

// In-place bursts: item i's PktTxRecord is rec[i] = vals | l4_off << 32 | flags << 48 | store << 56, and its
// datagram starts hdr octets (0, or NETCSUM_L2_HDR_ETHER for a frame) into the item. Writes the fields
// (store bit 0: IP at +10, bit 1: transport at +l4_off) and the flags (optional). A datagram flagged
// NETCSUM_PKT_EXT_HDR (an IPv6 chain past the kernel's window) is left as it is and returned: its index,
// the datagram's offset from the base and its length, for the caller to finish by the copy path.
struct TxSkipped {
    std::vector<uint32_t> idx;
    std::vector<uint64_t> off;
    std::vector<uint16_t> len;
};

inline TxSkipped apply_tx_records(const uint64_t* rec, uint8_t* base, const uint64_t* off, const uint16_t* len,
                                  uint64_t stride, uint32_t fixed_len, uint32_t hdr, uint32_t n, uint8_t* flags_out) {
    TxSkipped skip;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t r = rec[i];
        const uint32_t flags = (uint32_t)(r >> 48) & 0xFFu, store = (uint32_t)(r >> 56);
        const uint64_t o = (off ? off[i] : (uint64_t)i * stride) + hdr;
        if (flags & NETCSUM_PKT_EXT_HDR) {                  // (only an IP datagram gets this flag)
            skip.idx.push_back(i);
            skip.off.push_back(o);
            skip.len.push_back((uint16_t)((len ? len[i] : fixed_len) - hdr));
            continue;
        }
        uint8_t* p = base + o;
        const uint16_t ip = (uint16_t)r, l4 = (uint16_t)(r >> 16);
        if (store & 1u) memcpy(p + 10, &ip, 2);
        if (store & 2u) memcpy(p + ((r >> 32) & 0xFFFFu), &l4, 2);
        if (flags_out) flags_out[i] = (uint8_t)flags;
    }
    return skip;
}

}  // namespace nchost
