// netcsum_v6walk.h — the IPv6 extension-header walk of one datagram by a 16-lane group (walk_one),
// shared by the walk pass (netcsum_v6walk.hip, after the Tx and lane-group batch kernels) and by the
// run-stream Rx kernel (netcsum_pktstream.hip), which finishes its own deferred datagrams at the end
// of each run. The chain's rules are here (netcsum_v6walk.hip describes the pass); the transport and
// verdict rules after the chain are netcsum_ipparse.h's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "netcsum_device.h"
#include "netcsum_ipparse.h"
#include "netcsum_kernels.h"

namespace netcsum {
namespace v6walk {

// The datagram's octets as the rules' accessor (netcsum_ipparse.h): every octet is one load away, so
// the window is the whole datagram; octets at or past its end read as 0.
struct ByteWindow {
    const uint8_t* p;
    uint32_t       tot;
    __device__ __forceinline__ uint32_t limit() const { return tot; }
    template <int MinOff>
    __device__ __forceinline__ uint32_t dword(uint32_t off) const {
        uint32_t d = 0u;
#pragma unroll
        for (uint32_t k = 0u; k < 4u; ++k) {
            d |= (off + k < tot ? (uint32_t)p[off + k] : 0u) << (8u * k);
        }
        return d;
    }
};

// NetIPv6_RxOptHdr's option walk (net_ipv6.c:8604-8672) over a Hop-by-Hop / Destination Options
// header h of eh_len octets: an option whose type & 0x1F is not Pad1 (0), PadN (1) or Router Alert
// (5) and whose action bits (type & 0xC0) are not "skip" (0x00) drops the datagram
// (NET_IPv6_ERR_INVALID_EH_OPT); Pad1 advances one octet, every other option Len + 2. An option that
// starts at the header's last octet would have its Len read one past the header, but any value ends
// the walk there, so that octet is not read. Group-uniform byte loads (one cached line per 64 B).
__device__ __forceinline__ bool options_accept(const uint8_t* h, uint32_t eh_len) {
    for (uint32_t nto = 0u; nto + 2u < eh_len;) {
        const uint32_t t = h[2u + nto];
        const uint32_t opt = t & 0x1Fu;
        if (opt != 0u && opt != 1u && opt != 5u && (t & 0xC0u) != 0u) {
            return false;
        }
        nto += (opt == 0u) ? 1u : ((nto + 3u < eh_len ? (uint32_t)h[3u + nto] : 0u) + 2u);
    }
    return true;
}

// NetIPv6_RxRoutingHdr (net_ipv6.c:8735-8753): routing types 0, 1, 2 pass; any other type drops the
// datagram (NET_IPv6_ERR_INVALID_EH_OPT_SEQ) unless Segments Left is 0.
__device__ __forceinline__ bool routing_accepts(const uint8_t* h) {
    return h[2] <= 2u || h[3] == 0u;
}

// A datagram is finished by a group of kLanes lanes (a wave takes 4 datagrams at a time).
constexpr uint32_t kLanes = 16u;

// Ones'-complement sum, in big-endian half-words of the datagram, of its bytes [lo, hi) (lo even; an
// odd last octet padded with zero), the half-word at `skip` (even, or ~0u) counted as zero, folded to
// 16 bits (0 iff every counted octet is 0). The group's lanes read whole aligned 16-B chunks (bytes
// outside [lo, hi) masked; a chunk never leaves the 16-B block, hence the page, of a datagram byte)
// and add their little-endian half-words with v_sad_u16: with the datagram at an even address those
// are the big-endian ones byte-swapped, at an odd address they ARE the big-endian ones (RFC 1071 §2).
__device__ __forceinline__ uint32_t group_sum(const uint8_t* p, uint32_t lo, uint32_t hi, uint32_t skip, uint32_t lane) {
    const uintptr_t s0 = (uintptr_t)p + lo, e0 = (uintptr_t)p + hi;
    uint32_t s = 0u;
    for (uintptr_t c = (s0 & ~(uintptr_t)15u) + 16u * lane; c < e0; c += 16u * kLanes) {
        const u32x4 v = *reinterpret_cast<gu32x4*>(c);
        s = sum4(mask_chunk(v, (int)((intptr_t)s0 - (intptr_t)c), (int)((intptr_t)e0 - (intptr_t)c)), s);
    }                                               // <= 258 chunks of 8 half-words per lane
#pragma unroll
    for (int o = (int)kLanes / 2; o > 0; o >>= 1) {
        s += (uint32_t)__shfl_xor((int)s, o, (int)kLanes);
    }                                               // < 2^32: 32 788 half-words at most
    const uint32_t odd = (uint32_t)((uintptr_t)p & 1u);
    if (skip != ~0u) {                              // exact: those two octets were added above
        s -= ((uint32_t)p[skip] << (8u * odd)) + ((uint32_t)p[skip + 1u] << (8u * (odd ^ 1u)));
    }
    const uint32_t r = fold16(s);
    return odd ? r : rot8(r);
}

// A lane group finishes datagram i (all values below are uniform in the group; lane = its lane).
// SUMS (Rx, RxBurstSums): the group also writes the datagram's NETCSUM_FRAG_SUM record (A.sums_out): a
// fragment's payload [Fragment header end, tot) by the same group sum, 0 for anything else.
// walk_at: the datagram's `avail` octets at p; walk_one: datagram i of the batch's descriptors.
template <bool TX, bool SUMS = false>
__device__ __forceinline__ void walk_at(const PktBatchArgs& A, uint32_t i, uint8_t* p, uint32_t avail, uint32_t lane) {
    if (avail < 40u || (p[0] >> 4) != 6u) {
        return;                                     // not IPv6: the batch kernel's flag stands
    }
    const uint32_t tot = 40u + (((uint32_t)p[4] << 8) | (uint32_t)p[5]);
    if (tot > avail) {
        return;                                     // MALFORMED already (never EXT_HDR)
    }
    ip::Class c{};                                  // (flags: what this walk alone decides)
    c.v6 = true;
    c.tot = tot;
    c.l4_csum_off = ~0u;
    uint32_t nh = p[6], off = 40u;
    while (nh == 0u || nh == 43u || nh == 60u) {   // off grows by >= 8 per header: ends by tot
        if (nh == 0u && off != 40u) {
            c.flags = NETCSUM_PKT_EXT_HDR;          // Hop-by-Hop only first (net_ipv6.c:8307)
            break;
        }
        if (off + 8u > tot) {
            c.flags = NETCSUM_PKT_MALFORMED;        // the header would run past the payload
            break;
        }
        const uint32_t eh_len = ((uint32_t)p[off + 1u] + 1u) * 8u;
        if (off + eh_len > tot) {
            c.flags = NETCSUM_PKT_MALFORMED;        // (the reference reads on past the payload)
            break;
        }
        if (!(nh == 43u ? routing_accepts(p + off) : options_accept(p + off, eh_len))) {
            c.flags = NETCSUM_PKT_EXT_HDR;          // the reference drops the datagram here
            break;
        }
        nh = p[off];
        off += eh_len;
    }
    c.proto = nh;
    c.l4_off = off;
    uint32_t frag_rec = 0u;                         // SUMS: sum | len << 16
    if (c.flags == 0u) {
        if (nh == 44u) {
            c.flags = NETCSUM_PKT_FRAGMENT;
            if constexpr (SUMS) {
                if (tot - off > 8u) {               // octets after the 8-B Fragment header
                    // group_sum folds big-endian half-words; the record holds the host-order value
                    frag_rec = rot8(group_sum(p, off + 8u, tot, ~0u, lane)) | ((tot - off - 8u) << 16);
                }
            }
        } else if (ip::ext_hdr_value(nh)) {
            c.flags = NETCSUM_PKT_EXT_HDR;
        } else {
            ip::transport<TX, true, 0>(ByteWindow{p, tot}, A.udp_tx_csum, 0u, c);
        }
    }
    uint32_t sl4 = 0u;
    if (c.check_l4) {
        uint32_t s = group_sum(p, off, tot, TX ? c.l4_csum_off : ~0u, lane);
        if (c.pseudo) {
            s += group_sum(p, 8u, 40u, ~0u, lane);  // the addresses (folded values: no overflow)
        }
        // group_sum folds big-endian half-words; the rules take the host-order (little-endian) sum
        sl4 = fold16(rot8(fold16(s)) + c.pseudo_le);
    }
    const ip::Verdict vd = ip::verdict<TX>(c, 0u, sl4);
    const uint32_t f = vd.flags;
    if (TX && vd.cl4 != ~0u && lane == 0u) {        // memcpy of the host-order value
        p[c.l4_csum_off] = (uint8_t)(vd.cl4 & 0xFFu);
        p[c.l4_csum_off + 1u] = (uint8_t)(vd.cl4 >> 8);
        if (A.fieldpos_out) A.fieldpos_out[i] = kFieldL4 | c.l4_csum_off;
    }
    if (lane == 0u) {
        if (A.flags_out) A.flags_out[i] = (uint8_t)f;
        if (!TX && A.action_out) {
            A.action_out[i] = (uint8_t)rx_action(f, nh, true, A.rx_cfg);
        }
        if constexpr (SUMS) {
            A.sums_out[i] = frag_rec;
        }
    }
}

template <bool TX, bool SUMS = false>
__device__ __forceinline__ void walk_one(const PktBatchArgs& A, uint32_t i, uint32_t lane) {
    uint64_t off64;
    uint32_t avail;
    if (A.off) {
        off64 = A.off[i];
        avail = A.len[i];
    } else {
        off64 = (uint64_t)i * A.stride;
        avail = A.len_u;
    }
    walk_at<TX, SUMS>(A, i, const_cast<uint8_t*>(A.base) + off64, avail, lane);
}

// The calling wave's datagrams s0 + k whose lane k has `need` set, four at a time by its 16-lane
// groups (every lane of the wave must be active).
template <bool TX, bool SUMS = false>
__device__ __forceinline__ void walk_wave(const PktBatchArgs& A, uint32_t s0, bool need, uint32_t lane) {
    const uint32_t grp = lane / kLanes;
    uint64_t m = __ballot(need);                    // wave-uniform
    while (m != 0u) {                               // group g takes the g-th lowest set bit
        uint32_t j = ~0u;
#pragma unroll
        for (uint32_t g = 0; g < 64u / kLanes; ++g) {
            if (m != 0u) {
                j = (g == grp) ? (uint32_t)__builtin_ctzll(m) : j;
                m &= m - 1u;
            }
        }
        if (j != ~0u) {
            walk_one<TX, SUMS>(A, s0 + j, lane % kLanes);
        }
    }
}

// The same for a wave that keeps its datagrams' descriptors in registers and has none in memory (the
// burst server's Ether form): lane k holds datagram s0 + k's address `at` and octets present `avail`,
// and a group fetches its datagram's from lane j (ds_bpermute, by all 64 lanes: a group without a
// datagram this round reads its own lane's). SUMS: walk_at's (the datagram's record is the group's to write).
template <bool TX, bool SUMS = false>
__device__ __forceinline__ void walk_wave_regs(const PktBatchArgs& A, uint32_t s0, bool need, uint32_t lane, uintptr_t at,
                                               uint32_t avail) {
    const uint32_t grp = lane / kLanes;
    uint64_t m = __ballot(need);
    while (m != 0u) {
        uint32_t j = ~0u;
#pragma unroll
        for (uint32_t g = 0; g < 64u / kLanes; ++g) {
            if (m != 0u) {
                j = (g == grp) ? (uint32_t)__builtin_ctzll(m) : j;
                m &= m - 1u;
            }
        }
        const int src = (int)(j != ~0u ? j : lane);
        const uint64_t pj = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uint64_t)at >> 32), src, 64) << 32) |
                            (uint32_t)__shfl((int)(uint32_t)at, src, 64);
        const uint32_t aj = (uint32_t)__shfl((int)avail, src, 64);
        if (j != ~0u) {
            walk_at<TX, SUMS>(A, s0 + j, reinterpret_cast<uint8_t*>((uintptr_t)pj), aj, lane % kLanes);
        }
    }
}

}  // namespace v6walk
}  // namespace netcsum
