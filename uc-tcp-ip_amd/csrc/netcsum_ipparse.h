// netcsum_ipparse.h — the IP datagram parse and verdict rules of the packet kernels, stated once:
// which IPv4 / IPv6 datagrams are MALFORMED, FRAGMENT, L4_MALFORMED, UDP_NO_CSUM or EXT_HDR, where the
// transport checksum field sits, which pseudo-header applies, and what the folded sums mean (Rx
// verdict bits, Tx field values). The run-stream kernels (netcsum_pktstream.hip), the lane-group
// kernels (netcsum_packets.hip) and the extension-header walk (netcsum_v6walk.h) all call these
// functions; each supplies a small WINDOW ACCESSOR over the bytes it holds:
//     uint32_t limit() const;                       octets of the datagram readable without a dependent load
//     template <int MinOff> uint32_t dword(uint32_t off) const;
//                                                   little-endian dword at datagram offset off >= 16 * MinOff
// and keeps its own arithmetic (which sums it takes, from which registers) next to the call.
// Internal (not part of the ABI). C++17; __host__ __device__ under hipcc, plain C++ under g++
// (tests/c_ipparse/ipparse_caller.cpp runs the rules on the CPU).
//
// The reference lines the rules follow:
//   IPv4 header   version, IHL, total length vs. octets received          net_ipv4.c:5123-5254
//                 fragments (MF or offset != 0): IP verdict only           net_ipv4.c:6523
//                 Tx header checksum over a zeroed field, memcpy'd         net_ipv4.c:9573-9586
//   IPv6 header   40-B fixed header, payload length vs. octets received    net_ipv6.c:8290-8360
//                 extension headers, length (HdrExtLen + 1) * 8            net_ipv6.c:8396-8510, 8601
//                 Routing: type <= 2 or Segments Left 0 accepted           net_ipv6.c:8735-8753
//                 upper-layer length = payload - extension octets          net_ipv6.c:5682
//                 pseudo-header {src, dst, length (32), 0, next header}    net_ipv6.h:844-852
//   TCP           length >= 20; DataVerify / DataCalc + pseudo             net_tcp.c:7808-7818, 7851-7879, 29824-29862
//   UDP           length field == datagram length                          net_udp.c:1893-1907
//                 Rx field 0 = no checksum, accepted                       net_udp.c:1916-1920, 1947-1957, 1971
//                 Tx 0 -> 0xFFFF; checksums disabled -> 0                  net_udp.c:2891-2937
//   ICMPv4 / IGMP no pseudo-header                                         net_icmpv4.c:1676, 2204; net_igmp.c:1332, 1692
//   ICMPv6        Rx types 1, 3, 4: the message alone (HdrVerify)          net_icmpv6.c:2910-2920
//                 Rx types 128-131, 134-137: DataVerify + pseudo           net_icmpv6.c:2923-2942
//                 Rx other types: rejected before any checksum             net_icmpv6.c:2945-2948
//                 Tx every type through the pseudo-header, no 0 -> 0xFFFF  net_icmpv6.c:949-965, 1439
#pragma once

#include <stdint.h>

#include "../../include/netcsum_mi355x.h"

#if defined(__HIPCC__)
#include "netcsum_kernels.h"
#define NETCSUM_IP_FN __host__ __device__ __forceinline__
#else
#define NETCSUM_IP_FN static inline
#endif

namespace netcsum {

#if !defined(__HIPCC__)
// (netcsum_kernels.h, a HIP header, holds this for the library; the host-only build has no other copy)
NETCSUM_IP_FN bool udp_tx_compute(uint32_t mode, uint32_t field) { return mode == 1u || (mode == 2u && field != 0u); }
#endif

namespace ip {

NETCSUM_IP_FN uint32_t be16(uint32_t dw, int byte) {            // bytes byte, byte + 1 of dw, big-endian
    return (((dw >> (8 * byte)) & 0xFFu) << 8) | ((dw >> (8 * byte + 8)) & 0xFFu);
}

NETCSUM_IP_FN uint32_t swap16(uint32_t x) { return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu); }

NETCSUM_IP_FN uint32_t halfwords(uint32_t dw, uint32_t acc) {   // acc + the two half-words of dw
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u16(dw, 0u, acc);
#else
    return acc + (dw & 0xFFFFu) + (dw >> 16);
#endif
}

NETCSUM_IP_FN bool ext_hdr_value(uint32_t nh) {                 // net_ipv6.h NET_IP_HDR_PROTOCOL_EXT_*
    return nh == 0u || nh == 43u || nh == 44u || nh == 50u || nh == 51u || nh == 59u || nh == 60u ||
           nh == 135u || nh == 139u || nh == 140u || nh == 253u || nh == 254u;
}

// What the rules decide about one datagram before any sum is known.
struct Class {
    uint32_t flags;        // NETCSUM_PKT_* known from the parse (verdict() adds the checksum bits)
    uint32_t proto;        // transport protocol (IPv6: the last next-header value read)
    uint32_t l4_off;       // transport offset: IPv4 header length; IPv6 40 + walked headers (40 until the
                           // chain has been walked to a transport header; 0: malformed IPv4)
    uint32_t tot;          // datagram length by its own header
    uint32_t l4_csum_off;  // datagram offset of the transport checksum field (~0u: none)
    uint32_t pseudo_le;    // pseudo: little-endian word sum of the pseudo-header's words that are not
                           // datagram octets next to the transport part (IPv4: all of it; IPv6: length
                           // and next header, the addresses [8, 40) being summed with the transport part)
    uint32_t frag_off;     // FRAGMENT: the payload's offset and octets (RxBurstSums; len 0: nothing to
    uint32_t frag_len;     // sum, or frag_walk)
    bool     v6;
    bool     check_l4;     // a transport checksum is verified (Rx) / computed (Tx) over [l4_off, tot)
    bool     pseudo;       // ... with the pseudo-header
    bool     frag_walk;    // IPv6 fragment whose Fragment header ends past the window: the walk sums it
};

NETCSUM_IP_FN bool malformed(const Class& c) { return (c.flags & NETCSUM_PKT_MALFORMED) != 0u; }

// The transport step at c.l4_off of a datagram of c.tot octets, next header c.proto: shape checks, the
// checksum field, whether and with which pseudo-header it is checked. addr_le: IPv4, the addresses'
// half-word sum (IPv6: 0).
template <bool TX, bool V6, int MinOff, class W>
NETCSUM_IP_FN void transport(const W& w, uint32_t udp_mode, uint32_t addr_le, Class& c) {
    const uint32_t nh = c.proto, off = c.l4_off;
    const uint32_t ulen = c.tot - off;                           // upper-layer length (< 2^16)
    // the pseudo-header's {0, protocol, length} words (IPv6: the length's high half is 0) and addr_le
    const auto with_pseudo = [&]() {
        c.check_l4 = c.pseudo = true;
        c.pseudo_le = addr_le + (nh << 8) + swap16(ulen);
    };
    switch (nh) {
    case 6u:                                                     // TCP
        if (ulen < 20u) {
            c.flags |= NETCSUM_PKT_L4_MALFORMED;
            return;
        }
        with_pseudo();
        c.l4_csum_off = off + 16u;
        break;
    case 17u: {                                                  // UDP: length | checksum
        if (ulen < 8u) {
            c.flags |= NETCSUM_PKT_L4_MALFORMED;
            return;
        }
        const uint32_t du = w.template dword<MinOff>(off + 4u);
        if (be16(du, 0) != ulen) {
            c.flags |= NETCSUM_PKT_L4_MALFORMED;
            return;
        }
        c.l4_csum_off = off + 6u;
        if (!TX && (du >> 16) == 0u) {                           // no checksum transmitted
            c.flags |= NETCSUM_PKT_UDP_NO_CSUM | NETCSUM_PKT_L4_OK;
            return;
        }
        if (TX && !udp_tx_compute(udp_mode, du >> 16)) {
            c.flags |= NETCSUM_PKT_UDP_NO_CSUM;                  // verdict(): write 0 (NET_UDP_HDR_CHK_SUM_NONE)
            return;
        }
        with_pseudo();
        break;
    }
    case 1u:                                                     // ICMPv4 / IGMP: no pseudo-header
    case 2u:
        if (V6) {
            return;
        }
        if (ulen < 4u) {
            c.flags |= NETCSUM_PKT_L4_MALFORMED;
            return;
        }
        c.check_l4 = true;
        c.l4_csum_off = off + 2u;
        break;
    case 58u:                                                    // ICMPv6
        if (!V6) {
            return;
        }
        if (ulen < 4u) {
            c.flags |= NETCSUM_PKT_L4_MALFORMED;
            return;
        }
        c.l4_csum_off = off + 2u;
        if constexpr (TX) {
            with_pseudo();
        } else {
            const uint32_t type = w.template dword<MinOff>(off) & 0xFFu;
            if (type == 1u || type == 3u || type == 4u) {
                c.check_l4 = true;                               // the message alone
            } else if ((type >= 128u && type <= 131u) || (type >= 134u && type <= 137u)) {
                with_pseudo();
            }
        }
        break;
    default:
        break;
    }
}

// The IPv4 addresses' half-word sum (header dwords 3 and 4), the transport step's addr_le.
NETCSUM_IP_FN uint32_t addr4_le(uint32_t d3, uint32_t d4) { return halfwords(d3, halfwords(d4, 0u)); }

// IPv4 from the header's five dwords (the caller holds them: it sums the header from them) and, for
// the transport fields, the window; `avail` octets present. TRANSPORT false: the header step alone
// (MALFORMED, FRAGMENT, or l4_off / tot / proto for a transport step the caller runs itself).
template <bool TX, int MinOff, class W, bool TRANSPORT = true>
NETCSUM_IP_FN Class classify4(const W& w, uint32_t avail, uint32_t udp_mode, uint32_t d0, uint32_t d1, uint32_t d2,
                              uint32_t d3, uint32_t d4) {
    Class c{};
    c.l4_csum_off = ~0u;
    const uint32_t ver = (d0 >> 4) & 0xFu;
    const uint32_t hlen = (d0 & 0xFu) * 4u;
    c.tot = be16(d0, 2);
    const uint32_t frag = be16(d1, 2) & 0x3FFFu;                 // MF | fragment offset
    c.proto = (d2 >> 8) & 0xFFu;
    if (avail < 20u || ver != 4u || hlen < 20u || c.tot < hlen || c.tot > avail) {
        c.flags = NETCSUM_PKT_MALFORMED;
        return c;
    }
    c.l4_off = hlen;
    if (frag != 0u) {
        c.flags = NETCSUM_PKT_FRAGMENT;
        c.frag_off = hlen;
        c.frag_len = c.tot - hlen;
        return c;
    }
    if constexpr (TRANSPORT) {
        transport<TX, false, MinOff>(w, udp_mode, addr4_le(d3, d4), c);
    }
    return c;
}

// IPv6 from the fixed header's first two dwords and the window. Routing headers the reference accepts
// are walked here, up to 4 of them, while the chain and the transport fields stay inside the window;
// Hop-by-Hop / Destination Options headers (whose options NetIPv6_RxOptHdr walks), any other routing
// header, a chain past the window and every other extension header get EXT_HDR: the walk pass
// (netcsum_v6walk.h) then judges the datagram. An extension header running past the payload is
// MALFORMED (the reference has no such check and reads on).
template <bool TX, int MinOff, class W>
NETCSUM_IP_FN Class classify6(const W& w, uint32_t avail, uint32_t udp_mode, uint32_t d0, uint32_t d1) {
    Class c{};
    c.l4_csum_off = ~0u;
    c.v6 = true;
    c.tot = 40u + be16(d1, 0);
    c.proto = (d1 >> 16) & 0xFFu;
    c.l4_off = 40u;
    if (avail < 40u || ((d0 >> 4) & 0xFu) != 6u || c.tot > avail) {
        c.flags = NETCSUM_PKT_MALFORMED;
        return c;
    }
    const uint32_t limit = w.limit();
    uint32_t off = 40u;
    for (int e = 0; e < 4 && c.proto == 43u; ++e) {
        if (off + 8u > limit) {
            c.flags = NETCSUM_PKT_EXT_HDR;
            return c;
        }
        const uint32_t d = w.template dword<MinOff>(off);
        if (((d >> 16) & 0xFFu) > 2u && (d >> 24) != 0u) {
            c.flags = NETCSUM_PKT_EXT_HDR;
            return c;
        }
        off += (((d >> 8) & 0xFFu) + 1u) * 8u;
        c.proto = d & 0xFFu;
        if (off > c.tot) {                                       // extension header past the payload
            c.flags = NETCSUM_PKT_MALFORMED;
            return c;
        }
    }
    if (c.proto == 44u) {
        c.flags = NETCSUM_PKT_FRAGMENT;
        if (off + 8u < c.tot) {                                  // octets after the 8-B Fragment header
            if (off + 8u <= limit) {
                c.frag_off = off + 8u;
                c.frag_len = c.tot - (off + 8u);
            } else {
                c.frag_walk = true;
            }
        }
        return c;
    }
    if (ext_hdr_value(c.proto) || (off != 40u && off + 24u > limit)) {
        c.flags = NETCSUM_PKT_EXT_HDR;
        return c;
    }
    c.l4_off = off;
    transport<TX, true, MinOff>(w, udp_mode, 0u, c);
    return c;
}

// What the folded sums mean. sip: the IPv4 header's (IPv6: unused); sl4: the transport part's with the
// pseudo-header added; both 16-bit, 0xFFFF when the received checksum verifies. Tx: the sums are taken
// with the checksum fields counted as zero, and cip / cl4 are the host-order values to store at
// offset 10 / c.l4_csum_off (~0u: store nothing).
struct Verdict {
    uint32_t flags, cip, cl4;
};

template <bool TX>
NETCSUM_IP_FN Verdict verdict(const Class& c, uint32_t sip, uint32_t sl4) {
    Verdict v{c.flags, ~0u, ~0u};
    if (malformed(c)) {
        return v;
    }
    if constexpr (!TX) {
        v.flags |= (c.v6 || sip == 0xFFFFu) ? NETCSUM_PKT_IP_OK : 0u;   // IPv6: well-formed (no header checksum)
        if (c.check_l4) {
            v.flags |= NETCSUM_PKT_L4_CHECKED | ((sl4 == 0xFFFFu) ? NETCSUM_PKT_L4_OK : 0u);
        }
    } else {
        v.cip = c.v6 ? ~0u : ((~sip) & 0xFFFFu);
        v.flags |= NETCSUM_PKT_IP_OK;
        if (c.check_l4) {
            v.cl4 = (~sl4) & 0xFFFFu;
            if (c.proto == 17u && v.cl4 == 0u) {
                v.cl4 = 0xFFFFu;                                 // RFC 768
            }
            v.flags |= NETCSUM_PKT_L4_CHECKED | NETCSUM_PKT_L4_OK;
        } else if ((c.flags & NETCSUM_PKT_UDP_NO_CSUM) && c.l4_csum_off != ~0u) {
            v.cl4 = 0u;                                          // UDP checksums disabled
        }
    }
    return v;
}

}  // namespace ip
}  // namespace netcsum
