/*
 * netcsum_ether.h — the layer-2 classification rules of NetUtil_MI355X_RxBurstEther
 * (netcsum_mi355x.h (2b'''')) and the Tx frame rule of NetUtil_MI355X_TxBurstEther ((2b'''''),
 * NetCsum_L2TxClass below), each stated once: the demux kernels (csrc/netcsum_ether.hip), the burst
 * server's Ether forms and the host logic (host/netcsum_ether.c) all include this file. Plain C99; under hipcc NETCSUM_L2_FN adds
 * __host__ __device__.
 *
 * The rules are those of the reference's 802.x receive path, in its order of checks (the first check
 * that fails names the class): NetIF_802x_Rx's frame size (IF/net_if_802x.c:548-554, :1673-1685),
 * NetIF_802x_RxPktFrameDemux's destination and source addresses and the type / length split
 * (:1982-2050), the Ethernet II types (:2155-2187), and the 802.3 length, 802.2 LLC and SNAP checks
 * (:2266-2352).
 *
 * A frame's first NETCSUM_L2_HDR_OCTETS = 23 octets decide everything: the 22 octets of the longer
 * (802.3 + LLC + SNAP) header and the first octet of an IP datagram behind either header. They are
 * passed as six little-endian 32-bit words — w[k] holds octets 4k .. 4k+3, octet 4k in bits 0-7 —
 * the form in which the kernel has them after its aligned dword loads; octet 23 (bits 24-31 of w[5])
 * is never looked at. A frame shorter than NETCSUM_L2_FRAME_MIN is classified from its length alone:
 * its words are not looked at, and callers do not read them (NetCsum_L2Words is called for longer
 * frames only).
 */
#ifndef NETCSUM_ETHER_H
#define NETCSUM_ETHER_H

#include <stdint.h>

#include "netcsum_mi355x.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define NETCSUM_L2_FN static inline __host__ __device__
#else
#define NETCSUM_L2_FN static inline
#endif

#define NETCSUM_L2_HDR_OCTETS       23u     /* octets of a frame the rules read                           */
#define NETCSUM_L2_FRAME_MIN        60u     /* NET_IF_802x_FRAME_MIN_SIZE                                 */
#define NETCSUM_L2_FRAME_MIN_CRC    64u     /* NET_IF_802x_FRAME_MIN_CRC_SIZE: the length check applies   */
#define NETCSUM_L2_LEN_OVERHEAD     18u     /* NET_IF_HDR_SIZE_ETHER + NET_IF_802x_FRAME_CRC_SIZE         */
#define NETCSUM_L2_IEEE_LEN_MAX     1500u   /* NET_IF_IEEE_802_FRAME_LEN_MAX                              */
#define NETCSUM_L2_HDR_ETHER        14u     /* NET_IF_HDR_SIZE_ETHER                                      */
#define NETCSUM_L2_HDR_SNAP         22u     /* NET_IF_HDR_SIZE_IEEE_802                                   */
#define NETCSUM_L2_TYPE_IPV4        0x0800u
#define NETCSUM_L2_TYPE_IPV6        0x86DDu
#define NETCSUM_L2_TYPE_ARP         0x0806u

/* Octet k (0 .. 22) of the frame from its words. */
NETCSUM_L2_FN uint32_t NetCsum_L2Octet(const uint32_t w[6], uint32_t k) {
    return (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu;
}

/* The big-endian 16-bit value at octets k, k + 1. */
NETCSUM_L2_FN uint32_t NetCsum_L2Net16(const uint32_t w[6], uint32_t k) {
    return (NetCsum_L2Octet(w, k) << 8) | NetCsum_L2Octet(w, k + 1u);
}

/* The class of an IP / ARP type value behind header `ether` (1: Ethernet II, 0: SNAP). */
NETCSUM_L2_FN uint32_t NetCsum_L2TypeClass(uint32_t type, int ether) {
    switch (type) {
    case NETCSUM_L2_TYPE_IPV4: return ether ? NETCSUM_L2_ETHER_IPV4 : NETCSUM_L2_SNAP_IPV4;
    case NETCSUM_L2_TYPE_IPV6: return ether ? NETCSUM_L2_ETHER_IPV6 : NETCSUM_L2_SNAP_IPV6;
    case NETCSUM_L2_TYPE_ARP:  return ether ? NETCSUM_L2_ETHER_ARP : NETCSUM_L2_SNAP_ARP;
    default:                   return ether ? NETCSUM_L2_INV_ETHER_TYPE : NETCSUM_L2_INV_SNAP_TYPE;
    }
}

/*
 * The class (NETCSUM_L2_*) of a frame of `len` octets received whose first 23 octets are w[].
 * have_hw: the interface's address is known (0: promiscuous, the destination check is skipped);
 * hw_lo = its octets 0-3 as a little-endian word, hw_hi = octets 4-5 (bits 0-15).
 */
NETCSUM_L2_FN uint32_t NetCsum_L2Class(uint32_t len, const uint32_t w[6], uint32_t eth_cfg, int have_hw, uint32_t hw_lo,
                                       uint32_t hw_hi) {
    uint32_t dst_lo, dst_hi, src_lo, src_hi, type_len;

    if (len < NETCSUM_L2_FRAME_MIN) return NETCSUM_L2_INV_FRAME_SIZE;
    dst_lo = w[0];                                       /* octets 0-3                                   */
    dst_hi = w[1] & 0xFFFFu;                             /* octets 4-5                                   */
    if (have_hw) {
        const int bcast = dst_lo == 0xFFFFFFFFu && dst_hi == 0xFFFFu;
        const int mcast = (dst_lo & 1u) != 0u && (eth_cfg & NETCSUM_ETHCFG_MCAST_RX) != 0u;
        if (!bcast && !mcast && (dst_lo != hw_lo || dst_hi != (hw_hi & 0xFFFFu))) return NETCSUM_L2_INV_ADDR_DEST;
    }
    src_lo = w[1] >> 16;                                 /* octets 6-7                                   */
    src_hi = w[2];                                       /* octets 8-11                                  */
    if ((src_lo == 0u && src_hi == 0u) || (src_lo == 0xFFFFu && src_hi == 0xFFFFFFFFu)) return NETCSUM_L2_INV_ADDR_SRC;
    type_len = NetCsum_L2Net16(w, 12u);
    if (type_len > NETCSUM_L2_IEEE_LEN_MAX) return NetCsum_L2TypeClass(type_len, 1);
    /* IEEE 802.3 + 802.2 LLC + SNAP */
    if (len >= NETCSUM_L2_FRAME_MIN_CRC && type_len != ((len - NETCSUM_L2_LEN_OVERHEAD) & 0xFFFFu)) {
        return NETCSUM_L2_INV_LEN_FRAME;
    }
    if (NetCsum_L2Octet(w, 14u) != 0xAAu) return NETCSUM_L2_INV_LLC_DSAP;
    if (NetCsum_L2Octet(w, 15u) != 0xAAu) return NETCSUM_L2_INV_LLC_SSAP;
    if (NetCsum_L2Octet(w, 16u) != 0x03u) return NETCSUM_L2_INV_LLC_CTRL;
    if ((w[4] >> 8) != 0u) return NETCSUM_L2_INV_SNAP_CODE;       /* octets 17-19                        */
    return NetCsum_L2TypeClass(NetCsum_L2Net16(w, 20u), 0);
}

/*
 * The class of a frame of `len` octets about to be transmitted (NetUtil_MI355X_TxBurstEther,
 * netcsum_mi355x.h (2b''''')), from the same six words: what NetIF_802x_Tx built (IF/net_if_802x.c:2643-2778).
 * A frame shorter than NETCSUM_L2_FRAME_MIN did not come from the 802.x layer, which pads every frame to
 * it (NetIF_802x_TxPktPrepareFrame, :2764-2778): INV_FRAME_SIZE from `len` alone. No address checks: the
 * destination is what ARP / NDP resolved, broadcast or a group, the source the interface's own address
 * written by the stack, so the INV_ADDR_* classes are never produced. The reference transmits Ethernet II
 * only (:2691-2761): the type at +12 names the class, and every other value — the 802.3 length form
 * (<= 1500) included, whose Rx length check assumes an FCS a Tx frame does not carry — is INV_ETHER_TYPE.
 */
NETCSUM_L2_FN uint32_t NetCsum_L2TxClass(uint32_t len, const uint32_t w[6]) {
    if (len < NETCSUM_L2_FRAME_MIN) return NETCSUM_L2_INV_FRAME_SIZE;
    return NetCsum_L2TypeClass(NetCsum_L2Net16(w, 12u), 1);
}

/* Octets of layer-2 header in front of a class's payload: 14 / 22, 0 for the INV_* classes. */
NETCSUM_L2_FN uint32_t NetCsum_L2HdrLen(uint32_t cls) {
    switch (cls) {
    case NETCSUM_L2_ETHER_IPV4:
    case NETCSUM_L2_ETHER_IPV6:
    case NETCSUM_L2_ETHER_ARP: return NETCSUM_L2_HDR_ETHER;
    case NETCSUM_L2_SNAP_IPV4:
    case NETCSUM_L2_SNAP_IPV6:
    case NETCSUM_L2_SNAP_ARP:  return NETCSUM_L2_HDR_SNAP;
    default:                   return 0u;
    }
}

/*
 * Octets of the frame the IP checksum pass is given, from frame start + NetCsum_L2HdrLen: len - header
 * length for a frame of an IP class whose datagram's version nibble is the one its type names, else 0
 * (ARP, the INV_* classes, and a type / version mismatch: the reference calls NetIPv4_Rx / NetIPv6_Rx
 * by frame type and they reject the version before any checksum).
 */
NETCSUM_L2_FN uint32_t NetCsum_L2IPOctets(uint32_t cls, uint32_t len, const uint32_t w[6]) {
    const uint32_t hdr = NetCsum_L2HdrLen(cls);
    uint32_t ver;

    if (cls > NETCSUM_L2_SNAP_IPV6) return 0u;           /* (the four IP classes come first)             */
    ver = (hdr == NETCSUM_L2_HDR_ETHER ? NetCsum_L2Octet(w, NETCSUM_L2_HDR_ETHER) : NetCsum_L2Octet(w, NETCSUM_L2_HDR_SNAP)) >> 4;
    if (cls == NETCSUM_L2_ETHER_IPV4 || cls == NETCSUM_L2_SNAP_IPV4) return ver == 6u ? 0u : len - hdr;
    return ver == 6u ? len - hdr : 0u;
}

/* The six words of a frame in memory (host side; len >= NETCSUM_L2_HDR_OCTETS octets readable). */
NETCSUM_L2_FN void NetCsum_L2Words(const uint8_t *frame, uint32_t w[6]) {
    uint32_t k;

    for (k = 0u; k < 6u; ++k) {
        const uint32_t b3 = (4u * k + 3u < NETCSUM_L2_HDR_OCTETS) ? frame[4u * k + 3u] : 0u;
        w[k] = (uint32_t)frame[4u * k] | ((uint32_t)frame[4u * k + 1u] << 8) | ((uint32_t)frame[4u * k + 2u] << 16) | (b3 << 24);
    }
}

#endif /* NETCSUM_ETHER_H */
