// netcsum_etherhead.h — the head load and classify step of the 802.x demux, stated once for the lanes
// that do it: the demux kernels (netcsum_ether.hip ether_demux_kernel / ether_tx_demux_kernel, one lane per
// frame of a launch) and the resident burst server's Ether forms, Rx and Tx (netcsum_pktstream.hip, lane k
// of the wave that owns a run).
// The rules themselves are include/netcsum_ether.h's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/netcsum_ether.h"

namespace netcsum {

// What a lane knows of its frame after the step: the class and the octets of IP datagram behind the
// layer-2 header (0: none to check — ARP, the INV_* classes, a type / version mismatch).
struct EtherHead {
    uint32_t cls;          // NETCSUM_L2_*
    uint32_t ip;           // NetCsum_L2IPOctets
};

// The six head words (include/netcsum_ether.h) of the frame of `len` octets at address `start`, received
// or about to be transmitted. Which octets are read: the aligned dwords
// that cover [start, start + 23) — six, or seven when the start is 2 or 3 past a dword — shifted into
// place (v_alignbyte_b32); a frame shorter than 60 octets is classified from its length and not read
// at all, and every other frame holds at least 60 octets, so the dwords loaded are among those that
// cover [start, start + len).
__device__ __forceinline__ void ether_head_words(uintptr_t start, uint32_t len, uint32_t w[6]) {
    typedef const __attribute__((address_space(1))) uint32_t gu32;
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = 0u;
    if (len >= NETCSUM_L2_FRAME_MIN) {
        const uint32_t sh = (uint32_t)(start & 3u);
        gu32* q = reinterpret_cast<gu32*>(start - sh);
        uint32_t d[7];
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = q[k];
        d[6] = sh >= 2u ? q[6] : 0u;                     // octets 20-22 end in dword 6 only then
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
    }
}

__device__ __forceinline__ EtherHead ether_head(uintptr_t start, uint32_t len, uint32_t eth_cfg, uint32_t have_hw,
                                                uint32_t hw_lo, uint32_t hw_hi) {
    uint32_t w[6];
    ether_head_words(start, len, w);
    EtherHead h;
    h.cls = NetCsum_L2Class(len, w, eth_cfg, (int)have_hw, hw_lo, hw_hi);
    h.ip = NetCsum_L2IPOctets(h.cls, len, w);
    return h;
}

// The frame of `len` octets about to be transmitted at `start`: the same head load, the Tx rule
// (NetCsum_L2TxClass: no address checks, Ethernet II only).
__device__ __forceinline__ EtherHead ether_head_tx(uintptr_t start, uint32_t len) {
    uint32_t w[6];
    ether_head_words(start, len, w);
    EtherHead h;
    h.cls = NetCsum_L2TxClass(len, w);
    h.ip = NetCsum_L2IPOctets(h.cls, len, w);
    return h;
}

}  // namespace netcsum
