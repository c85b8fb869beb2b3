// netcsum_ether.hip — the 802.x demux pass of NetUtil_MI355X_RxBurstEther (include/netcsum_mi355x.h
// (2b'''')): a front pass over a burst of Ethernet frames that leaves the packet kernels untouched. One
// lane per frame: the lane classifies its frame by the rules of include/netcsum_ether.h (the reference's
// NetIF_802x_Rx / NetIF_802x_RxPktFrameDemux, in their order of checks) and writes the class and the
// offset/length descriptor of the IP datagram for the offset/length Rx burst that follows on the stream.
//
// (The resident burst server does the same step inside the waves that stream the datagrams, without this
// pass: netcsum_pktstream.hip pkt_ether_run. The head load is stated once for both, netcsum_etherhead.h.)
//
// Reads: the rules need a frame's first 23 octets. A frame may start at any address, so the lane loads
// the aligned dwords that cover [start, start + 23) — six, or seven when the start is 2 or 3 past a
// dword — and shifts them into place (v_alignbyte_b32); no byte loads (the compiler fetches the same
// dwords with wider 4-B-aligned loads: x4, x2 and the conditional seventh). A frame shorter than 60 octets
// is classified from its length and not read at all; every other frame holds at least 60 octets, so the
// dwords loaded are among those that cover [start, start + len). Cost: one 64-B sector per frame, two
// when the 23 octets straddle a sector boundary (a start at 42 .. 63 past one); neighbouring lanes' frames
// are a slot apart, so nothing coalesces on the read side and the pass is bound by sectors, not bytes.
// Writes: lane-consecutive, 1 + 8 + 2 B per frame.
#include <hip/hip_runtime.h>

#include "../../include/netcsum_ether.h"
#include "netcsum_etherhead.h"
#include "netcsum_kernels.h"

namespace netcsum {

namespace {

__global__ __launch_bounds__(kEtherDemuxBlock) void ether_demux_kernel(const EtherDemuxArgs A) {
    const uint32_t i = blockIdx.x * kEtherDemuxBlock + threadIdx.x;
    if (i >= A.n) return;
    const uint64_t o = A.off ? A.off[i] : (uint64_t)i * A.stride;
    const uint32_t len = A.len ? A.len[i] : A.len_u;
    const EtherHead h = ether_head(reinterpret_cast<uintptr_t>(A.base) + o, len, A.eth_cfg, A.have_hw, A.hw_lo, A.hw_hi);
    A.l2_out[i] = (uint8_t)h.cls;
    A.off_out[i] = h.ip ? o + NetCsum_L2HdrLen(h.cls) : o;
    A.len_out[i] = (uint16_t)h.ip;
}

// The Tx demux of NetUtil_MI355X_TxBurstEther ((2b''''')): the same lane per frame and head load with the
// Tx rule (NetCsum_L2TxClass: the frame's length, then the Ethernet II type; octets 12 - 14 decide
// everything, the same one or two sectors per frame), and the descriptor of the datagram TxBurst is to
// finalize: {start + 14, len - 14}, or {start, 0} for a frame that carries none. It writes nothing to
// the ring.
__global__ __launch_bounds__(kEtherDemuxBlock) void ether_tx_demux_kernel(const EtherDemuxArgs A) {
    const uint32_t i = blockIdx.x * kEtherDemuxBlock + threadIdx.x;
    if (i >= A.n) return;
    const uint64_t o = A.off ? A.off[i] : (uint64_t)i * A.stride;
    const uint32_t len = A.len ? A.len[i] : A.len_u;
    const EtherHead h = ether_head_tx(reinterpret_cast<uintptr_t>(A.base) + o, len);
    A.l2_out[i] = (uint8_t)h.cls;
    A.off_out[i] = h.ip ? o + NETCSUM_L2_HDR_ETHER : o;
    A.len_out[i] = (uint16_t)h.ip;
}

}  // namespace

hipError_t launch_ether_tx_demux(const EtherDemuxArgs& a, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(ether_tx_demux_kernel, dim3(ether_demux_blocks(a.n)), dim3(kEtherDemuxBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ether_demux(const EtherDemuxArgs& a, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(ether_demux_kernel, dim3(ether_demux_blocks(a.n)), dim3(kEtherDemuxBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace netcsum
