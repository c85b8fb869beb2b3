// netcsum_ether.hip — the 802.x demux pass of NetUtil_MI355X_RxBurstEther (include/netcsum_mi355x.h
// (2b'''')): a front pass over a burst of Ethernet frames that leaves the packet kernels untouched. One
// lane per frame: the lane classifies its frame by the rules of include/netcsum_ether.h (the reference's
// NetIF_802x_Rx / NetIF_802x_RxPktFrameDemux, in their order of checks) and writes the class and the
// offset/length descriptor of the IP datagram for the offset/length Rx burst that follows on the stream.
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
#include "netcsum_kernels.h"

namespace netcsum {

namespace {

typedef const __attribute__((address_space(1))) uint32_t gu32;

__global__ __launch_bounds__(kEtherDemuxBlock) void ether_demux_kernel(const EtherDemuxArgs A) {
    const uint32_t i = blockIdx.x * kEtherDemuxBlock + threadIdx.x;
    if (i >= A.n) return;
    const uint64_t o = A.off ? A.off[i] : (uint64_t)i * A.stride;
    const uint32_t len = A.len ? A.len[i] : A.len_u;
    uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (len >= NETCSUM_L2_FRAME_MIN) {
        const uintptr_t start = reinterpret_cast<uintptr_t>(A.base) + o;
        const uint32_t sh = (uint32_t)(start & 3u);
        gu32* q = reinterpret_cast<gu32*>(start - sh);
        uint32_t d[7];
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = q[k];
        d[6] = sh >= 2u ? q[6] : 0u;                     // octets 20-22 end in dword 6 only then
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
    }
    const uint32_t cls = NetCsum_L2Class(len, w, A.eth_cfg, (int)A.have_hw, A.hw_lo, A.hw_hi);
    const uint32_t ip = NetCsum_L2IPOctets(cls, len, w);
    A.l2_out[i] = (uint8_t)cls;
    A.off_out[i] = ip ? o + NetCsum_L2HdrLen(cls) : o;
    A.len_out[i] = (uint16_t)ip;
}

}  // namespace

hipError_t launch_ether_demux(const EtherDemuxArgs& a, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(ether_demux_kernel, dim3(ether_demux_blocks(a.n)), dim3(kEtherDemuxBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace netcsum
