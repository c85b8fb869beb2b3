// netcsum_packets.hip — gfx950 IPv4 / IPv6 packet-batch kernels, lane-group form.
//
// RX (fused validation, one HBM pass per packet): the IP header's and the transport checksum of every
//   received datagram are verified with the pseudo-header built in registers from the IP header,
//   instead of two passes (header verify, then transport verify) over HBM.
// TX (finalize, in place): the same sums with the checksum fields treated as zero, then the checksums
//   are written back.
// Which datagrams get which verdict, where the fields sit, which pseudo-header applies and the order
// of the checks are the rules of netcsum_ipparse.h (with the reference lines they follow), shared with
// the run-stream kernels (netcsum_pktstream.hip) and the extension-header walk (netcsum_v6walk.h);
// this file holds the lane-group window over a packet's first chunks and the sums.
//
// Work decomposition: the pipelined v2 structure of netcsum_kernels.hip (G >= 8 lanes per
// packet, K chunks per lane per pass, the next packet's loads in flight while the current one is
// reduced). Header fields are extracted from the loaded chunks with cross-lane shuffles and
// v_alignbyte_b32, so no load depends on packet contents. Two region sums (IP header, transport
// part) per packet; each region starts at an even packet offset, so the packet's address parity
// decides the rotation of both.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "netcsum_device.h"
#include "netcsum_ipparse.h"
#include "netcsum_kernels.h"
#include "netcsum_tables.h"

namespace netcsum {

namespace {

template <int K>
struct PktStage {
    u32x4     v[K];
    uint32_t  lead;      // packet start offset inside its first 16-B chunk
    uint32_t  avail;     // bytes of the packet present in the buffer
    uintptr_t a;         // packet start address
};

// Pins a stage's loaded chunks behind everything issued before this point (an empty asm with a
// memory clobber that reads and writes them): the consume of the stage cannot be hoisted into the
// next stage's issue, so the wave issues all K loads of the next stage before it waits for this one
// (the Tx instantiation otherwise stalled on `s_waitcnt vmcnt(8)` between its issue loads).
template <int K>
__device__ __forceinline__ void pin_chunks(u32x4 (&v)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        asm volatile("" : "+v"(v[k]) : : "memory");
    }
}

// The packet's frame starts at the 16-B boundary below it; chunk c of the frame is
// [q0 + 16c, q0 + 16c + 16).
template <int G, int K, bool NT>
__device__ __forceinline__ void pkt_issue(PktStage<K>& st, uintptr_t a, uint32_t avail, int lane) {
    st.a = a;
    st.lead = (uint32_t)(a & 15u);
    st.avail = avail;
    const uintptr_t q0 = a - st.lead;
    const uint32_t nch = (avail + st.lead + 15u) >> 4;
    const uintptr_t z = zero_addr();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t c = (uint32_t)(k * G + lane);
        gu32x4* src = reinterpret_cast<gu32x4*>((c < nch) ? (q0 + 16u * (uintptr_t)c) : z);
        st.v[k] = load16<NT>(src);
    }
}

__device__ __forceinline__ uint32_t pick4(u32x4 v, uint32_t comp) {
    uint32_t r = v.x;
    r = (comp == 1u) ? v.y : r;
    r = (comp == 2u) ? v.z : r;
    r = (comp == 3u) ? v.w : r;
    return r;
}

// Little-endian dword at packet offset i (lead + i + 7 < 16*G: the bytes sit in chunk slot 0 of
// the group's lanes). All lanes of the group get the same value.
__device__ __forceinline__ uint32_t pkt_dword(u32x4 v0, uint32_t lead, uint32_t i, int gbase) {
    const uint32_t r = lead + i;
    const uint32_t t = r >> 2;
    const uint32_t lo = (uint32_t)__shfl((int)pick4(v0, t & 3u), gbase + (int)(t >> 2), 64);
    const uint32_t hi = (uint32_t)__shfl((int)pick4(v0, (t + 1u) & 3u), gbase + (int)((t + 1u) >> 2), 64);
    const uint32_t b = r & 3u;
    return b ? __builtin_amdgcn_alignbyte(hi, lo, b) : lo;
}

// What frame byte f adds to this lane's unfolded v_sad_u16 accumulator, read from the lane's OWN
// k = 0 chunk (0 unless the lane holds the byte; weight 2^(8(f&1)) in the absolute LE frame). Tx
// checksum fields count as zero: their bytes are subtracted where they were summed, with no
// cross-lane traffic (the transport field's offset depends on the IP header length, so a shuffle
// would add a dependent LDS round trip per packet).
__device__ __forceinline__ uint32_t own_byte(u32x4 v0, uint32_t f, int lane) {
    const uint32_t b = (pick4(v0, (f >> 2) & 3u) >> (8u * (f & 3u))) & 0xFFu;
    return ((uint32_t)lane == (f >> 4)) ? (b << (8u * (f & 1u))) : 0u;
}

// The group's k = 0 chunks as the rules' accessor (netcsum_ipparse.h): the first 16 G - lead octets of
// the datagram. The dword reads are cross-lane shuffles, so every lane of the group takes every read.
template <int G>
struct GroupWindow {
    u32x4    v0;
    uint32_t lead;
    int      gbase;
    __device__ __forceinline__ uint32_t limit() const { return 16u * (uint32_t)G - lead; }
    template <int MinOff>
    __device__ __forceinline__ uint32_t dword(uint32_t off) const {
        return pkt_dword(v0, lead, off, gbase);
    }
};

struct PktInfo {
    ip::Class c;           // what the rules decide (netcsum_ipparse.h)
    uint32_t hlen;         // IPv4: IP header length. IPv6: bytes before the transport sum's start
                           // (8: the addresses open the sum; an ICMPv6 error is summed without them: its
                           // offset; SUMS: a fragment's payload offset). 0: malformed
    uint32_t l4_end;       // packet offset one past the transport part (0: malformed)
    uint32_t ext_end;      // IPv6: packet offset of the transport header (40 + extension headers)
};

// IPv6: no header checksum. The addresses are packet bytes [8, 40), contiguous with the transport
// part, so the transport sum runs over [8, end) — less the walked Routing headers [40, ext_end) — and
// only the length and next-header words of the pseudo-header are added in registers.
template <int G, bool TX, bool SUMS = false>
__device__ __forceinline__ PktInfo pkt_parse_v6(const GroupWindow<G>& w, uint32_t avail, uint32_t udp_mode, uint32_t d0,
                                                uint32_t d1) {                 // packet dwords 0 and 1
    PktInfo p;
    p.c = ip::classify6<TX, 0>(w, avail, udp_mode, d0, d1);
    const ip::Class& c = p.c;
    p.l4_end = ip::malformed(c) ? 0u : c.tot;
    p.ext_end = c.l4_off;
    p.hlen = ip::malformed(c)                     ? 0u
             : (SUMS && c.frag_len != 0u)         ? c.frag_off
             : (!TX && c.check_l4 && !c.pseudo)   ? c.l4_off
                                                  : 8u;
    return p;
}

template <int G, bool TX>
__device__ __forceinline__ PktInfo pkt_parse(const GroupWindow<G>& w, uint32_t avail, uint32_t udp_mode, uint32_t d0,
                                             uint32_t d1) {                    // packet dwords 0 and 1
    PktInfo p;
    const uint32_t d2 = w.template dword<0>(8u);
    const uint32_t d3 = w.template dword<0>(12u);
    const uint32_t d4 = w.template dword<0>(16u);
    p.c = ip::classify4<TX, 0>(w, avail, udp_mode, d0, d1, d2, d3, d4);
    p.hlen = p.c.l4_off;
    p.l4_end = ip::malformed(p.c) ? 0u : p.c.tot;
    p.ext_end = 40u;
    return p;
}

template <int G>
__device__ __forceinline__ void store_csum(uintptr_t a, uint32_t off, uint32_t host_val) {
    // global (not flat) stores: a flat store counts in lgkmcnt too and makes the waitcnt pass
    // drain vmcnt(0) in the next stage's issue. memcpy of the host-order value.
    __attribute__((address_space(1))) uint8_t* p = (__attribute__((address_space(1))) uint8_t*)(a + off);
    p[0] = (uint8_t)(host_val & 0xFFu);
    p[1] = (uint8_t)(host_val >> 8);
}

constexpr uint32_t kOOB = 0xFFFFFFFFu;     // buffer offset at/after every num_records: store dropped
constexpr int kRsrcWord3 = 0x00020000;     // gfx9-family raw buffer V# word 3

__device__ __forceinline__ __amdgpu_buffer_rsrc_t byte_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, kRsrcWord3);
}

__device__ __forceinline__ void store_byte(__amdgpu_buffer_rsrc_t r, uint32_t v, uint32_t off) {
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(v & 0xFFu), r, (int)off, 0, 0);
}

// A packet's stores, deferred: the kernel issues them right AFTER the next stage's loads, so no
// wait for a stage's loads can also wait for the previous packet's stores (the VMEM counter retires
// in issue order). Measured (profiles/r1tx11_tx_sweep.jsonl): no change for Tx — its extra time over
// Rx is the 2 M scattered header writes themselves (Tx with the stores compiled out: 0.250 ms).
struct PktStore {
    uintptr_t a;       // packet address
    uint32_t  vals;    // Tx: IP checksum | transport checksum << 16 (host order)
    uint32_t  meta;    // Tx: transport field offset, Rx: action | flags << 16 | store IP << 24 | store L4 << 25 |
                       // lane stores << 26
    uint32_t  idx;     // packet index (flags)
};

// BS (strided batches): every store is a raw buffer store executed by ALL lanes, the lanes that store
// nothing carrying an out-of-range offset, so every path issues the same VMEM stores and the
// compiler's vmcnt bookkeeping stays exact (stores under a lane-0 branch make it conservative).
// SUMS (Rx, RxBurstSums): ps.vals is the packet's NETCSUM_FRAG_SUM record, stored as one dword.
template <int G, bool TX, bool BS, bool SUMS = false>
__device__ __forceinline__ void pkt_store(const PktStore& ps, const PktBatchArgs& A) {
    const uint32_t f = (ps.meta >> 16) & 0xFFu;
    const bool me = (ps.meta >> 26) & 1u;
    if (me && ((f & NETCSUM_PKT_EXT_HDR) || (SUMS && ps.vals == kFragSumWalk)) && A.defer_word != nullptr) {
        *A.defer_word = A.defer_tag;                             // the walk pass has work (benign race)
    }
    const bool si = TX && ((ps.meta >> 24) & 1u), sl = TX && ((ps.meta >> 25) & 1u);
    const uint32_t l4off = ps.meta & 0xFFFFu;
    if constexpr (BS) {
        // Packets of one stage lie within a few strides of the wave's lane-0 packet (the lowest
        // address of the stage; if lane 0 stores nothing, no lane does), so a V# based there
        // reaches them with 32-bit offsets.
        const uintptr_t wb = (((uintptr_t)__builtin_amdgcn_readfirstlane((uint32_t)(ps.a >> 32))) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)ps.a);
        const uint32_t o = (uint32_t)(ps.a - wb);
        if constexpr (TX) {
            const __amdgpu_buffer_rsrc_t rp = byte_rsrc(reinterpret_cast<const void*>(wb), 0xFFFFFFFFu);
            store_byte(rp, ps.vals, si ? o + 10u : kOOB);        // memcpy of the host-order values
            store_byte(rp, ps.vals >> 8, si ? o + 11u : kOOB);
            store_byte(rp, ps.vals >> 16, sl ? o + l4off : kOOB);
            store_byte(rp, ps.vals >> 24, sl ? o + l4off + 1u : kOOB);
        }
        const __amdgpu_buffer_rsrc_t rf = byte_rsrc(A.flags_out, A.flags_out ? A.n : 0u);
        store_byte(rf, f, me ? ps.idx : kOOB);
        if constexpr (TX) {                                      // host-memory forms: what was written
            const uint64_t qb = A.fieldpos_out ? (uint64_t)A.n * 4u : 0u;
            const __amdgpu_buffer_rsrc_t rq = byte_rsrc(A.fieldpos_out, (uint32_t)(qb < 0xFFFFFFFFull ? qb : 0xFFFFFFFFull));
            __builtin_amdgcn_raw_buffer_store_b32((si ? kFieldIP : 0u) | (sl ? kFieldL4 | l4off : 0u), rq,
                                                  (int)(me ? ps.idx * 4u : kOOB), 0, 0);
        }
        if constexpr (!TX) {
            const __amdgpu_buffer_rsrc_t ra = byte_rsrc(A.action_out, A.action_out ? A.n : 0u);
            store_byte(ra, l4off, me ? ps.idx : kOOB);
        }
        if constexpr (SUMS) {                                    // (n < 2^30, RxBurstSums checks: 4 n fits the V#)
            const __amdgpu_buffer_rsrc_t rs = byte_rsrc(A.sums_out, A.n < (1u << 30) ? A.n * 4u : 0u);
            __builtin_amdgcn_raw_buffer_store_b32(ps.vals, rs, (int)(me && ps.idx < (1u << 30) ? ps.idx * 4u : kOOB), 0, 0);
        }
    } else {
        if (!me) {
            return;
        }
        if (si) {
            store_csum<G>(ps.a, 10u, ps.vals & 0xFFFFu);
        }
        if (sl) {
            store_csum<G>(ps.a, l4off, ps.vals >> 16);
        }
        if (A.flags_out) {
            A.flags_out[ps.idx] = (uint8_t)f;
        }
        if (!TX && A.action_out) {
            A.action_out[ps.idx] = (uint8_t)l4off;
        }
        if (TX && A.fieldpos_out) {
            A.fieldpos_out[ps.idx] = (si ? kFieldIP : 0u) | (sl ? kFieldL4 | l4off : 0u);
        }
        if constexpr (SUMS) {
            A.sums_out[ps.idx] = ps.vals;
        }
    }
}

template <int G, int K, bool NT, bool TX, int VER, bool SUMS = false>
__device__ __forceinline__ PktStore pkt_consume(const PktStage<K>& st, const PktBatchArgs& A, uint32_t idx, bool valid,
                                                int lane, int gbase) {
    // One sum over [lead, lead + end) (end = transport end, or the IP header end when the transport
    // part is not checked), plus the IP header alone from the k = 0 chunks (lead + hlen < 16*G).
    // Both are exact integer sums of the same frame half-words, so the transport part is their
    // difference — exact, hence still zero iff all its bytes are zero (the reference's all-zero ->
    // 0 / 0xFFFF distinction). TX checksum fields count as zero: their bytes are subtracted from
    // the owning lane's sums.
    //
    // The chunks are summed UNMASKED (chunks past `end` dropped by a select on their sum); the bytes
    // of the frame before the packet and those past `end` in the last chunk are subtracted once per
    // lane afterwards (low_bytes), instead of masking every chunk: the packet kernels are VALU-issue
    // bound (profiles/r1txp_pmc.json), and per-chunk edge masks executed on every k slot dominated.
    const uint32_t lead = st.lead;
    // VER 4 / 6: one IP version per batch; VER 0: per packet by the version nibble (a mixed NIC ring)
    // (the first two dwords, read once, outside the per-version branch)
    const uint32_t d0 = pkt_dword(st.v[0], lead, 0u, gbase);
    const uint32_t d1 = pkt_dword(st.v[0], lead, 4u, gbase);
    const bool is6 = (VER == 6) || (VER == 0 && ((d0 >> 4) & 0xFu) == 6u);
    const GroupWindow<G> win{st.v[0], lead, gbase};
    const PktInfo p = is6 ? pkt_parse_v6<G, TX, SUMS>(win, st.avail, A.udp_tx_csum, d0, d1)
                         : pkt_parse<G, TX>(win, st.avail, A.udp_tx_csum, d0, d1);
    const ip::Class& pc = p.c;
    // SUMS: a fragment's payload [hlen, l4_end) is summed as a transport part is
    const uint32_t frag_len = SUMS ? pc.frag_len : 0u;
    const uint32_t end = (pc.check_l4 || frag_len != 0u) ? p.l4_end : p.hlen;
    const uint32_t rend = lead + end;
    const uint32_t nch = (rend + 15u) >> 4;
    const uint32_t cl = nch - 1u;                                // chunk holding byte rend - 1 (~0u: none)
    uint32_t acc = 0u;
    u32x4 vl = u32x4{0u, 0u, 0u, 0u};                            // that chunk, on the lane holding it
#pragma unroll
    for (int k = 0; k < K; ++k) {
        // Every loaded register is consumed on every path (no branch: a load left unconsumed on some
        // path stays "pending" across the loop back-edge and the compiler drains vmcnt(0) there).
        const uint32_t c = (uint32_t)(k * G + lane);
        const u32x4 v = st.v[k];
        const uint32_t sv = sum4(v, 0u);
        acc += (c < nch) ? sv : 0u;
        vl.x = (c == cl) ? v.x : vl.x;
        vl.y = (c == cl) ? v.y : vl.y;
        vl.z = (c == cl) ? v.z : vl.z;
        vl.w = (c == cl) ? v.w : vl.w;
    }
    const int l16 = 16 * lane;
    const uint32_t pre = low_bytes(st.v[0], (int)lead - l16);   // frame bytes before the packet
    acc -= pre + (sum4(vl, 0u) - low_bytes(vl, (int)(rend - 16u * cl)));
    const uint32_t ip_raw = low_bytes(st.v[0], (int)(lead + p.hlen) - l16) - pre;
    if (nch > (uint32_t)(G * K)) {                               // packets longer than one pass
        const uintptr_t q0 = st.a - lead;
        for (uint32_t c0 = (uint32_t)(G * K); c0 < nch; c0 += (uint32_t)(G * K)) {
            u32x4 w[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t c = c0 + (uint32_t)(k * G + lane);
                w[k] = load16<NT>(reinterpret_cast<gu32x4*>((c < nch) ? (q0 + 16u * (uintptr_t)c) : zero_addr()));
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t c = c0 + (uint32_t)(k * G + lane);
                u32x4 v = w[k];                                  // zero chunk past the range
                if (c < nch) {
                    v = edge_mask_rel(v, c, lead, rend);
                }
                acc = sum4(v, acc);
            }
        }
    }
    uint32_t acc_ip = ip_raw, acc_l4 = acc - ip_raw;
    if (is6 && p.ext_end > 40u && p.hlen == 8u) {                 // addresses + transport, not the ext headers
        acc_l4 -= low_bytes(st.v[0], (int)(lead + p.ext_end) - l16) - low_bytes(st.v[0], (int)(lead + 40u) - l16);
    }
    if (TX) {
        if (!is6 && !ip::malformed(pc)) {
            acc_ip -= own_byte(st.v[0], lead + 10u, lane) + own_byte(st.v[0], lead + 11u, lane);
        }
        if (pc.check_l4) {
            const uint32_t f = lead + pc.l4_csum_off;
            acc_l4 -= own_byte(st.v[0], f, lane) + own_byte(st.v[0], f + 1u, lane);
        }
    }
    uint32_t sip = fold16(acc_ip), sl4 = fold16(acc_l4);
    if (lead & 1u) {                                              // both regions start at even offsets
        sip = rot8(sip);
        sl4 = rot8(sl4);
    }
    sip = fold16(group_sum<G>(sip));
    sl4 = fold16(group_sum<G>(sl4) + pc.pseudo_le);
    const ip::Verdict vd = ip::verdict<TX>(pc, sip, sl4);
    const uint32_t f = vd.flags, cip = vd.cip, cl4 = vd.cl4;     // Tx values to store; ~0u = none
    PktStore ps;
    ps.a = st.a;
    ps.vals = (cip & 0xFFFFu) | ((cl4 & 0xFFFFu) << 16);
    if constexpr (SUMS) {                                        // sl4: the payload's folded sum (no pseudo-header)
        ps.vals = frag_len != 0u ? (sl4 & 0xFFFFu) | (frag_len << 16) : (pc.frag_walk ? kFragSumWalk : 0u);
    }
    const uint32_t low = TX ? (pc.l4_csum_off & 0xFFFFu) : rx_action(f, pc.proto, is6, A.rx_cfg);
    ps.meta = low | ((f & 0xFFu) << 16) | (cip != ~0u ? 1u << 24 : 0u) |
              (cl4 != ~0u ? 1u << 25 : 0u) | ((valid && lane == 0) ? 1u << 26 : 0u);
    ps.idx = idx;
    return ps;
}

template <bool VARLEN>
__device__ __forceinline__ void pkt_desc(const PktBatchArgs& A, uint32_t i, uint64_t& off, uint32_t& avail) {
    if constexpr (VARLEN) {
        const uint32_t ic = (i < A.n) ? i : 0u;
        off = A.off[ic];
        avail = A.len[ic];
    } else {
        off = (uint64_t)i * A.stride;
        avail = A.len_u;
    }
}

// 4 waves per SIMD: the Tx instantiations otherwise take 131 VGPRs (3 waves), 25 % less memory
// parallelism than Rx (122 VGPRs); capped at 128 they do not spill (profiles/r1txp_pmc.json).
template <int G, int K, bool VARLEN, bool NT, bool TX, int VER, bool SUMS = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) pkt_batch_kernel(PktBatchArgs A) {
    static_assert(G >= 8, "header extraction needs the first 6 chunks in slot 0");
    const int lane = (int)(threadIdx.x & (G - 1));
    const int gbase = (int)(threadIdx.x & 63) & ~(G - 1);
    const uint32_t gpb = blockDim.x / G;
    const uint32_t grp = threadIdx.x / G;
    uint32_t first, step, end;
    if (A.tile) {
        const uint64_t t0 = (uint64_t)blockIdx.x * gpb * A.tile;
        first = (uint32_t)t0 + grp;
        step = gpb;
        end = (uint32_t)min<uint64_t>(t0 + (uint64_t)gpb * A.tile, A.n);
    } else {
        first = blockIdx.x * gpb + grp;
        step = gridDim.x * gpb;
        end = A.n;
    }
    const uint32_t cnt = group_iters(first, step, end);
    const uint32_t iters = __builtin_amdgcn_readfirstlane(cnt);   // wave-uniform trip count
    if (iters == 0u) {
        return;
    }
    const uintptr_t base = (uintptr_t)A.base;
    const uintptr_t z = zero_addr();
    PktStage<K> S0, S1;
    uint64_t off;
    uint32_t avail;
    uint32_t i = first;
    bool v0 = cnt != 0u, v1 = false;
    pkt_desc<VARLEN>(A, i, off, avail);
    pkt_issue<G, K, NT>(S0, v0 ? base + off : z, v0 ? avail : 0u, lane);
    PktStore pend{z, 0u, 0u, 0u};                                // nothing to store yet
    for (uint32_t j = 0u; j < iters; j += 2u) {                  // one scalar exit (see seg_pipe_kernel)
        uint32_t nx = i + step;
        v1 = j + 1u < cnt;
        pkt_desc<VARLEN>(A, nx, off, avail);
        pkt_issue<G, K, NT>(S1, v1 ? base + off : z, v1 ? avail : 0u, lane);
        pkt_store<G, TX, !VARLEN, SUMS>(pend, A);                // previous packet's stores, after the loads
        pin_chunks<K>(S0.v);
        pend = pkt_consume<G, K, NT, TX, VER, SUMS>(S0, A, i, v0, lane, gbase);
        i = nx;
        nx = i + step;
        v0 = j + 2u < cnt;
        pkt_desc<VARLEN>(A, nx, off, avail);
        pkt_issue<G, K, NT>(S0, v0 ? base + off : z, v0 ? avail : 0u, lane);
        pkt_store<G, TX, !VARLEN, SUMS>(pend, A);
        pin_chunks<K>(S1.v);
        pend = pkt_consume<G, K, NT, TX, VER, SUMS>(S1, A, i, v1, lane, gbase);
        i = nx;
    }
    pkt_store<G, TX, !VARLEN, SUMS>(pend, A);
}

template <int G, int K, bool VARLEN, bool TX, int VER>
hipError_t launch_pkt_gk(const PktBatchArgs& a, const LaunchCfg& c, hipStream_t s) {
    const uint32_t gpb = 256u / G;
    int grid;
    if (a.tile) {
        const uint64_t per = (uint64_t)gpb * a.tile;
        grid = (int)(((uint64_t)a.n + per - 1u) / per);
    } else {
        grid = c.grid > 0 ? c.grid : (int)(((uint64_t)a.n + gpb - 1u) / gpb);
    }
    // fragment payload sums (RxBurstSums): Rx of mixed batches only; one IP version has no such instantiation
    constexpr bool kSums = !TX && VER == 0;
    if (!TX && !kSums && a.sums_out != nullptr) return hipErrorInvalidValue;
    using Sums = std::conditional_t<kSums, dsp::Flag, dsp::Of<false>>;
    return dsp::pick(hipErrorInvalidValue, [&](auto nt, auto sums) {
        hipLaunchKernelGGL((pkt_batch_kernel<G, K, VARLEN, nt, TX, VER, sums>), dim3(grid), dim3(256), 0, s, a);
        return hipGetLastError();
    }, dsp::Flag{c.nt}, Sums{kSums && a.sums_out != nullptr});
}

}  // namespace

// ip_ver 4 or 6, else the mixed form; group 8, 16 or 32, else 64; K 4 or 8 chunks per lane at group
// 8, 3 or 6 at 16 and 32, 4 at 64.
hipError_t launch_pkt_batch(const PktBatchArgs& a, const LaunchCfg& c, bool tx, int ip_ver, hipStream_t s) {
    const int gl = c.group_lanes;
    const int g = (gl == 8 || gl == 16 || gl == 32) ? gl : 64;
    const int k = g == 64 ? 4 : g == 8 ? (c.chunks_per_pass <= 4 ? 4 : 8) : (c.chunks_per_pass <= 3 ? 3 : 6);
    return dsp::pick_tuple(PktGroupTable{}, hipErrorInvalidValue, [&](auto gc, auto kc) {
        return dsp::pick(hipErrorInvalidValue, [&](auto varlen, auto txc, auto ver) {
            return launch_pkt_gk<gc, kc, varlen, txc, ver>(a, c, s);
        }, dsp::Flag{a.off != nullptr}, dsp::Flag{tx}, dsp::Or<0, 4, 6>{ip_ver});
    }, g, k);
}

}  // namespace netcsum
