// The kernel families' legal template-argument sets that are not full products, and the depth
// lists: each stated once, read by the launcher, the occupancy query and the support predicate
// (plain C++17, no HIP: tests/c_dispatch checks them on the CPU).
#pragma once

#include <algorithm>

#include "netcsum_dispatch.h"

namespace netcsum {

template <auto... Vs>
using Tu = dsp::Tup<Vs...>;

// seg_tile_kernel: (G lanes per segment, P KiB image pieces, K chunks per lane).
using TileTable = dsp::Table<Tu<1, 2, 3>, Tu<1, 4, 6>, Tu<4, 1, 1>, Tu<4, 2, 2>, Tu<8, 2, 2>, Tu<8, 4, 4>, Tu<16, 4, 4>,
                             Tu<16, 6, 6>, Tu<16, 8, 8>, Tu<32, 2, 2>, Tu<32, 4, 3>, Tu<32, 4, 4>, Tu<32, 8, 8>, Tu<64, 2, 2>,
                             Tu<64, 4, 4>, Tu<64, 8, 8>>;

// seg_hdr_kernel: (P pieces per tile, S stages, H headers per lane). H 1: P <= 5; H 4: S <= 3.
using HdrTable = dsp::Table<
    Tu<1, 2, 1>, Tu<1, 3, 1>, Tu<1, 4, 1>, Tu<2, 2, 1>, Tu<2, 3, 1>, Tu<2, 4, 1>, Tu<3, 2, 1>, Tu<3, 3, 1>, Tu<3, 4, 1>,
    Tu<4, 2, 1>, Tu<4, 3, 1>, Tu<4, 4, 1>, Tu<5, 2, 1>, Tu<5, 3, 1>, Tu<5, 4, 1>,
    Tu<1, 2, 2>, Tu<1, 3, 2>, Tu<1, 4, 2>, Tu<2, 2, 2>, Tu<2, 3, 2>, Tu<2, 4, 2>, Tu<3, 2, 2>, Tu<3, 3, 2>, Tu<3, 4, 2>,
    Tu<4, 2, 2>, Tu<4, 3, 2>, Tu<4, 4, 2>, Tu<5, 2, 2>, Tu<5, 3, 2>, Tu<5, 4, 2>, Tu<6, 2, 2>, Tu<6, 3, 2>, Tu<6, 4, 2>,
    Tu<1, 2, 4>, Tu<1, 3, 4>, Tu<2, 2, 4>, Tu<2, 3, 4>, Tu<3, 2, 4>, Tu<3, 3, 4>, Tu<4, 2, 4>, Tu<4, 3, 4>,
    Tu<5, 2, 4>, Tu<5, 3, 4>, Tu<6, 2, 4>, Tu<6, 3, 4>>;

// The header tile's stages for the requested count and h headers per lane: 2..4 (H = 4: 2..3).
inline int hdr_stages(int stages, int h) {
    return std::min(stages == 3 ? 3 : (stages == 4 ? 4 : 2), h == 4 ? 3 : 4);
}

// pkt_stream_kernel: (D pieces in flight, BND bound, VL offset/length), the same for every IP
// version and for the SUMS forms: every bound with 4 pieces in flight, 8 with bounds 0, 2 and 3;
// offset/length runs in the live-piece forms 1 and 2.
using PktStreamTable = dsp::Table<Tu<4, 0, false>, Tu<4, 1, false>, Tu<4, 2, false>, Tu<4, 3, false>, Tu<8, 0, false>,
                                  Tu<8, 2, false>, Tu<8, 3, false>, Tu<4, 1, true>, Tu<4, 2, true>, Tu<8, 2, true>>;

// pkt_batch_kernel: (G lanes per packet, K chunks per lane).
using PktGroupTable = dsp::Table<Tu<8, 4>, Tu<8, 8>, Tu<16, 3>, Tu<16, 6>, Tu<32, 3>, Tu<32, 6>, Tu<64, 4>>;

// Pieces in flight.
using StreamDepth = dsp::Of<4, 6, 8>;          // seg_stream_kernel
using VarlenDepth = dsp::Or<4, 8>;             // seg_stream_varlen_kernel: 8, and 4 for every other request
using LiveDepth = dsp::Of<4, 8>;               // seg_live_varlen_kernel, seg_hdrstream_kernel

}  // namespace netcsum
