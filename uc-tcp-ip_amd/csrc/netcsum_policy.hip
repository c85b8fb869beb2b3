// netcsum_policy.hip — launch policy of the batch ABI: which kernel form, geometry and run length a
// segment batch, a packet batch and a host burst get, from the batch's shape and the calling thread's
// Tune alone. Decisions only: nothing here launches, allocates or waits, and nothing stores to a tuning
// knob; the only runtime calls are the cached compute-unit count and the occupancy queries under
// GRID_MULT > 1. The entry points (netcsum_abi.hip) act on what these functions return, and every
// decision is observable in NetUtil_MI355X_LastLaunch() (tools/launch_matrix.py records them).
#include <algorithm>
#include <cstdio>

#include "netcsum_device.h"
#include "netcsum_host.h"

namespace nchost {
namespace {

int pow2_group(uint32_t want) {                     // smallest supported group >= want
    static const int gs[] = {1, 4, 8, 16, 32, 64};
    for (int g : gs) {
        if ((uint32_t)g >= want) return g;
    }
    return 64;
}

int chunk_slots(uint32_t want) {                    // smallest supported K >= want
    static const int ks[] = {1, 2, 3, 4, 6, 8};
    for (int k : ks) {
        if ((uint32_t)k >= want) return k;
    }
    return 8;
}

uint32_t gcd_u32(uint32_t a, uint32_t b) {
    while (b) {
        const uint32_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// v4 (wave-tile LDS image) geometry for a strided batch, if one compiled instantiation fits:
// G lanes per segment (S = 64/G segments per wave-tile), P KiB image per stage, K chunks per lane.
bool choose_tile(const netcsum::SegBatchArgs& a, int g_force, int k_force, int* g_out, int* p_out, int* k_out) {
    if (a.seg_off != nullptr || a.seg_stride < a.seg_len || a.seg_stride > 0xFFFFFFFFull) return false;
    const uint32_t stride = (uint32_t)a.seg_stride;
    const uint32_t g16 = stride ? gcd_u32(stride, 16u) : 16u;
    const uint32_t maxlead = (uint32_t)((uintptr_t)a.base % g16) + (16u - g16);   // worst first-chunk offset
    const uint32_t nchmax = (maxlead + a.seg_len + 15u) >> 4;
    static const int gs[] = {1, 4, 8, 16, 32, 64};
    static const int ps[] = {1, 2, 4, 6, 8};
    static const int ks[] = {1, 2, 3, 4, 6, 8};
    for (int g : gs) {
        if (g_force && g != g_force) continue;
        const uint32_t S = 64u / (uint32_t)g;
        const uint64_t img = (uint64_t)(S - 1u) * stride + a.seg_len + 127u;
        const uint64_t pimg = a.pseudo ? (uint64_t)(S - 1u) * a.pseudo_stride + a.pseudo_len + 15u : 0u;
        if (pimg > 1024u) continue;
        const uint32_t kneed = (nchmax + (uint32_t)g - 1u) / (uint32_t)g;
        if (!g_force && kneed > 8u) continue;            // prefer the narrowest group that fits
        for (int p : ps) {
            if ((uint64_t)p * 1024u < img) continue;
            for (int k : ks) {
                if (k_force && k != k_force) continue;
                if ((uint32_t)k < kneed) continue;
                if (netcsum::tile_supported(g, p, k)) {
                    *g_out = g;
                    *p_out = p;
                    *k_out = k;
                    return true;
                }
            }
        }
    }
    return false;
}

}  // namespace

// Geometry policy (round-1 measurements on MI355X, profiles/r1_sweep_*.jsonl):
//  * kernel 2 (pipelined register loads) is the fastest form for C2, C3 and C4;
//  * G = narrowest lane group whose 8 chunk slots per lane cover a segment (1500 B -> G 16, K 6;
//    20-B headers -> G 1, K 2), from the exact worst-case chunk count of the batch's alignment;
//  * contiguous block tiles of 4 segments per group (grid = n / (groups per block * 4));
//  * non-temporal loads when G >= 8 (lane groups share no 16-B chunks); plain loads for narrow
//    groups, whose neighbouring lanes re-read shared chunks through L1/L2.
netcsum::LaunchCfg choose_cfg(const Tune& t, int dev, const netcsum::SegBatchArgs& a, uint32_t len_hint) {
    const bool varlen = a.seg_off != nullptr;
    netcsum::LaunchCfg c{};
    c.block = t.block;
    if (c.block < 64 || c.block > 1024 || (c.block & 63)) c.block = 256;
    c.kernel = t.kernel;
    c.cus = cu_count(dev);
    c.grid_mult = t.grid_mult;
    c.grid = t.grid;                       // > 0: fixed grid (grid-stride mode)
    const int tile = t.tile;
    c.tile = tile >= 0 ? tile : (c.grid > 0 ? 0 : 4);
    const int nt = t.nt;

    if (c.kernel == 0) {
        c.kernel = netcsum::hdrstream_supported(a) ? 8
                 : netcsum::hdr_supported(a) ? 7
                 : netcsum::small_supported(a) ? 5
                 : (netcsum::stream_dense(a) || (varlen && netcsum::stream_supported(a))) ? 6 : 2;
    }
    if (c.kernel == 8) {
        if (netcsum::hdrstream_supported(a)) {
            // Run-stream header form (the default for packed 16 / 20-B headers, C3): TILE > 0 =
            // headers per wave run, CHUNKS 4 / 8 = pieces in flight (auto 4), non-temporal loads
            // unless NT_LOADS 0. Auto run: the most headers (multiple of 16) whose bytes fit the 4
            // pieces in flight from any 128-B lead, so a wave reads its run in ONE round: 192 x 20 B
            // with the row touch = 0.0583 ms against 0.0627 for kernel 7 (r2c3u / r2c3p sweeps).
            int d = t.chunks;
            c.chunks_per_pass = (d == 8) ? 8 : 4;
            c.stream_spw = tile > 0 ? (uint32_t)tile : ((4096u - 128u) / a.seg_len) & ~15u;
            c.nt = nt != 0;
            c.group_lanes = 64;
            c.blocks_needed = 0;
            return c;
        }
        c.kernel = 7;                                  // outside its domain: the LDS-tile header form
    }
    if (c.kernel == 7) {
        if (netcsum::hdr_supported(a)) {
            // Defaults from the r2 sweeps (C3, 16 M x 20 B, tools/c3_sweep.py): 4 headers per lane
            // (256-header tiles = 5 whole KiB now that the piece count is exact), 2 tiles in flight,
            // 2 tiles per wave (grid = tiles / 8): 0.0615 ms = 6.0 TB/s vs 0.063 for round 1's 2
            // headers x 3 tiles x 4 tiles per wave; GRID_MULT > 1 instead sizes the grid as resident
            // blocks x CUs x mult.
            const bool auto_h = !(tile == 1 || tile == 2 || tile == 4);
            c.tile = netcsum::hdr_lanes_h(a, auto_h ? 4 : tile);   // TILE = headers per lane (1, 2, 4)
            int st = t.chunks;
            if (!(st == 2 || st == 3 || st == 4)) st = (c.tile == 2) ? 3 : 2;
            c.chunks_per_pass = st;
            c.group_lanes = 1;
            c.nt = true;
            c.blocks_needed = 0;
            if (c.grid <= 0) {
                const uint64_t tiles = ((uint64_t)a.n_seg + 64u * c.tile - 1u) / (64u * c.tile);
                const uint64_t per_wave = (auto_h && c.tile == 4) ? 2u : 4u;
                c.grid = c.grid_mult > 1 ? netcsum::hdr_occupancy(a, st, c.tile) * c.cus * c.grid_mult
                                         : (int)std::max<uint64_t>(1u, (tiles + 4u * per_wave - 1u) / (4u * per_wave));
            }
            return c;
        }
        c.kernel = 5;                                  // outside its domain: the register form
    }
    if (c.kernel == 6) {
        if (netcsum::stream_supported(a)) {
            int d = t.chunks;
            if (!(d == 4 || d == 6 || d == 8)) d = 4;
            c.chunks_per_pass = d;
            c.nt = nt != 0;                                // default non-temporal: the run is read once
            // Run length (segments per wave): TILE > 0 sets it; GRID_BLOCKS > 0 forces 4 x grid runs;
            // GRID_MULT > 1 sizes runs for that many rounds of resident waves; default 16 segments
            // (r1w5 sweep, C2: runs of 16 read 6.8 TB/s, single-round runs of 128 6.6 TB/s — short
            // runs keep the waves in flight on nearby bytes).
            uint64_t waves;
            if (tile > 0) {
                waves = ((uint64_t)a.n_seg + (uint64_t)tile - 1u) / (uint64_t)tile;
            } else if (c.grid > 0) {
                waves = 4ull * (uint64_t)c.grid;
            } else if (c.grid_mult > 1) {
                waves = (uint64_t)netcsum::stream_occupancy(d, a, c.nt) * 4u * (uint64_t)c.cus * (uint64_t)c.grid_mult;
            } else {
                // runs of 16 segments for dense batches (C2); varlen ones (C4) size their runs on the
                // device to about RUN_BYTES (launch_batch), the grid covering the shortest run, or take
                // runs of 8 (r2ct) with VARLEN_RUN_BYTES 0
                c.run_bytes = varlen ? netcsum::varlen_run_bytes(t) : 0u;
                uint64_t run = !varlen ? 16u : c.run_bytes ? netcsum::kVarlenSpwMin : 8u;
                if (!varlen) {
                    // a run whose bytes are a multiple of 16 KiB (16 x 1 / 2 / 4 / 8 KiB segments) or
                    // past 48 KiB (9000-B jumbo frames) runs at 79-87 % of spec against 90-91 % for
                    // runs of about 20 KiB that are not (profiles/r6zq_seglen.jsonl: 1024 B x 16
                    // 0.2397 ms, x 20 0.2091; 4096 x 16 0.2183, x 5 0.2069; 9000 x 16 0.2359, x 2
                    // 0.2071); C2's 16 x 1500 B stays
                    const uint64_t st = a.seg_stride ? a.seg_stride : a.seg_len;
                    if ((16u * st) % 16384u == 0u || 16u * st > 49152u) {
                        run = std::max<uint64_t>(1u, (20480u + st / 2u) / st);
                        if ((run * st) % 16384u == 0u && st % 16384u != 0u) run += 1u;
                    }
                }
                if (!varlen) {                         // small batches: latency-bound runs halve until
                    while (run > 1u && (uint64_t)a.n_seg < 2048u * run) run >>= 1;   // >= 2048 waves
                }                                      // (as the packet batches, pkt_batch)
                waves = ((uint64_t)a.n_seg + run - 1u) / run;
            }
            c.stream_spw = netcsum::stream_spw(a, waves);
            c.group_lanes = 64;
            c.blocks_needed = 0;
            return c;
        }
        c.kernel = 2;                                  // varlen, sparse or short segments: general form
    }
    if (c.kernel == 5) {
        if (netcsum::small_supported(a)) {
            c.group_lanes = 1;
            c.chunks_per_pass = (int)((a.seg_len + 3u) >> 2);   // dwords per segment
            c.tile = tile >= 0 ? tile : (c.grid > 0 ? 0 : 1);   // one pass: r1u sweep (C3)
            c.nt = false;
            c.blocks_needed = 0;
            return c;
        }
        c.kernel = 2;                                  // not small / aligned: general form
    }
    if (c.kernel == 4) {
        int g = 0, p = 0, k = 0;
        if (choose_tile(a, t.group, t.chunks, &g, &p, &k)) {
            c.group_lanes = g;
            c.tile_pieces = p;
            c.chunks_per_pass = k;
            c.block = 256;                             // 4 independent waves per block
            c.blocks_needed = 0;
            c.nt = nt != 0;
            return c;
        }
        c.kernel = 2;                                  // varlen, or no instantiation fits
    }
    uint32_t chunks;                                   // worst-case 16-B chunks per segment
    if (varlen) {
        chunks = 288u;                                 // assume the C4 mean (~4.5 KB)
    } else {
        const uint32_t stride = (uint32_t)a.seg_stride;
        const uint32_t g16 = stride ? gcd_u32(stride, 16u) : 16u;
        const uint32_t maxlead = (uint32_t)((uintptr_t)a.base % g16) + (16u - g16);
        chunks = (maxlead + len_hint + 15u) >> 4;
        if (chunks == 0u) chunks = 1u;
    }
    const uint32_t kmax = (c.kernel == 2 || c.kernel == 3) ? 8u : 4u;
    int g = t.group;
    if (g == 0) {
        g = varlen ? 32 : pow2_group((chunks + kmax - 1u) / kmax);
    }
    g = pow2_group((uint32_t)g);
    c.group_lanes = g;
    int k = t.chunks;
    if (k == 0) {
        k = chunk_slots(std::min<uint32_t>(kmax, std::max<uint32_t>(1u, (chunks + (uint32_t)g - 1u) / (uint32_t)g)));
    }
    c.chunks_per_pass = k;
    c.nt = nt >= 0 ? (nt != 0) : (g >= 8);
    const uint32_t gpb = (uint32_t)(c.block / g);
    c.blocks_needed = ((uint64_t)a.n_seg + gpb - 1u) / gpb;
    return c;
}

// ----------------------------------------------------------- packet batches
// Live-piece runs span at most 63 KiB (kLiveReach): the longest run of strided slots within it.
static uint64_t live_reach_run(uint64_t stride, uint32_t pkt_len) {
    return (netcsum::kLiveReach - 128u - (uint64_t)pkt_len) / std::max<uint64_t>(stride, 1u) + 1u;
}

// The default run of the run-stream form: about `budget` bytes of slots of `per` bytes in multiples of
// 8 datagrams, 8..64 (mixed rings: 40 KB in multiples of 16).
static uint32_t pkt_default_run(int ip_ver, uint64_t per, uint64_t budget) {
    return ip_ver == 0 ? (uint32_t)std::min<uint64_t>(64u, std::max<uint64_t>(16u, (40960u / per) & ~15ull))
                       : (uint32_t)std::min<uint64_t>(64u, std::max<uint64_t>(8u, (budget / per) & ~7ull));
}

static bool tile_run(int tile) { return tile > 0 && tile <= 64; }   // TUNE_TILE sets the run length

NET_ERR pkt_decide(const Tune& t, const PktJob& j, PktPlan& p) {
    const bool tx = j.tx;
    const int ip_ver = j.ip_ver;
    netcsum::PktBatchArgs& a = p.a;
    a.base = static_cast<const uint8_t*>(j.base);
    a.off = j.off;
    a.len = j.len;
    a.stride = j.stride;
    a.len_u = j.pkt_len;
    a.n = j.n;
    a.flags_out = j.flags;
    a.udp_tx_csum = j.udp_mode;
    a.action_out = tx ? nullptr : j.action;
    a.rx_cfg = j.rx_cfg;
    if (tx) {
        a.fieldpos_out = j.fieldpos;
    } else {
        a.sums_out = reinterpret_cast<uint32_t*>(j.sums);
    }
    netcsum::LaunchCfg& c = p.c;
    const uint32_t chunks = j.off ? 288u : ((uint32_t)j.pkt_len + 30u) / 16u;
    int g = t.group;
    if (g < 8) {
        g = j.off ? 32 : std::max(8, pow2_group((chunks + 5u) / 6u));
    }
    c.group_lanes = pow2_group((uint32_t)g);
    c.chunks_per_pass = (int)std::min<uint32_t>(8u, std::max<uint32_t>(1u, (chunks + c.group_lanes - 1u) / c.group_lanes));
    // Strided batches store through a buffer resource based at each wave's first packet of a stage,
    // reaching the stage's other 64/G - 1 packets by 32-bit offsets (netcsum_packets.hip pkt_store):
    // a stride that would wrap them is refused, never silently mis-addressed.
    if (j.off == nullptr && (uint64_t)(64u / (uint32_t)c.group_lanes - 1u) * j.stride + 65536u >= 0xFFFFFFFFull) {
        return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
    }
    // Rx streams with nt loads; Tx re-writes header lines it has just read and is faster with plain
    // loads (profiles/r1tc_tx_sweep.jsonl: 0.323 vs 0.356 ms at tile 2).
    c.nt = t.nt >= 0 ? (t.nt != 0) : !tx;
    c.grid = t.grid;
    const int tile = t.tile;
    // Run-stream form (netcsum_pktstream.hip) for dense strided IPv4 batches unless the lane-group
    // kernel is forced (TUNE_KERNEL 2); TILE > 0 sets its packets per wave run (default 16).
    // Defaults from the r2tx sweep (tools/pkt_stream_probe.py, 1 M x 1500-B IPv4/TCP): runs of 8
    // packets, 4 pieces in flight, nt loads (Rx 0.215 ms); Tx in two passes (checksum pass writing
    // 8-B records + scatter pass: 0.288 ms against 0.296 for in-pass field writes). Mixed rings run
    // both parses in a wave whose lanes disagree on the version, and a run of 16 spreads that over
    // twice the bytes (profiles/r2zb_pkt_stream_mixed_v6_v4.jsonl, alternating ring: Rx 0.243 ->
    // 0.2185 ms, Tx 0.302 -> 0.292); IPv4 and IPv6 alone stay at 8 (16: +0.9 % / +0.2 %). Shorter
    // datagrams need longer runs (a run's cost is per datagram event AND per wave): about 20 KB per
    // run in multiples of 8 datagrams, 8..64 (40 KB in multiples of 16 for mixed rings); r2zq sweep
    // (tools/pkt_run_probe.py): Rx of 256-B datagrams 0.891 -> 0.567 ms, 576-B 0.424 -> 0.29,
    // 1000-B 0.259 -> 0.222; 1500-B keeps 8.
    // IPv6 / mixed batches through the lane-group kernel: a second pass walks the extension-header
    // chains the batch kernel left as EXT_HDR (netcsum_v6walk.hip). It reads the flags, so a Tx batch
    // without d_flags gets them in the stream's scratch buffer. (The run-stream path walks them
    // inside its own launches.)
    // (an Rx burst without d_flags keeps them there too, or nowhere for IPv4, whose kernels write
    // each action directly)
    p.walk = ip_ver != 4;
    p.own_flags = p.walk && j.flags == nullptr;
    // Which bytes of each slot are read (NETCSUM_TUNE_PKT_BOUND, netcsum_pktstream.hip): by default the
    // whole span for packed batches (0), else the live pieces with piece 0 loaded during the parse (2;
    // since the one-mask sentinel pop it beats form 3 on every ring layout, profiles/r4m_ring_probe.jsonl:
    // 1520-B slots at +14, 1500-B datagrams 0.2177 against 0.2197 ms, the mixed ring 0.1532 against
    // 0.1583, 2-KiB slots at +64 0.2522 against 0.2677); a burst read in place from host memory may
    // prefer the whole-span form 0 (bound_pref: one PCIe round trip). Live-piece runs span at most
    // 63 KiB (kLiveReach).
    p.d = t.chunks == 8 ? 8 : 4;
    // (a packed batch, stride == pkt_len, says every byte is datagram: nothing to skip, form 0;
    // r4f ring probe: 1 M x 1500 B Rx 0.2145 ms against 0.2188 in form 3)
    p.dense = j.off == nullptr && j.stride <= (uint64_t)j.pkt_len + 64u;
    const bool packed = j.off == nullptr && j.stride == (uint64_t)j.pkt_len;
    const int tb0 = t.pkt_bound;
    p.bound_default = tb0 < 0 || tb0 == 4;                  // (4: ring plans, else as the default)
    int bound = !p.bound_default ? tb0 : (packed ? 0 : 2);
    if (j.bound_pref >= 0 && p.bound_default) {             // the caller's preference, where it applies
        if (netcsum::pkt_stream_supported(a, ip_ver, j.bound_pref)) bound = j.bound_pref;
    }
    if (p.d == 8 && bound == 1) bound = 2;                  // (8 pieces in flight: forms 0, 2, 3)
    if (!netcsum::pkt_stream_supported(a, ip_ver, bound) && bound >= 1 && p.dense && p.bound_default) {
        bound = 0;                                          // datagrams > 64384 B: past the bitmap's reach
    }
    p.bound = bound;
    p.stream = t.kernel != 2 && netcsum::pkt_stream_supported(a, ip_ver, bound);
    if (!p.stream) {
        a.tile = tile >= 0 ? (uint32_t)tile : (c.grid > 0 ? 0u : 2u);      // tile 2: best Rx/Tx point (r1m sweep)
        return NET_UTIL_ERR_NONE;
    }
    // offset/length runs: 16 datagrams (their lengths are on the device; the device checks each
    // run's order and reach, and takes a run datagram by datagram otherwise)
    // the live-piece forms parse first, so their runs are longer: about 24 KB of strided span, which
    // gives 1520-B slots runs of 16 (the mixed 40/576/1500-B ring: 0.1532 ms against 0.1921 for 8)
    // and 2-KiB slots runs of 8 (0.2522 against 0.2627 for 16; profiles/r4m_ring_probe.jsonl);
    // offset/length runs 16 (32: 64 KiB of 2-KiB slots, past the reach)
    const uint64_t per = j.off ? 2048u : std::max<uint64_t>(a.stride, 1u);
    const uint64_t budget = bound == 0 ? 20480u : j.off ? 32768u : 24576u;
    uint32_t run = pkt_default_run(ip_ver, per, budget);
    // dense IPv4 / IPv6 runs of long datagrams: a run of 8 whose bytes are a multiple of 16 KiB or
    // past 48 KiB (2 / 4 / 8 KiB, 9000-B datagrams) runs at 78-88 % of spec, runs of about 10 KiB at
    // 88-92 % (profiles/r6zu_pktlen.jsonl: 2048 B x 8 0.2120 ms, x 5 0.2046; 4096 x 8 0.2219, x 2
    // 0.2050; 8192 x 8 0.2393, x 1 0.2042; 9000 x 8 0.2166, x 1 0.2138); 1500 B keeps its 8
    if (ip_ver != 0 && bound == 0 && !j.off && ((uint64_t)run * per % 16384u == 0u || (uint64_t)run * per > 49152u)) {
        run = (uint32_t)std::max<uint64_t>(1u, 10240u / per);
    }
    // small batches (NIC bursts) are latency-bound: a run costs ~run x len / 4 KiB memory round
    // trips, so runs halve until the batch spreads over >= 2048 waves (burst of 256 mixed frames:
    // Rx 19.9 -> 13.3 us, Tx 22.8 -> 15.7 us; 16 Ki frames: runs of 8, 19.2 -> 17.2 us;
    // profiles/r3t_burst_run_probe.jsonl); batches of >= 2048 runs keep the run length above
    p.spw = tile_run(tile) ? (uint32_t)tile : run;
    if (!tile_run(tile)) {
        while (p.spw > 1u && (uint64_t)j.n < 2048ull * p.spw) p.spw >>= 1;
    }
    // The ring's plan (netcsum_pktstream.hip pkt_plan_block): for strided batches that are not
    // packed — by default from 16 Ki datagrams (smaller ones are bursts, latency-bound, with the
    // runs halved above), always with TUNE_PKT_BOUND 4 — the launch samples its datagrams in one
    // extra block and leaves the form and run length for the next batch on the same ring (same
    // base, stride, bytes present, count, IP version) in coherent host memory; a batch whose ring
    // has a plan runs in it, the first one in the host's default above.
    // Offset/length batches take ring plans too, keyed on their descriptor arrays: the run length
    // (by the streamed bytes, capped by the sampled pitch to the reach) and the residency.
    // (NETCSUM_TUNE_STREAM_WAVES set: measurements of fixed residencies take no plans)
    p.plan_ring = !packed && j.bound_pref < 0 && p.d == 4 && !tile_run(tile) &&
                  (tb0 == 4 || (tb0 < 0 && j.n >= 16384u)) && j.rec_only == nullptr &&
                  !netcsum::stream_waves_tuned(t) && netcsum::pkt_stream_supported(a, ip_ver, 2);
    if (p.plan_ring) {
        if (j.off == nullptr && netcsum::pkt_stream_supported(a, ip_ver, 0)) {
            p.run0 = pkt_default_run(ip_ver, per, 20480u);
            while (p.run0 > 1u && (uint64_t)j.n < 2048ull * p.run0) p.run0 >>= 1;
        }
        p.cap = j.off ? 64u : live_reach_run(j.stride, j.pkt_len);
        p.cap = std::min<uint64_t>(p.cap, std::max<uint64_t>(8u, ((uint64_t)j.n / 2048u) & ~7ull));
        p.cap = std::min<uint64_t>(p.cap, 64u);
    }
    p.snt = t.nt >= 0 ? (t.nt != 0) : true;
    // Tx passes: auto = two (8-B records, then a scatter pass: 1 M x 1500 B 0.2918 against 0.2954
    // ms in one pass) from 64 Ki datagrams up, one below (a burst is then a single launch)
    p.two = tx && (j.rec_only != nullptr || t.tx_passes == 2 || (t.tx_passes == 0 && j.n >= 65536u));
    return NET_UTIL_ERR_NONE;
}

// The run-stream form's last word: a live-piece run kept within the reach, and the launch's name.
void pkt_settle(const Tune& t, const PktJob& j, PktPlan& p) {
    // IPv6 / mixed: the Rx and one-pass Tx kernels, and two-pass Tx's scatter pass, finish their
    // deferred datagrams themselves (no deferral word, no walk launch, no flags in scratch)
    if (p.bound >= 1 && j.off == nullptr) {            // (the device plan sizes its own runs)
        const uint64_t cap = live_reach_run(j.stride, j.pkt_len);
        if (p.spw > cap && t.tile > 0 && p.bound_default && p.dense) {
            p.bound = 0;                                  // a run length asked for: the whole-span form
        } else {
            p.spw = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(p.spw, cap));
        }
    }
    snprintf(p.desc, sizeof p.desc, "pkt_stream_kernel<D=%d%s,%s,%s%s> block=256 pkts_per_wave=%u bound=%d%s%s%s%s%s", p.d,
             p.snt ? ",nt" : "", j.tx ? "tx" : "rx", j.ip_ver == 4 ? "v4" : j.ip_ver == 6 ? "v6" : "mixed",
             !j.tx && p.a.sums_out ? ",sums" : "", p.spw, p.bound,
             j.off ? (p.vl_inline ? " offlen (inline fallback)" : " offlen +pkt_vl_deferred_kernel") : "",
             p.two ? " +pkt_scatter_kernel" : "", p.walk ? " +inline_v6_walk" : "", p.plan_note, p.ahead_note);
}

// ----------------------------------------------------------- host bursts
// The server's form for a burst (BurstPost::form >> 1 and its run length), or false when the burst is
// outside the run-stream kernel's domain (the launch path takes it).
// The server's run length: one run per wave of the grid until the runs reach 16 frames (Ether bursts,
// whose datagrams the server's waves find themselves, take it as it is: their tail is the offset/length
// form's, which fits any layout).
uint32_t server_run(uint32_t n_pkt) {
    return std::max<uint32_t>(1u, std::min<uint32_t>(16u, (n_pkt + 4u * kServerBlocks - 1u) / (4u * kServerBlocks)));
}

bool server_form(const uint64_t* h_off, uint64_t stride, CPU_INT16U pkt_len, uint32_t n_pkt, uint32_t* form, uint32_t* spw) {
    netcsum::PktBatchArgs a{};
    a.off = h_off;
    a.len = reinterpret_cast<const uint16_t*>(h_off);     // (only tested against nullptr)
    a.stride = stride;
    a.len_u = pkt_len;
    a.n = n_pkt;
    uint32_t run = server_run(n_pkt);
    if (h_off != nullptr) {
        *form = netcsum::kBurstOffLen;
        if (!netcsum::pkt_stream_supported(a, 0, 2)) return false;
    } else if (stride <= (uint64_t)pkt_len + 64u && netcsum::pkt_stream_supported(a, 0, 0)) {
        *form = netcsum::kBurstWhole;                   // (kBurstBound: one PCIe round trip)
    } else if (netcsum::pkt_stream_supported(a, 0, 2)) {
        *form = netcsum::kBurstLive;
        run = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(run, live_reach_run(stride, pkt_len)));
    } else {
        return false;
    }
    *spw = run;
    return true;
}

}  // namespace nchost
