// ipparse_caller.cpp — the packet kernels' IP parse and verdict rules (uc-tcp-ip_amd/csrc/netcsum_ipparse.h)
// run on the CPU, as plain C++: the same header the three kernels include, with a window accessor
// over a byte array that refuses every read outside the window it was given.
//
// stdin, one datagram per line:
//     <hex octets | -> <avail> <limit> <tx 0|1> <udp_tx_csum 0|1|2> <sums 0|1> [<walk nh> <walk off>]
// avail: octets present; limit: octets of the datagram the "kernel" can read without a dependent load.
// With the last two fields the line is judged as the extension-header walk judges a datagram whose
// chain it has walked to next header nh at offset off (the transport and verdict steps alone, the window
// being the whole datagram). Per line, stdout:
//     DEFER                                      the window rules leave it to the walk pass
//     <flags> <cip|-> <cl4|-> <l4 field offset|-> <fragment sum> <fragment octets>     (hex, hex, hex, dec, hex, dec)
// The sums are taken here with a byte loop over exactly the octets the classification describes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "netcsum_ipparse.h"

namespace ip = netcsum::ip;

namespace {

struct ByteWindow {
    const uint8_t* p;
    uint32_t       avail, lim;
    uint32_t limit() const { return lim; }
    template <int MinOff>
    uint32_t dword(uint32_t off) const {
        if (off < 16u * (uint32_t)MinOff || off + 4u > lim || off + 4u > avail) {
            std::fprintf(stderr, "read of [%u, %u) outside the window (MinOff %d, limit %u, avail %u)\n", off, off + 4u, MinOff,
                         lim, avail);
            std::exit(3);
        }
        return (uint32_t)p[off] | ((uint32_t)p[off + 1u] << 8) | ((uint32_t)p[off + 2u] << 16) | ((uint32_t)p[off + 3u] << 24);
    }
};

uint32_t fold16(uint32_t s) {
    s = (s & 0xFFFFu) + (s >> 16);
    return (s & 0xFFFFu) + (s >> 16);
}

// Little-endian half-word sum of octets [lo, hi) (lo even), the two octets at `skip` counted as zero, folded.
uint32_t sum_le(const std::vector<uint8_t>& b, uint32_t lo, uint32_t hi, uint32_t skip) {
    uint32_t s = 0u;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t v = (skip != ~0u && (i == skip || i == skip + 1u)) ? 0u : b[i];
        s = fold16(s + (((i - lo) & 1u) ? v << 8 : v));
    }
    return s;
}

uint32_t head_dword(const std::vector<uint8_t>& b, uint32_t avail, uint32_t off) {   // octets past avail: 0
    uint32_t d = 0u;
    for (uint32_t k = 0u; k < 4u; ++k) {
        d |= (off + k < avail ? (uint32_t)b[off + k] : 0u) << (8u * k);
    }
    return d;
}

template <bool TX>
void judge(const std::vector<uint8_t>& b, uint32_t avail, uint32_t limit, uint32_t udp_mode, bool sums, int walk_nh,
           uint32_t walk_off) {
    const ByteWindow w{b.data(), avail, limit};
    const uint32_t d0 = head_dword(b, avail, 0u), d1 = head_dword(b, avail, 4u);
    ip::Class c{};
    if (walk_nh >= 0) {                                          // as walk_one: the chain is walked already
        c.v6 = true;
        c.tot = 40u + ip::be16(d1, 0);
        c.l4_csum_off = ~0u;
        c.proto = (uint32_t)walk_nh;
        c.l4_off = walk_off;
        ip::transport<TX, true, 0>(ByteWindow{b.data(), avail, c.tot}, udp_mode, 0u, c);
    } else if (((d0 >> 4) & 0xFu) == 6u) {                       // mixed batches: by the version nibble
        c = ip::classify6<TX, 2>(w, avail, udp_mode, d0, d1);
    } else {
        const uint32_t d2 = head_dword(b, avail, 8u), d3 = head_dword(b, avail, 12u), d4 = head_dword(b, avail, 16u);
        c = ip::classify4<TX, 1>(w, avail, udp_mode, d0, d1, d2, d3, d4);
        // the run-stream lane's way: the header step alone, then the transport step called by itself
        ip::Class s = ip::classify4<TX, 1, ByteWindow, false>(w, avail, udp_mode, d0, d1, d2, d3, d4);
        if (s.l4_off != 0u && s.frag_off == 0u) {
            ip::transport<TX, false, 1>(w, udp_mode, ip::addr4_le(d3, d4), s);
        }
        if (s.flags != c.flags || s.proto != c.proto || s.l4_off != c.l4_off || s.tot != c.tot || s.l4_csum_off != c.l4_csum_off ||
            s.pseudo_le != c.pseudo_le || s.frag_off != c.frag_off || s.frag_len != c.frag_len || s.check_l4 != c.check_l4 ||
            s.pseudo != c.pseudo) {
            std::fprintf(stderr, "IPv4: header step + transport step differ from the whole classification\n");
            std::exit(4);
        }
    }
    if ((c.flags & NETCSUM_PKT_EXT_HDR) || (sums && c.frag_walk)) {
        std::puts("DEFER");
        return;
    }
    uint32_t sip = 0u, sl4 = 0u;
    if (!ip::malformed(c) && !c.v6) {
        sip = sum_le(b, 0u, c.l4_off, TX ? 10u : ~0u);
    }
    if (c.check_l4) {
        sl4 = sum_le(b, c.l4_off, c.tot, TX ? c.l4_csum_off : ~0u);
        if (c.v6 && c.pseudo) {
            sl4 = fold16(sl4 + sum_le(b, 8u, 40u, ~0u));         // the addresses
        }
        sl4 = fold16(sl4 + c.pseudo_le);
    }
    const ip::Verdict v = ip::verdict<TX>(c, sip, sl4);
    uint32_t fsum = 0u, flen = 0u;
    if (sums && c.frag_len != 0u) {
        fsum = sum_le(b, c.frag_off, c.tot, ~0u);
        flen = c.frag_len;
    }
    char cip[16] = "-", cl4[16] = "-", fo[16] = "-";
    if (v.cip != ~0u) std::snprintf(cip, sizeof cip, "%x", v.cip);
    if (v.cl4 != ~0u) std::snprintf(cl4, sizeof cl4, "%x", v.cl4);
    if (c.l4_csum_off != ~0u) std::snprintf(fo, sizeof fo, "%u", c.l4_csum_off);
    std::printf("%x %s %s %s %x %u\n", v.flags, cip, cl4, fo, fsum, flen);
}

int hexval(char ch) {
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
    return -1;
}

}  // namespace

int main() {
    std::vector<char> buf(1 << 18);
    while (std::fgets(buf.data(), (int)buf.size(), stdin)) {
        char* sp = std::strchr(buf.data(), ' ');
        if (!sp) return 2;
        std::vector<uint8_t> b;
        if (buf[0] != '-') {
            for (const char* q = buf.data(); q + 1 < sp; q += 2) {
                const int hi = hexval(q[0]), lo = hexval(q[1]);
                if (hi < 0 || lo < 0) return 2;
                b.push_back((uint8_t)(hi * 16 + lo));
            }
        }
        unsigned avail, limit, tx, udp, sums;
        int wnh = -1;
        unsigned woff = 0;
        const int got = std::sscanf(sp, "%u %u %u %u %u %d %u", &avail, &limit, &tx, &udp, &sums, &wnh, &woff);
        if ((got != 5 && got != 7) || avail > b.size()) return 2;
        b.resize(avail);                                         // ASan guards every octet past `avail`
        b.shrink_to_fit();
        if (tx) {
            judge<true>(b, avail, limit, udp, sums != 0u, wnh, woff);
        } else {
            judge<false>(b, avail, limit, udp, sums != 0u, wnh, woff);
        }
    }
    return 0;
}
