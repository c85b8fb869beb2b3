// hostplan_caller.cpp — a stand-alone check of uc-tcp-ip_amd/csrc/netcsum_hostplan.h (no HIP, no device):
// the chunk planner, the slot layout and the two Tx record appliers against values worked out here by
// brute force or written down as literals. Usage: hostplan_caller plan | layout | records. Prints one line
// "ok <checks>" and exits 0, or names the first failing check on stderr and exits 1.
// Built and run by tests/test_hostplan_cpu.py with -fsanitize=address,undefined -Wall -Wextra -Werror.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "netcsum_hostplan.h"

using namespace nchost;

static long g_checks = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++g_checks;                                       \
        if (!(cond)) {                                    \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            exit(1);                                      \
        }                                                 \
    } while (0)

// ---------------------------------------------------------------------------------------------- planner
static int test_plan() {
    const uint32_t ns[] = {1, 2, 7, 29}, chunks[] = {0, 1, 3, 7, 64};
    const uint64_t stride = 1520;
    const uint32_t fixed = 1514;
    for (uint32_t n : ns) {
        // offsets out of order (a permutation of slots of 1600 octets, from +3), one length zero
        std::vector<uint64_t> off(n);
        std::vector<uint16_t> len(n);
        for (uint32_t i = 0; i < n; ++i) {
            off[i] = 3u + 1600ull * ((i * 5u + 2u) % n);        // (5 is coprime to 1, 2, 7, 29)
            len[i] = (uint16_t)(60u + 97u * i);
        }
        len[n / 2] = 0;
        for (uint32_t nc : chunks) {
            for (int shape = 0; shape < 4; ++shape) {            // neither, both, lengths only, offsets only
                const uint64_t* o = (shape == 1 || shape == 3) ? off.data() : nullptr;
                const uint16_t* l = (shape == 1 || shape == 2) ? len.data() : nullptr;
                const ChunkPlan p = plan_chunks(o, l, stride, fixed, n, nc);
                uint32_t want_nc = nc == 0 ? 1u : nc;
                if (want_nc > n) want_nc = n;
                uint32_t per = 1;                                // the smallest per with per * want_nc >= n
                while ((uint64_t)per * want_nc < n) ++per;
                CHECK(p.per == per, "n %u chunks %u shape %d: per %u, want %u", n, nc, shape, p.per, per);
                CHECK(!p.ch.empty() && p.ch.size() <= want_nc, "n %u chunks %u: %zu chunks", n, nc, p.ch.size());
                uint32_t next = 0;
                uint64_t maxb = 0;
                for (size_t k = 0; k < p.ch.size(); ++k) {
                    const HostChunk& q = p.ch[k];
                    CHECK(q.s0 == next && q.ns >= 1, "n %u chunks %u: chunk %zu starts at %u, want %u", n, nc, k, q.s0, next);
                    if (k + 1 < p.ch.size()) CHECK(q.ns == per, "n %u chunks %u: chunk %zu has %u items", n, nc, k, q.ns);
                    uint64_t lo = ~0ull, hi = 0;
                    for (uint32_t i = q.s0; i < q.s0 + q.ns; ++i) {
                        const uint64_t at = o ? off[i] : (uint64_t)i * stride, ln = l ? len[i] : fixed;
                        if (at < lo) lo = at;
                        if (at + ln > hi) hi = at + ln;
                    }
                    CHECK(q.lo == lo && q.hi == hi, "n %u chunks %u shape %d chunk %zu: [%llu, %llu), want [%llu, %llu)", n, nc,
                          shape, k, (unsigned long long)q.lo, (unsigned long long)q.hi, (unsigned long long)lo,
                          (unsigned long long)hi);
                    if (hi - lo > maxb) maxb = hi - lo;
                    next += q.ns;
                }
                CHECK(next == n, "n %u chunks %u: the chunks cover %u items", n, nc, next);
                CHECK(p.max_span == maxb, "n %u chunks %u shape %d: max span %llu, want %llu", n, nc, shape,
                      (unsigned long long)p.max_span, (unsigned long long)maxb);
            }
        }
    }
    // a chunk of empty items only: lo == hi
    const uint64_t off0[2] = {40, 8};
    const uint16_t len0[2] = {0, 0};
    const ChunkPlan z = plan_chunks(off0, len0, 0, 0, 2, 2);
    CHECK(z.ch.size() == 2 && z.ch[0].lo == 40 && z.ch[0].hi == 40 && z.ch[1].lo == 8 && z.max_span == 0, "empty items");
    CHECK(plan_chunks(nullptr, nullptr, 8, 8, 0, 3).ch.empty(), "no items, no chunks");
    // descriptor staging: offsets rebased to lo, lengths copied, an absent array untouched
    {
        const uint64_t o[5] = {900, 100, 500, 300, 700};
        const uint16_t l[5] = {1, 2, 3, 4, 5};
        const HostChunk q = chunk_span(o, l, 0, 0, 1, 3);
        uint64_t so[3] = {7, 7, 7};
        uint16_t sl[3] = {9, 9, 9};
        stage_descriptors(o, l, q, so, sl);
        CHECK(q.lo == 100 && so[0] == 0 && so[1] == 400 && so[2] == 200 && sl[0] == 2 && sl[1] == 3 && sl[2] == 4, "staged both");
        uint64_t so2[3] = {7, 7, 7};
        stage_descriptors(nullptr, l, q, so2, sl);
        CHECK(so2[0] == 7 && so2[2] == 7, "no offsets: nothing written");
        uint16_t sl2[3] = {9, 9, 9};
        stage_descriptors(o, nullptr, q, so, sl2);
        CHECK(sl2[0] == 9 && sl2[2] == 9, "no lengths: nothing written");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- layout
static size_t A(size_t x) { return (x + 255u) / 256u * 256u; }   // (this file's own rounding)

struct Takes {
    std::vector<size_t> bytes, off;
    SlotLayout          lay;
    size_t take(size_t b) {
        bytes.push_back(b);
        off.push_back(lay.take(b));
        return off.back();
    }
};

static void check_regions(const Takes& t, const char* what) {
    size_t end = 0;
    for (size_t i = 0; i < t.off.size(); ++i) {
        CHECK(t.off[i] % 256u == 0, "%s: region %zu at %zu", what, i, t.off[i]);
        CHECK(t.off[i] >= end, "%s: region %zu at %zu overlaps the one before (ends %zu)", what, i, t.off[i], end);
        if (t.bytes[i]) end = t.off[i] + t.bytes[i];
        if (i) CHECK(t.off[i] >= t.off[i - 1], "%s: region %zu out of order", what, i);
    }
    CHECK(t.lay.total() >= end && t.lay.total() % 256u == 0, "%s: total %zu, last region ends %zu", what, t.lay.total(), end);
}

// The offsets in request order and the total, as literal numbers (worked out by hand from the forms' former
// chains of al256 sums at per = 5 and a span of 7595 octets: 7680 for the bytes, 256 for every other region
// that is present). `need`: what the form asked ensure_pipe for before, which the total must cover.
static void expect(const Takes& t, std::initializer_list<size_t> off, size_t total, size_t need, const char* what) {
    CHECK(t.off == std::vector<size_t>(off), "%s: offsets differ from the literals", what);
    CHECK(t.lay.total() == total && total >= need, "%s: total %zu, want %zu (the form needs %zu)", what, t.lay.total(), total, need);
}

static int test_layout() {
    {
        Takes t;
        CHECK(t.take(0) == 0 && t.take(0) == 0 && t.lay.total() == 0, "empty regions take no room");
        CHECK(t.take(1) == 0 && t.take(256) == 256 && t.take(257) == 512 && t.take(0) == 1024 && t.take(5) == 1024, "order");
        CHECK(t.lay.total() == 1280, "total %zu", t.lay.total());
        check_regions(t, "plain");
    }
    // The five forms' slots at per = 5 and a chunk span of 7595 octets, without (opt 0) and with (opt 1) their
    // optional parts, against the sums of al256 as the forms wrote them out before the layout helper.
    const size_t per = 5, maxb = 7595;
    for (int opt = 0; opt < 2; ++opt) {
        {   // ChkSumBatchStridedHost: [segment bytes | pseudo-headers | outputs]; opt: pseudo-headers of 12 octets at stride 16
            const size_t ph_bytes = opt ? (per - 1u) * 16u + 12u : 0u, out_elt = 2;
            Takes d;
            d.take(maxb);
            const size_t o_ph = d.take(ph_bytes), o_out = d.take(per * out_elt);
            const size_t w_ph = A(maxb), w_out = w_ph + A(ph_bytes);
            CHECK(o_ph == w_ph && o_out == w_out && d.lay.total() == w_out + A(per * out_elt), "strided opt %d", opt);
            if (opt) expect(d, {0, 7680, 7936}, 8192, 8192, "strided with pseudo-headers");
            else expect(d, {0, 7680, 7680}, 7936, 7936, "strided");
            check_regions(d, "strided");
        }
        {   // ChkSumBatchVarLenHost: [bytes | offsets | lengths | pseudo-headers | outputs]; host [offsets | lengths]
            const size_t ph_bytes = opt ? (per - 1u) * 16u + 12u : 0u, elt = 1;
            Takes d, h;
            d.take(maxb);
            const size_t o_off = d.take(per * 8u), o_len = d.take(per * 2u), o_ph = d.take(ph_bytes), o_out = d.take(per * elt);
            const size_t hs_off = h.take(per * 8u), hs_len = h.take(per * 2u);
            const size_t w_off = A(maxb), w_len = w_off + A(per * 8u), w_ph = w_len + A(per * 2u), w_out = w_ph + A(ph_bytes);
            CHECK(o_off == w_off && o_len == w_len && o_ph == w_ph && o_out == w_out && d.lay.total() == w_out + A(per * elt),
                  "varlen opt %d", opt);
            CHECK(hs_off == 0 && hs_len == A(per * 8u) && h.lay.total() >= A(per * 8u) + per * 2u, "varlen host");
            if (opt) expect(d, {0, 7680, 7936, 8192, 8448}, 8704, 8704, "varlen with pseudo-headers");
            else expect(d, {0, 7680, 7936, 8192, 8192}, 8448, 8448, "varlen");
            expect(h, {0, 256}, 512, 266, "varlen host");
            check_regions(d, "varlen");
            check_regions(h, "varlen host");
        }
        for (int varlen = 0; varlen < 2; ++varlen) {
            // packet batches: [bytes | offsets | lengths | flags | actions | field positions | records | fragment sums];
            // host [offsets | lengths | records]; opt 0: Rx, opt 1: Tx, and Rx with sums
            for (int tx = 0; tx <= opt; ++tx) {
                const bool sums = opt && !tx;
                Takes d, h;
                d.take(maxb);
                const size_t o_off = d.take(varlen ? per * 8u : 0u), o_len = d.take(varlen ? per * 2u : 0u);
                const size_t o_fl = d.take(per), o_act = d.take(per);
                const size_t o_fp = d.take(tx ? per * 4u : 0u), o_rec = d.take(tx ? per * 8u : 0u);
                const size_t o_sum = d.take(sums ? per * 4u : 0u);
                h.take(varlen ? per * 8u : 0u);
                const size_t hs_len = h.take(varlen ? per * 2u : 0u), hs_rec = h.take(tx ? per * 8u : 0u);
                const size_t w_off = A(maxb), w_len = w_off + A(varlen ? per * 8u : 0u);
                const size_t w_fl = w_len + A(varlen ? per * 2u : 0u), w_act = w_fl + A(per);
                const size_t w_fp = w_act + A(per), w_rec = w_fp + A(tx ? per * 4u : 0u);
                const size_t wh_rec = varlen ? A(per * 8u) + A(per * 2u) : 0u;
                const size_t w_sum = w_rec + A(tx ? per * 8u : 0u);
                CHECK(o_off == w_off && o_len == w_len && o_fl == w_fl && o_act == w_act && o_fp == w_fp && o_rec == w_rec &&
                          o_sum == w_sum && d.lay.total() == w_sum + A(sums ? per * 4u : 0u),
                      "packets varlen %d tx %d sums %d", varlen, tx, (int)sums);
                CHECK(hs_rec == wh_rec && hs_len == (varlen ? 256u : 0u) && h.lay.total() >= wh_rec + (tx ? per * 8u : 0u),
                      "packets host varlen %d tx %d", varlen, tx);
                CHECK((h.lay.total() != 0) == (varlen || tx), "packets: the host slot is empty exactly for fixed-length Rx");
                if (!varlen && !tx) expect(d, {0, 7680, 7680, 7680, 7936, 8192, 8192, 8192}, sums ? 8448 : 8192, sums ? 8448 : 8192, "packets rx");
                if (!varlen && tx) expect(d, {0, 7680, 7680, 7680, 7936, 8192, 8448, 8704}, 8704, 8704, "packets tx");
                if (varlen && !tx) expect(d, {0, 7680, 7936, 8192, 8448, 8704, 8704, 8704}, sums ? 8960 : 8704, sums ? 8960 : 8704, "packets rx offlen");
                if (varlen && tx) expect(d, {0, 7680, 7936, 8192, 8448, 8704, 8960, 9216}, 9216, 9216, "packets tx offlen");
                if (!varlen && !tx) expect(h, {0, 0, 0}, 0, 0, "packets rx host");
                if (!varlen && tx) expect(h, {0, 0, 0}, 256, 40, "packets tx host");
                if (varlen && !tx) expect(h, {0, 256, 512}, 512, 512, "packets rx offlen host");
                if (varlen && tx) expect(h, {0, 256, 512}, 768, 552, "packets tx offlen host");
                check_regions(d, "packets");
                check_regions(h, "packets host");
            }
        }
        for (int shape = 0; shape < 4; ++shape) {                // neither, both, lengths only, offsets only
            const bool has_off = shape == 1 || shape == 3, has_len = shape == 1 || shape == 2;
            {   // RxBurstEtherHost: [bytes | offsets | lengths | flags | actions | classes | fragment sums]; host [offsets | lengths]
                Takes d, h;
                d.take(maxb);
                const size_t o_off = d.take(has_off ? per * 8u : 0u), o_len = d.take(has_len ? per * 2u : 0u);
                const size_t o_fl = d.take(per), o_act = d.take(per), o_l2 = d.take(per), o_sum = d.take(opt ? per * 4u : 0u);
                h.take(has_off ? per * 8u : 0u);
                const size_t hs_len = h.take(has_len ? per * 2u : 0u);
                const size_t w_off = A(maxb), w_len = w_off + A(has_off ? per * 8u : 0u);
                const size_t w_fl = w_len + A(has_len ? per * 2u : 0u), w_act = w_fl + A(per), w_l2 = w_act + A(per);
                const size_t w_sum = w_l2 + A(per);
                const size_t wh_len = A(has_off ? per * 8u : 0u);
                CHECK(o_off == w_off && o_len == w_len && o_fl == w_fl && o_act == w_act && o_l2 == w_l2 && o_sum == w_sum &&
                          d.lay.total() == w_sum + A(opt ? per * 4u : 0u),
                      "ether rx shape %d opt %d", shape, opt);
                CHECK(hs_len == wh_len && h.lay.total() == wh_len + A(has_len ? per * 2u : 0u), "ether rx host shape %d", shape);
                CHECK((h.lay.total() != 0) == (has_off || has_len), "ether rx: host slot empty exactly without descriptors");
                const size_t fl_at[4] = {7680, 8192, 7936, 7936}, len_at[4] = {7680, 7936, 7680, 7936};   // by shape
                const size_t f = fl_at[shape], tot = f + (opt ? 1024u : 768u);
                expect(d, {0, 7680, len_at[shape], f, f + 256, f + 512, f + 768}, tot, tot, "ether rx");
                const size_t hlen_at[4] = {0, 256, 0, 256}, htot[4] = {0, 512, 256, 256};
                expect(h, {0, hlen_at[shape]}, htot[shape], htot[shape], "ether rx host");
                check_regions(d, "ether rx");
                check_regions(h, "ether rx host");
            }
            if (opt) continue;
            {   // TxBurstEtherHost: [bytes | offsets | lengths | flags | classes | field positions | records]; host [offsets | lengths | records]
                Takes d, h;
                d.take(maxb);
                const size_t o_off = d.take(has_off ? per * 8u : 0u), o_len = d.take(has_len ? per * 2u : 0u);
                const size_t o_fl = d.take(per), o_l2 = d.take(per), o_fp = d.take(per * 4u), o_rec = d.take(per * 8u);
                h.take(has_off ? per * 8u : 0u);
                const size_t hs_len = h.take(has_len ? per * 2u : 0u), hs_rec = h.take(per * 8u);
                const size_t w_off = A(maxb), w_len = w_off + A(has_off ? per * 8u : 0u);
                const size_t w_fl = w_len + A(has_len ? per * 2u : 0u), w_l2 = w_fl + A(per);
                const size_t w_fp = w_l2 + A(per), w_rec = w_fp + A(per * 4u);
                const size_t wh_len = A(has_off ? per * 8u : 0u), wh_rec = wh_len + A(has_len ? per * 2u : 0u);
                CHECK(o_off == w_off && o_len == w_len && o_fl == w_fl && o_l2 == w_l2 && o_fp == w_fp && o_rec == w_rec &&
                          d.lay.total() == w_rec + A(per * 8u),
                      "ether tx shape %d", shape);
                CHECK(hs_len == wh_len && hs_rec == wh_rec && h.lay.total() >= wh_rec + per * 8u && h.lay.total() != 0,
                      "ether tx host shape %d", shape);
                const size_t fl_at[4] = {7680, 8192, 7936, 7936}, len_at[4] = {7680, 7936, 7680, 7936};   // by shape
                const size_t f = fl_at[shape];
                expect(d, {0, 7680, len_at[shape], f, f + 256, f + 512, f + 768}, f + 1024, f + 1024, "ether tx");
                const size_t hlen_at[4] = {0, 256, 0, 256}, hrec_at[4] = {0, 512, 256, 256};
                expect(h, {0, hlen_at[shape], hrec_at[shape]}, hrec_at[shape] + 256, hrec_at[shape] + 40, "ether tx host");
                check_regions(d, "ether tx");
                check_regions(h, "ether tx host");
            }
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- records
// Four items of 200 distinct octets each in a buffer of 1000 (item i at 40 + 230 i in the strided form; in
// the offset form at 710, 20, 480, 250, out of order, with lengths 180, 200, 190, 170).
static const uint64_t kOff[4] = {710, 20, 480, 250};
static const uint16_t kLen[4] = {180, 200, 190, 170};

static std::vector<uint8_t> fresh() {
    std::vector<uint8_t> b(1000);
    for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)(i * 7u + (i >> 8) * 13u + 1u);
    return b;
}

// `want`: the original with 2 octets put at each (position, value) — the value's octets as memcpy stores them.
static void put16(std::vector<uint8_t>& b, uint64_t at, uint16_t v) { memcpy(&b[at], &v, 2); }

static void expect_equal(const std::vector<uint8_t>& got, const std::vector<uint8_t>& want, const char* what) {
    for (size_t i = 0; i < got.size(); ++i) CHECK(got[i] == want[i], "%s: octet %zu is %02x, want %02x", what, i, got[i], want[i]);
}

static int test_records() {
    const uint32_t l4_at[4] = {0, 0, 36, 60};                   // the transport field's place in items 2 and 3
    for (int offs = 0; offs < 2; ++offs) {
        const uint64_t* off = offs ? kOff : nullptr;
        const uint16_t* len = offs ? kLen : nullptr;
        const uint64_t stride = offs ? 0 : 230, base_at = offs ? 0 : 40;
        auto start = [&](uint32_t i) { return base_at + (offs ? kOff[i] : (uint64_t)i * stride); };
        for (uint32_t hdr : {0u, (uint32_t)NETCSUM_L2_HDR_ETHER}) {
            const std::string tag = std::string(offs ? "offsets" : "strided") + (hdr ? " +14" : " +0");
            // in place: store masks none, IP only, L4 only, both; then the same with item 1 flagged EXT_HDR
            for (int ext = 0; ext < 2; ++ext) {
                uint64_t rec[4];
                const uint8_t flags[4] = {0x00, (uint8_t)(ext ? (NETCSUM_PKT_EXT_HDR | 0x02) : 0x04), 0x11, 0x03};
                for (uint32_t i = 0; i < 4; ++i) {
                    const uint64_t vals = (0xA1B2u + i) | ((uint64_t)(0xC3D4u + i) << 16);
                    rec[i] = vals | ((uint64_t)l4_at[i] << 32) | ((uint64_t)flags[i] << 48) | ((uint64_t)i << 56);   // store = i
                }
                std::vector<uint8_t> got = fresh(), want = fresh();
                uint8_t fl[4] = {0xEE, 0xEE, 0xEE, 0xEE};
                const TxSkipped skip = apply_tx_records(rec, got.data() + base_at, off, len, stride, 200, hdr, 4, fl);
                if (!ext) put16(want, start(1) + hdr + 10, 0xA1B3);             // item 1: IP only
                put16(want, start(2) + hdr + l4_at[2], 0xC3D6);                  // item 2: L4 only
                put16(want, start(3) + hdr + 10, 0xA1B5);                        // item 3: both
                put16(want, start(3) + hdr + l4_at[3], 0xC3D7);
                expect_equal(got, want, (tag + " in place").c_str());
                for (uint32_t i = 0; i < 4; ++i) {
                    const uint8_t w = (ext && i == 1) ? 0xEE : flags[i];         // (a skipped item's flags: the caller's)
                    CHECK(fl[i] == w, "%s: flags[%u] %02x, want %02x", tag.c_str(), i, fl[i], w);
                }
                if (ext) {
                    CHECK(skip.idx.size() == 1 && skip.off.size() == 1 && skip.len.size() == 1 && skip.idx[0] == 1, "%s: skip list",
                          tag.c_str());
                    CHECK(skip.off[0] == (offs ? kOff[1] : stride) + hdr && skip.len[0] == (offs ? kLen[1] : 200u) - hdr,
                          "%s: skipped at %llu len %u", tag.c_str(), (unsigned long long)skip.off[0], skip.len[0]);
                } else {
                    CHECK(skip.idx.empty() && skip.off.empty() && skip.len.empty(), "%s: nothing skipped", tag.c_str());
                }
                std::vector<uint8_t> got2 = fresh();                             // no flags array
                (void)apply_tx_records(rec, got2.data() + base_at, off, len, stride, 200, hdr, 4, nullptr);
                expect_equal(got2, want, (tag + " in place, no flags").c_str());
            }
            // copy pipeline: the gather's records of items s0 = 1 .. 3 (none, L4 only, both) and of item 0 (IP only)
            {
                uint64_t rec[3];
                const uint32_t pos[3] = {0x0000FFFFu, kRecFieldL4 | l4_at[2], kRecFieldIP | kRecFieldL4 | l4_at[3]};
                for (uint32_t i = 0; i < 3; ++i) rec[i] = (0x1357u + i) | ((uint64_t)(0x2468u + i) << 16) | ((uint64_t)pos[i] << 32);
                const uint64_t rec0 = 0x9999u | (0x7777ull << 16) | ((uint64_t)(kRecFieldIP | 0x50u) << 32);
                std::vector<uint8_t> got = fresh(), want = fresh();
                apply_field_records(got.data() + base_at + hdr, off, stride, 1, 3, rec);
                apply_field_records(got.data() + base_at + hdr, off, stride, 0, 1, &rec0);
                put16(want, start(2) + hdr + l4_at[2], 0x2469);
                put16(want, start(3) + hdr + 10, 0x1359);
                put16(want, start(3) + hdr + l4_at[3], 0x246A);
                put16(want, start(0) + hdr + 10, 0x9999);
                expect_equal(got, want, (tag + " gathered").c_str());
            }
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "plan") test_plan();
    else if (what == "layout") test_layout();
    else if (what == "records") test_records();
    else {
        fprintf(stderr, "usage: %s plan | layout | records\n", argv[0]);
        return 2;
    }
    printf("ok %ld\n", g_checks);
    return 0;
}
