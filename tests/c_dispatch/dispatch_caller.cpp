// Stand-alone check of uc-tcp-ip_amd/csrc/netcsum_dispatch.h and netcsum_tables.h as plain C++17
// (nothing from HIP). The callables return the constants they were handed, packed into one number;
// every run-time value of a range is tried and the set that matched is compared with the expected
// set, written out here as literals. Usage: dispatch_caller helper|tables ; prints "ok <checks>".
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <tuple>

#include "netcsum_dispatch.h"
#include "netcsum_tables.h"

using namespace netcsum;

static long g_checks = 0;

#define CHECK(c)                                                          \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

using Set3 = std::set<std::tuple<int, int, int>>;
constexpr long kMiss = -7;

static long pack(long a, long b = 0, long c = 0, long d = 0) {
    return ((a * 1000 + b) * 1000 + c) * 1000 + d;
}

// every (a, b, c) of [lo, hi)^3 that the table hands to its callable, which must be (a, b, c) itself
template <typename Table>
static Set3 matched3(Table t, int lo, int hi, int c_lo, int c_hi) {
    Set3 got;
    for (int a = lo; a < hi; ++a) {
        for (int b = lo; b < hi; ++b) {
            for (int c = c_lo; c < c_hi; ++c) {
                const long r = dsp::pick_tuple(t, kMiss, [](auto x, auto y, auto z) { return pack(x, y, z); }, a, b, c);
                CHECK(r == kMiss || r == pack(a, b, c));
                if (r != kMiss) got.insert({a, b, c});
            }
        }
    }
    return got;
}

template <typename Axis>
static std::set<int> matched1(int lo, int hi) {
    std::set<int> got;
    for (int v = lo; v < hi; ++v) {
        const long r = dsp::pick(kMiss, [](auto x) { return (long)x; }, Axis{v});
        CHECK(r == kMiss || r == v);
        if (r != kMiss) got.insert(v);
    }
    return got;
}

static void helper() {
    // Of: each listed value selects itself and only itself; any other reports no match
    CHECK((matched1<dsp::Of<4, 6, 8>>(-70, 70) == std::set<int>{4, 6, 8}));
    CHECK((matched1<dsp::Of<7>>(-70, 70) == std::set<int>{7}));
    // Or: each listed value selects itself, every other the fallback, never the miss value
    for (int v = -70; v < 70; ++v) {
        const long r = dsp::pick(kMiss, [](auto x) { return (long)x; }, dsp::Or<64, 1, 4, 8, 16, 32>{v});
        CHECK(r == ((v == 1 || v == 4 || v == 8 || v == 16 || v == 32) ? v : 64));
        const long w = dsp::pick(kMiss, [](auto x) { return (long)x; }, dsp::Or<1, 0, 2>{v});
        CHECK(w == ((v == 0 || v == 2) ? v : 1));
    }
    // Flag: bool constants
    CHECK(dsp::pick(kMiss, [](auto b) { return (long)std::is_same<typename decltype(b)::value_type, bool>::value; },
                    dsp::Flag{true}) == 1);
    CHECK(dsp::pick(kMiss, [](auto b) { return b ? 5L : 6L; }, dsp::Flag{false}) == 6);
    CHECK(dsp::pick(kMiss, [](auto b) { return b ? 5L : 6L; }, dsp::Flag{true}) == 5);
    // several axes: every constant arrives, in the order given; one unlisted Of value misses the whole pick
    for (int g = 0; g < 70; ++g) {
        for (int k = 0; k < 10; ++k) {
            for (int vl = 0; vl < 2; ++vl) {
                for (int d = 3; d < 10; ++d) {
                    const long r = dsp::pick(kMiss, [](auto a, auto b, auto c, auto e) { return pack(a, b, c, e); },
                                             dsp::Or<64, 1, 4, 8, 16, 32>{g}, dsp::Or<4, 1, 2, 3>{k}, dsp::Flag{vl != 0},
                                             dsp::Of<4, 6, 8>{d});
                    const int eg = (g == 1 || g == 4 || g == 8 || g == 16 || g == 32) ? g : 64;
                    const int ek = (k >= 1 && k <= 3) ? k : 4;
                    CHECK(r == ((d == 4 || d == 6 || d == 8) ? pack(eg, ek, vl, d) : kMiss));
                }
            }
        }
    }
    // no axis at all: the callable itself
    CHECK(dsp::pick(kMiss, [] { return 3L; }) == 3);
    // the callable runs exactly once
    int calls = 0;
    dsp::pick(0, [&](auto, auto) { return ++calls; }, dsp::Or<2, 2, 3>{2}, dsp::Of<1, 1>{1});
    CHECK(calls == 1);
    // tuples: each listed tuple selects itself and only itself; no per-axis matching
    using Tb = dsp::Table<dsp::Tup<1, 2, 3>, dsp::Tup<3, 2, 1>, dsp::Tup<2, 2, 2>>;
    CHECK((matched3(Tb{}, -2, 6, -2, 6) == Set3{{1, 2, 3}, {3, 2, 1}, {2, 2, 2}}));
    calls = 0;
    dsp::pick_tuple(dsp::Table<dsp::Tup<1, true>, dsp::Tup<1, true>>{}, 0, [&](auto, auto) { return ++calls; }, 1, true);
    CHECK(calls == 1);
    // mixed value types: unsigned run-time values against int constants, a bool member
    CHECK(dsp::pick_tuple(dsp::Table<dsp::Tup<5, false>, dsp::Tup<5, true>>{}, kMiss,
                          [](auto a, auto b) { return pack(a, b ? 1 : 0); }, 5u, true) == pack(5, 1));
    CHECK(dsp::pick_tuple(dsp::Table<dsp::Tup<5, false>>{}, kMiss, [](auto a, auto b) { return pack(a, b ? 1 : 0); }, 5u,
                          true) == kMiss);
}

static void tables() {
    // seg_tile_kernel (G, P, K)
    CHECK((matched3(TileTable{}, 0, 70, 0, 10) ==
           Set3{{1, 2, 3}, {1, 4, 6}, {4, 1, 1}, {4, 2, 2}, {8, 2, 2}, {8, 4, 4}, {16, 4, 4}, {16, 6, 6}, {16, 8, 8},
                {32, 2, 2}, {32, 4, 3}, {32, 4, 4}, {32, 8, 8}, {64, 2, 2}, {64, 4, 4}, {64, 8, 8}}));
    // seg_hdr_kernel (P, S, H)
    CHECK((matched3(HdrTable{}, 0, 9, 0, 9) ==
           Set3{{1, 2, 1}, {1, 3, 1}, {1, 4, 1}, {2, 2, 1}, {2, 3, 1}, {2, 4, 1}, {3, 2, 1}, {3, 3, 1}, {3, 4, 1},
                {4, 2, 1}, {4, 3, 1}, {4, 4, 1}, {5, 2, 1}, {5, 3, 1}, {5, 4, 1},
                {1, 2, 2}, {1, 3, 2}, {1, 4, 2}, {2, 2, 2}, {2, 3, 2}, {2, 4, 2}, {3, 2, 2}, {3, 3, 2}, {3, 4, 2},
                {4, 2, 2}, {4, 3, 2}, {4, 4, 2}, {5, 2, 2}, {5, 3, 2}, {5, 4, 2}, {6, 2, 2}, {6, 3, 2}, {6, 4, 2},
                {1, 2, 4}, {1, 3, 4}, {2, 2, 4}, {2, 3, 4}, {3, 2, 4}, {3, 3, 4}, {4, 2, 4}, {4, 3, 4},
                {5, 2, 4}, {5, 3, 4}, {6, 2, 4}, {6, 3, 4}}));
    // the header tile's stages: 3 and 4 as asked, anything else 2; at most 3 with 4 headers per lane
    for (int st = -3; st < 12; ++st) {
        for (int h : {1, 2, 4}) {
            const int want = (st == 3) ? 3 : (st == 4) ? (h == 4 ? 3 : 4) : 2;
            CHECK(hdr_stages(st, h) == want);
        }
    }
    // pkt_stream_kernel (D, BND, VL)
    Set3 got;
    for (int d = 0; d < 12; ++d) {
        for (int b = -1; b < 6; ++b) {
            for (int vl = 0; vl < 2; ++vl) {
                const long r = dsp::pick_tuple(PktStreamTable{}, kMiss,
                                               [](auto x, auto y, auto z) { return pack(x, y, z ? 1 : 0); }, d, b, vl != 0);
                CHECK(r == kMiss || r == pack(d, b, vl));
                if (r != kMiss) got.insert({d, b, vl});
            }
        }
    }
    CHECK((got == Set3{{4, 0, 0}, {4, 1, 0}, {4, 2, 0}, {4, 3, 0}, {8, 0, 0}, {8, 2, 0}, {8, 3, 0}, {4, 1, 1}, {4, 2, 1},
                       {8, 2, 1}}));
    // pkt_batch_kernel (G, K)
    std::set<std::pair<int, int>> gk;
    for (int g = 0; g < 70; ++g) {
        for (int k = 0; k < 10; ++k) {
            const long r = dsp::pick_tuple(PktGroupTable{}, kMiss, [](auto x, auto y) { return pack(x, y); }, g, k);
            CHECK(r == kMiss || r == pack(g, k));
            if (r != kMiss) gk.insert({g, k});
        }
    }
    CHECK((gk == std::set<std::pair<int, int>>{{8, 4}, {8, 8}, {16, 3}, {16, 6}, {32, 3}, {32, 6}, {64, 4}}));
    // the depth lists
    CHECK((matched1<StreamDepth>(-20, 20) == std::set<int>{4, 6, 8}));
    CHECK((matched1<LiveDepth>(-20, 20) == std::set<int>{4, 8}));
    for (int d = -20; d < 20; ++d) {
        CHECK(dsp::pick(kMiss, [](auto x) { return (long)x; }, VarlenDepth{d}) == (d == 8 ? 8 : 4));
    }
}

int main(int argc, char** argv) {
    const char* part = argc > 1 ? argv[1] : "";
    if (part[0] == 'h') {
        helper();
    } else if (part[0] == 't') {
        tables();
    } else {
        fprintf(stderr, "usage: %s helper|tables\n", argv[0]);
        return 2;
    }
    printf("ok %ld\n", g_checks);
    return 0;
}
