/*
 * frag_caller.c — plain C caller of NetUtil_MI355X_FragSumCalc / FragSumVerify (include/netcsum_mi355x.h
 * (2b''')), the way an integration calls them where NetIPv4_RxPktFragReasm returns a completed
 * datagram. Host code only: built from this file and uc-tcp-ip_amd/host/netcsum_fragsum.c, under
 * -fsanitize=address,undefined (tests/test_fragsum_cpu.py). No device, no library.
 *
 * Every expectation is computed here, octet by octet: the datagram's checksum over
 * pseudo-header + payload as one stream of big-endian words (RFC 1071), and each fragment's record
 * as its own padded word sum, folded, in host order. Exit status 0 = every comparison held.
 */
#include <netcsum_mi355x.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;

static unsigned rnd(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 24);
}

static unsigned fold(unsigned long long s)
{
    while (s >> 16) {
        s = (s & 0xFFFFu) + (s >> 16);
    }
    return (unsigned)s;
}

/* folded sum of the big-endian words of p[0, n), an odd last octet padded with zero */
static unsigned be_sum(const unsigned char *p, size_t n, unsigned long long acc)
{
    size_t i;
    for (i = 0; i + 1 < n; i += 2) {
        acc += ((unsigned)p[i] << 8) | p[i + 1];
    }
    if (i < n) {
        acc += (unsigned)p[i] << 8;
    }
    return fold(acc);
}

static unsigned short to_host(unsigned be)       /* a big-endian word's value as a host uint16_t */
{
    unsigned char b[2];
    unsigned short h;
    b[0] = (unsigned char)(be >> 8);
    b[1] = (unsigned char)be;
    memcpy(&h, b, 2);
    return h;
}

static int failures;

#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);      \
            ++failures;                                                  \
        }                                                                \
    } while (0)

/* One datagram of n octets cut into pieces of the given lengths; pseudo-header of ps octets. */
static void one_case(size_t n, const size_t *cut, unsigned n_cut, size_t ps, int corrupt, int zero)
{
    unsigned char *stream = (unsigned char *)malloc(ps + n + 1);
    NETCSUM_FRAG_SUM *rec = (NETCSUM_FRAG_SUM *)malloc((n_cut + 1) * sizeof *rec);
    unsigned char *pseudo = (unsigned char *)malloc(ps + 1);
    size_t i, pos = 0;
    unsigned k, want;
    NET_CHK_SUM got = 0x1234;
    CPU_BOOLEAN ok = 7;

    if (stream == NULL || rec == NULL || pseudo == NULL) {
        abort();
    }
    for (i = 0; i < ps + n; ++i) {
        stream[i] = zero ? 0 : (unsigned char)rnd();
    }
    memcpy(pseudo, stream, ps);
    if (!zero && n >= 19) {                              /* a valid checksum field in one word of the stream */
        const size_t f = ps + 16 + (ps & 1u);
        unsigned c;
        stream[f] = stream[f + 1] = 0;
        c = ~be_sum(stream, ps + n, 0) & 0xFFFFu;
        stream[f] = (unsigned char)(c >> 8);
        stream[f + 1] = (unsigned char)c;
    }
    if (corrupt && n != 0) {
        stream[ps + rnd() % n] ^= (unsigned char)(1u << (rnd() % 8));
    }
    for (k = 0; k < n_cut; ++k) {                        /* what RxBurstSums reports per fragment */
        rec[k].len = (uint16_t)cut[k];
        rec[k].sum = cut[k] ? to_host(be_sum(stream + ps + pos, cut[k], 0)) : 0;
        pos += cut[k];
    }
    EXPECT(pos == n);
    /* the reference's NULL chain never sums an odd pseudo-header's last octet (net_util.c:1591-1611) */
    want = be_sum(stream, (n_cut == 0 && (ps & 1u)) ? ps - 1 : ps + n, 0);
    EXPECT(NetUtil_MI355X_FragSumCalc(rec, n_cut, ps ? pseudo : NULL, (CPU_INT16U)ps, &got) == NET_UTIL_ERR_NONE);
    EXPECT(got == (NET_CHK_SUM)~to_host(want));
    EXPECT(NetUtil_MI355X_FragSumVerify(rec, n_cut, ps ? pseudo : NULL, (CPU_INT16U)ps, &ok) == NET_UTIL_ERR_NONE);
    EXPECT(ok == (want == 0xFFFFu ? DEF_OK : DEF_FAIL));
    if (!zero && !corrupt && n >= 19) {
        EXPECT(ok == DEF_OK);
    }
    free(pseudo);
    free(rec);
    free(stream);
}

int main(void)
{
    static const size_t pseudo_sizes[] = {0, 12, 40, 11};
    size_t cut[64];
    unsigned t, k;
    NETCSUM_FRAG_SUM two[2] = {{1u, 65528u}, {2u, 7u}};
    NET_CHK_SUM c = 0;
    CPU_BOOLEAN ok = 0;

    for (t = 0; t < 400; ++t) {
        /* fragments as the stack accepts them: multiples of 8, then a last piece of any length */
        size_t n = 0;
        unsigned n_cut = 1 + rnd() % 45;
        for (k = 0; k + 1 < n_cut; ++k) {
            cut[k] = 8u * (1 + rnd() % 180);
            n += cut[k];
        }
        cut[n_cut - 1] = 1 + rnd() % 1480;
        n += cut[n_cut - 1];
        if (n > 65515) {
            continue;
        }
        one_case(n, cut, n_cut, pseudo_sizes[t % 4], (int)(t & 1u), 0);
    }
    for (t = 0; t < 200; ++t) {                          /* any lengths: odd and empty middle pieces */
        size_t n = 0;
        unsigned n_cut = 2 + rnd() % 6;
        for (k = 0; k < n_cut; ++k) {
            cut[k] = rnd() % 5 == 0 ? 0 : rnd() % 300;
            n += cut[k];
        }
        one_case(n, cut, n_cut, pseudo_sizes[t % 4], (int)(t % 3u == 0), 0);
    }
    cut[0] = 1480;
    cut[1] = 333;
    one_case(1813, cut, 2, 12, 0, 1);                    /* all zero: 0xFFFF, not 0 */
    one_case(0, cut, 0, 12, 0, 0);                       /* NULL chain */
    one_case(0, cut, 0, 11, 0, 0);
    cut[0] = 65528;
    cut[1] = 7;
    one_case(65535, cut, 2, 12, 0, 0);                   /* the bound, inside */

    two[1].len = 8u;                                     /* 65 536 octets */
    EXPECT(NetUtil_MI355X_FragSumCalc(two, 2, NULL, 0, &c) == NET_UTIL_ERR_MI355X_INVALID_ARG);
    EXPECT(NetUtil_MI355X_FragSumVerify(two, 2, NULL, 0, &ok) == NET_UTIL_ERR_MI355X_INVALID_ARG);
    EXPECT(NetUtil_MI355X_FragSumCalc(NULL, 2, NULL, 0, &c) == NET_ERR_FAULT_NULL_PTR);
    EXPECT(NetUtil_MI355X_FragSumCalc(two, 1, NULL, 0, NULL) == NET_ERR_FAULT_NULL_PTR);
    EXPECT(NetUtil_MI355X_FragSumVerify(two, 1, NULL, 12, &ok) == NET_ERR_FAULT_NULL_PTR);
    EXPECT(NetUtil_MI355X_FragSumVerify(two, 1, NULL, 0, NULL) == NET_ERR_FAULT_NULL_PTR);
    EXPECT(NetUtil_MI355X_FragSumVerify(NULL, 0, NULL, 0, &ok) == NET_UTIL_ERR_NONE && ok == DEF_FAIL);

    if (failures) {
        fprintf(stderr, "frag_caller: %d failures\n", failures);
        return 1;
    }
    printf("frag_caller ok\n");
    return 0;
}
