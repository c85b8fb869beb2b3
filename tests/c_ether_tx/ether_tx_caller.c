/*
 * ether_tx_caller.c — plain C99 caller of NetUtil_MI355X_EtherTxClass (include/netcsum_mi355x.h (2b''''')),
 * built by tests/test_ether_tx_cpu.py from host/netcsum_ether.c alone with -fsanitize=address,undefined.
 * Its own main and its own expectations: frames written out by hand, each in a heap block of exactly its
 * octets, so that a read past the frame (or any read of a runt) is an AddressSanitizer error.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "netcsum_mi355x.h"

static int failures;

#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

#define DST_NEXT  0x02, 0xC0, 0xFF, 0xEE, 0x00, 0x01
#define DST_BCAST 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF
#define DST_MCAST 0x33, 0x33, 0x00, 0x00, 0x00, 0x01
#define SRC_OWN   0x02, 0x11, 0x22, 0x33, 0x44, 0x55
#define SRC_NULL  0x00, 0x00, 0x00, 0x00, 0x00, 0x00

/* head: the first octets of the frame; len: the frame's octets (the rest zero, as the padding is). */
static uint8_t classify(const uint8_t *head, size_t head_len, uint16_t len, uint16_t *hdr)
{
    uint8_t *f = (uint8_t *)malloc(len ? len : 1u);
    uint8_t cls;

    if (f == NULL) {
        abort();
    }
    memset(f, 0, len ? len : 1u);
    memcpy(f, head, head_len < len ? head_len : len);
    cls = NetUtil_MI355X_EtherTxClass(len ? f : NULL, len, hdr);
    free(f);
    return cls;
}

#define CLASSIFY(arr, len, hdr) classify(arr, sizeof(arr), (uint16_t)(len), hdr)

int main(void)
{
    static const uint8_t v4[]       = {DST_NEXT, SRC_OWN, 0x08, 0x00, 0x45, 0x00};
    static const uint8_t v6[]       = {DST_MCAST, SRC_OWN, 0x86, 0xDD, 0x60, 0x00};
    static const uint8_t arp[]      = {DST_BCAST, SRC_OWN, 0x08, 0x06, 0x00, 0x01};
    static const uint8_t vlan[]     = {DST_NEXT, SRC_OWN, 0x81, 0x00, 0x00, 0x05};
    static const uint8_t t1501[]    = {DST_NEXT, SRC_OWN, 0x05, 0xDD, 0x45, 0x00};
    static const uint8_t snap_v4[]  = {DST_NEXT, SRC_OWN, 0x00, 0x2E, 0xAA, 0xAA, 0x03, 0x00, 0x00, 0x00, 0x08, 0x00, 0x45};
    static const uint8_t len_1500[] = {DST_NEXT, SRC_OWN, 0x05, 0xDC, 0xAA, 0xAA, 0x03, 0x00, 0x00, 0x00, 0x08, 0x00, 0x45};
    static const uint8_t src_null[] = {DST_NEXT, SRC_NULL, 0x08, 0x00, 0x45, 0x00};
    static const uint8_t src_bc[]   = {DST_NEXT, DST_BCAST, 0x86, 0xDD, 0x60, 0x00};
    static const uint8_t v4_nib6[]  = {DST_NEXT, SRC_OWN, 0x08, 0x00, 0x60, 0x00};
    uint16_t hdr = 0xFFFFu;
    uint8_t one = 0x08;
    uint32_t ctr[NETCSUM_L2_NBR_CLASSES];
    uint8_t l2[4];

    /* the three types the reference transmits, at the minimum and the maximum frame */
    EXPECT(CLASSIFY(v4, 60, &hdr) == NETCSUM_L2_ETHER_IPV4 && hdr == 14u);
    EXPECT(CLASSIFY(v4, 1514, &hdr) == NETCSUM_L2_ETHER_IPV4 && hdr == 14u);
    EXPECT(CLASSIFY(v6, 74, &hdr) == NETCSUM_L2_ETHER_IPV6 && hdr == 14u);
    EXPECT(CLASSIFY(arp, 60, &hdr) == NETCSUM_L2_ETHER_ARP && hdr == 14u);
    EXPECT(CLASSIFY(arp, 60, NULL) == NETCSUM_L2_ETHER_ARP);           /* the header length is optional */
    /* any other type, the 802.3 length form included: never built by the Tx path */
    EXPECT(CLASSIFY(vlan, 64, &hdr) == NETCSUM_L2_INV_ETHER_TYPE && hdr == 0u);
    EXPECT(CLASSIFY(t1501, 64, &hdr) == NETCSUM_L2_INV_ETHER_TYPE && hdr == 0u);
    EXPECT(CLASSIFY(snap_v4, 64, &hdr) == NETCSUM_L2_INV_ETHER_TYPE && hdr == 0u);
    EXPECT(CLASSIFY(snap_v4, 60, &hdr) == NETCSUM_L2_INV_ETHER_TYPE && hdr == 0u);
    EXPECT(CLASSIFY(len_1500, 1518, &hdr) == NETCSUM_L2_INV_ETHER_TYPE && hdr == 0u);
    /* no address checks */
    EXPECT(CLASSIFY(src_null, 60, &hdr) == NETCSUM_L2_ETHER_IPV4 && hdr == 14u);
    EXPECT(CLASSIFY(src_bc, 80, &hdr) == NETCSUM_L2_ETHER_IPV6 && hdr == 14u);
    /* the class is the type's; the version nibble only decides what the checksum pass is given */
    EXPECT(CLASSIFY(v4_nib6, 60, &hdr) == NETCSUM_L2_ETHER_IPV4 && hdr == 14u);
    /* the length rule comes first and reads nothing: 59 octets, a 1-octet block called 59, NULL, 0 */
    EXPECT(CLASSIFY(v4, 59, &hdr) == NETCSUM_L2_INV_FRAME_SIZE && hdr == 0u);
    EXPECT(CLASSIFY(v4, 14, &hdr) == NETCSUM_L2_INV_FRAME_SIZE && hdr == 0u);
    EXPECT(CLASSIFY(v4, 0, &hdr) == NETCSUM_L2_INV_FRAME_SIZE && hdr == 0u);
    {
        uint8_t *p = (uint8_t *)malloc(1u);
        if (p == NULL) {
            abort();
        }
        *p = one;
        EXPECT(NetUtil_MI355X_EtherTxClass(p, 59, &hdr) == NETCSUM_L2_INV_FRAME_SIZE && hdr == 0u);
        free(p);
    }
    EXPECT(NetUtil_MI355X_EtherTxClass(NULL, 1514, &hdr) == NETCSUM_L2_INV_FRAME_SIZE && hdr == 0u);
    /* the Rx tally counts a Tx burst's classes too */
    memset(ctr, 0, sizeof ctr);
    l2[0] = NETCSUM_L2_ETHER_IPV4;
    l2[1] = NETCSUM_L2_ETHER_ARP;
    l2[2] = NETCSUM_L2_ETHER_IPV4;
    l2[3] = NETCSUM_L2_INV_ETHER_TYPE;
    EXPECT(NetUtil_MI355X_RxBurstEtherTally(l2, 4u, ctr) == NET_UTIL_ERR_NONE);
    EXPECT(ctr[NETCSUM_L2_ETHER_IPV4] == 2u && ctr[NETCSUM_L2_ETHER_ARP] == 1u && ctr[NETCSUM_L2_INV_ETHER_TYPE] == 1u);

    if (failures != 0) {
        fprintf(stderr, "ether_tx_caller: %d failure(s)\n", failures);
        return 1;
    }
    printf("ether_tx_caller ok\n");
    return 0;
}
