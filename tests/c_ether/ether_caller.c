/*
 * ether_caller.c — plain C99 caller of NetUtil_MI355X_EtherClass / RxBurstEtherTally
 * (include/netcsum_mi355x.h (2b'''')), built by tests/test_ether_cpu.py from host/netcsum_ether.c alone with
 * -fsanitize=address,undefined. Its own main and its own expectations: a dozen frames written out by
 * hand, each in a heap block of exactly the octets received, so that a read past the frame (or any
 * read of a runt) is an AddressSanitizer error.
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

static const uint8_t HW[6] = {0x02, 0x00, 0x5E, 0x10, 0x20, 0x30};

#define DST_HW    0x02, 0x00, 0x5E, 0x10, 0x20, 0x30
#define DST_OTHER 0x02, 0x00, 0x5E, 0x10, 0x20, 0x31
#define DST_BCAST 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF
#define DST_MCAST 0x33, 0x33, 0x00, 0x00, 0x00, 0x01
#define SRC_OK    0x02, 0x11, 0x22, 0x33, 0x44, 0x55
#define SRC_NULL  0x00, 0x00, 0x00, 0x00, 0x00, 0x00
#define LLC_SNAP(t_hi, t_lo) 0xAA, 0xAA, 0x03, 0x00, 0x00, 0x00, t_hi, t_lo

/* head: the first octets of the frame; len: the octets received (the rest zero). */
static uint8_t classify(const uint8_t *head, size_t head_len, uint16_t len, uint32_t eth_cfg, const uint8_t *hw,
                        uint16_t *hdr)
{
    uint8_t *f = (uint8_t *)malloc(len ? len : 1u);
    uint8_t cls;

    if (f == NULL) {
        abort();
    }
    memset(f, 0, len ? len : 1u);
    memcpy(f, head, head_len < len ? head_len : len);
    cls = NetUtil_MI355X_EtherClass(len ? f : NULL, len, eth_cfg, hw, hdr);
    free(f);
    return cls;
}

#define CLASSIFY(arr, len, cfg, hw, hdr) classify(arr, sizeof(arr), (uint16_t)(len), cfg, hw, hdr)

int main(void)
{
    static const uint8_t e2_v4[]    = {DST_HW, SRC_OK, 0x08, 0x00, 0x45, 0x00};
    static const uint8_t e2_v6[]    = {DST_BCAST, SRC_OK, 0x86, 0xDD, 0x60, 0x00};
    static const uint8_t e2_arp[]   = {DST_BCAST, SRC_OK, 0x08, 0x06, 0x00, 0x01};
    static const uint8_t e2_vlan[]  = {DST_HW, SRC_OK, 0x81, 0x00, 0x00, 0x05};
    static const uint8_t e2_1501[]  = {DST_HW, SRC_OK, 0x05, 0xDD, 0xAA, 0xAA, 0x03, 0x00, 0x00, 0x00, 0x08, 0x00};
    static const uint8_t e2_other[] = {DST_OTHER, SRC_OK, 0x08, 0x00, 0x45, 0x00};
    static const uint8_t e2_mcast[] = {DST_MCAST, SRC_OK, 0x86, 0xDD, 0x60, 0x00};
    static const uint8_t e2_src0[]  = {DST_OTHER, SRC_NULL, 0x08, 0x00, 0x45, 0x00};
    static const uint8_t e2_srcff[] = {DST_HW, DST_BCAST, 0x81, 0x00, 0x45, 0x00};
    /* 100 octets received: length field 100 - 18 = 82 = 0x52 */
    static const uint8_t sn_v4[]    = {DST_HW, SRC_OK, 0x00, 0x52, LLC_SNAP(0x08, 0x00), 0x45};
    static const uint8_t sn_v6[]    = {DST_HW, SRC_OK, 0x00, 0x52, LLC_SNAP(0x86, 0xDD), 0x60};
    static const uint8_t sn_arp[]   = {DST_HW, SRC_OK, 0x00, 0x52, LLC_SNAP(0x08, 0x06), 0x00};
    static const uint8_t sn_len[]   = {DST_HW, SRC_OK, 0x00, 0x53, LLC_SNAP(0x08, 0x00), 0x45};
    static const uint8_t sn_dsap[]  = {DST_HW, SRC_OK, 0x00, 0x52, 0xAB, 0xAA, 0x03, 0x00, 0x00, 0x00, 0x08, 0x00};
    static const uint8_t sn_ssap[]  = {DST_HW, SRC_OK, 0x00, 0x52, 0xAA, 0xAB, 0x03, 0x00, 0x00, 0x00, 0x08, 0x00};
    static const uint8_t sn_ctrl[]  = {DST_HW, SRC_OK, 0x00, 0x52, 0xAA, 0xAA, 0x13, 0x00, 0x00, 0x00, 0x08, 0x00};
    static const uint8_t sn_code[]  = {DST_HW, SRC_OK, 0x00, 0x52, 0xAA, 0xAA, 0x03, 0x00, 0x00, 0x01, 0x08, 0x00};
    static const uint8_t sn_type[]  = {DST_HW, SRC_OK, 0x00, 0x52, LLC_SNAP(0x80, 0x35)};
    static const uint8_t sn_1500[]  = {DST_HW, SRC_OK, 0x05, 0xDC, LLC_SNAP(0x08, 0x00), 0x45};
    uint16_t hdr = 0xFFFFu;
    uint32_t ctr[NETCSUM_L2_NBR_CLASSES];
    uint8_t l2[6];
    uint32_t k;

    /* Ethernet II */
    EXPECT(CLASSIFY(e2_v4, 60, 0u, HW, &hdr) == NETCSUM_L2_ETHER_IPV4 && hdr == 14u);
    EXPECT(CLASSIFY(e2_v4, 1514, 0u, HW, NULL) == NETCSUM_L2_ETHER_IPV4);
    EXPECT(CLASSIFY(e2_v6, 60, 0u, HW, &hdr) == NETCSUM_L2_ETHER_IPV6 && hdr == 14u);
    EXPECT(CLASSIFY(e2_arp, 60, 0u, HW, &hdr) == NETCSUM_L2_ETHER_ARP && hdr == 14u);
    EXPECT(CLASSIFY(e2_vlan, 64, 0u, HW, &hdr) == NETCSUM_L2_INV_ETHER_TYPE && hdr == 0u);
    EXPECT(CLASSIFY(e2_1501, 64, 0u, HW, &hdr) == NETCSUM_L2_INV_ETHER_TYPE && hdr == 0u);
    /* runts: classified from the length, never read */
    hdr = 0xFFFFu;
    EXPECT(CLASSIFY(e2_v4, 59, 0u, HW, &hdr) == NETCSUM_L2_INV_FRAME_SIZE && hdr == 0u);
    EXPECT(CLASSIFY(e2_v4, 14, 0u, NULL, NULL) == NETCSUM_L2_INV_FRAME_SIZE);
    EXPECT(CLASSIFY(e2_v4, 0, 0u, HW, NULL) == NETCSUM_L2_INV_FRAME_SIZE);
    /* addresses */
    EXPECT(CLASSIFY(e2_other, 60, 0u, HW, &hdr) == NETCSUM_L2_INV_ADDR_DEST && hdr == 0u);
    EXPECT(CLASSIFY(e2_other, 60, 0u, NULL, &hdr) == NETCSUM_L2_ETHER_IPV4 && hdr == 14u);       /* promiscuous */
    EXPECT(CLASSIFY(e2_mcast, 60, 0u, HW, NULL) == NETCSUM_L2_INV_ADDR_DEST);
    EXPECT(CLASSIFY(e2_mcast, 60, NETCSUM_ETHCFG_MCAST_RX, HW, NULL) == NETCSUM_L2_ETHER_IPV6);
    EXPECT(CLASSIFY(e2_mcast, 60, 0u, NULL, NULL) == NETCSUM_L2_ETHER_IPV6);
    EXPECT(CLASSIFY(e2_src0, 60, 0u, HW, NULL) == NETCSUM_L2_INV_ADDR_DEST);                     /* earlier check wins */
    EXPECT(CLASSIFY(e2_src0, 60, 0u, NULL, NULL) == NETCSUM_L2_INV_ADDR_SRC);
    EXPECT(CLASSIFY(e2_srcff, 60, 0u, HW, NULL) == NETCSUM_L2_INV_ADDR_SRC);                     /* ... before the type */
    /* IEEE 802.3 + LLC/SNAP */
    EXPECT(CLASSIFY(sn_v4, 100, 0u, HW, &hdr) == NETCSUM_L2_SNAP_IPV4 && hdr == 22u);
    EXPECT(CLASSIFY(sn_v6, 100, 0u, HW, &hdr) == NETCSUM_L2_SNAP_IPV6 && hdr == 22u);
    EXPECT(CLASSIFY(sn_arp, 100, 0u, HW, &hdr) == NETCSUM_L2_SNAP_ARP && hdr == 22u);
    EXPECT(CLASSIFY(sn_v4, 101, 0u, HW, &hdr) == NETCSUM_L2_INV_LEN_FRAME && hdr == 0u);
    EXPECT(CLASSIFY(sn_len, 100, 0u, HW, NULL) == NETCSUM_L2_INV_LEN_FRAME);
    EXPECT(CLASSIFY(sn_len, 64, 0u, HW, NULL) == NETCSUM_L2_INV_LEN_FRAME);
    EXPECT(CLASSIFY(sn_len, 63, 0u, HW, NULL) == NETCSUM_L2_SNAP_IPV4);                          /* 60-63: no length check */
    EXPECT(CLASSIFY(sn_len, 60, 0u, HW, NULL) == NETCSUM_L2_SNAP_IPV4);
    EXPECT(CLASSIFY(sn_dsap, 100, 0u, HW, NULL) == NETCSUM_L2_INV_LLC_DSAP);
    EXPECT(CLASSIFY(sn_dsap, 99, 0u, HW, NULL) == NETCSUM_L2_INV_LEN_FRAME);                     /* the length comes first */
    EXPECT(CLASSIFY(sn_ssap, 100, 0u, HW, NULL) == NETCSUM_L2_INV_LLC_SSAP);
    EXPECT(CLASSIFY(sn_ctrl, 100, 0u, HW, NULL) == NETCSUM_L2_INV_LLC_CTRL);
    EXPECT(CLASSIFY(sn_code, 100, 0u, HW, NULL) == NETCSUM_L2_INV_SNAP_CODE);
    EXPECT(CLASSIFY(sn_type, 100, 0u, HW, NULL) == NETCSUM_L2_INV_SNAP_TYPE);
    EXPECT(CLASSIFY(sn_1500, 1518, 0u, HW, &hdr) == NETCSUM_L2_SNAP_IPV4 && hdr == 22u);         /* 1500: still a length */

    /* tally */
    memset(ctr, 0, sizeof ctr);
    l2[0] = NETCSUM_L2_ETHER_IPV4;
    l2[1] = NETCSUM_L2_INV_SNAP_TYPE;
    l2[2] = NETCSUM_L2_ETHER_IPV4;
    l2[3] = NETCSUM_L2_INV_ADDR_SRC;
    l2[4] = NETCSUM_L2_SNAP_IPV6;
    l2[5] = NETCSUM_L2_NBR_CLASSES;
    EXPECT(NetUtil_MI355X_RxBurstEtherTally(l2, 5u, ctr) == NET_UTIL_ERR_NONE);
    EXPECT(ctr[NETCSUM_L2_ETHER_IPV4] == 2u && ctr[NETCSUM_L2_INV_SNAP_TYPE] == 1u && ctr[NETCSUM_L2_INV_ADDR_SRC] == 1u &&
           ctr[NETCSUM_L2_SNAP_IPV6] == 1u);
    EXPECT(NetUtil_MI355X_RxBurstEtherTally(l2, 6u, ctr) == NET_UTIL_ERR_MI355X_INVALID_ARG);    /* nothing counted */
    for (k = 0u, hdr = 0u; k < NETCSUM_L2_NBR_CLASSES; ++k) {
        hdr = (uint16_t)(hdr + ctr[k]);
    }
    EXPECT(hdr == 5u);
    EXPECT(NetUtil_MI355X_RxBurstEtherTally(NULL, 1u, ctr) == NET_ERR_FAULT_NULL_PTR);
    EXPECT(NetUtil_MI355X_RxBurstEtherTally(l2, 1u, NULL) == NET_ERR_FAULT_NULL_PTR);
    EXPECT(NetUtil_MI355X_RxBurstEtherTally(NULL, 0u, ctr) == NET_UTIL_ERR_NONE);

    if (failures != 0) {
        fprintf(stderr, "ether_caller: %d failures\n", failures);
        return 1;
    }
    printf("ether_caller ok\n");
    return 0;
}
