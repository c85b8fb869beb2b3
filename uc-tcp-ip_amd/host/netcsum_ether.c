/*
 * netcsum_ether.c — host side of the Ethernet-frame Rx and Tx bursts (include/netcsum_mi355x.h (2b''''),
 * (2b''''')). Plain C99, host logic only.
 *
 * NetUtil_MI355X_EtherClass applies the layer-2 rules of include/netcsum_ether.h — the ones the demux
 * kernel applies per frame — to one frame in host memory, NetUtil_MI355X_EtherTxClass the Tx rule
 * (NetCsum_L2TxClass, the Tx demux kernel's), and NetUtil_MI355X_RxBurstEtherTally turns a
 * burst's per-frame classes into counts: the INV_* ones are the increments the reference's interface
 * layer would have made (RxInvFrameCtr, RxInvAddrDestCtr, RxInvAddrSrcCtr of
 * Net_ErrCtrs.IFs.IFs_802x, IF/net_if_802x.c:550, :2010, :2022, :2183, :2270-2348).
 */
#include "../../include/netcsum_ether.h"

#include <stddef.h>

uint8_t NetUtil_MI355X_EtherClass(const void *frame, uint16_t len, uint32_t eth_cfg, const uint8_t *hw_addr,
                                  uint16_t *p_hdr_len)
{
    uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t hw_lo = 0u, hw_hi = 0u, cls;

    if (len >= NETCSUM_L2_FRAME_MIN && frame != NULL) {  /* (a runt is classified unread) */
        NetCsum_L2Words((const uint8_t *)frame, w);
    }
    if (hw_addr != NULL) {
        hw_lo = (uint32_t)hw_addr[0] | ((uint32_t)hw_addr[1] << 8) | ((uint32_t)hw_addr[2] << 16) | ((uint32_t)hw_addr[3] << 24);
        hw_hi = (uint32_t)hw_addr[4] | ((uint32_t)hw_addr[5] << 8);
    }
    /* a NULL frame can only be the runt it is classified as */
    cls = NetCsum_L2Class(frame != NULL ? len : 0u, w, eth_cfg, hw_addr != NULL, hw_lo, hw_hi);
    if (p_hdr_len != NULL) {
        *p_hdr_len = (uint16_t)NetCsum_L2HdrLen(cls);
    }
    return (uint8_t)cls;
}

uint8_t NetUtil_MI355X_EtherTxClass(const void *frame, uint16_t len, uint16_t *p_hdr_len)
{
    uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t cls;

    if (len >= NETCSUM_L2_FRAME_MIN && frame != NULL) {  /* (a runt is classified unread) */
        NetCsum_L2Words((const uint8_t *)frame, w);
    }
    cls = NetCsum_L2TxClass(frame != NULL ? len : 0u, w);
    if (p_hdr_len != NULL) {
        *p_hdr_len = (uint16_t)NetCsum_L2HdrLen(cls);
    }
    return (uint8_t)cls;
}

NET_ERR NetUtil_MI355X_RxBurstEtherTally(const uint8_t *h_l2, uint32_t n_frame, uint32_t *ctr)
{
    uint32_t i;

    if (ctr == NULL || (h_l2 == NULL && n_frame != 0u)) {
        return NET_ERR_FAULT_NULL_PTR;
    }
    for (i = 0u; i < n_frame; ++i) {
        if (h_l2[i] >= NETCSUM_L2_NBR_CLASSES) {
            return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
        }
    }
    for (i = 0u; i < n_frame; ++i) {
        ctr[h_l2[i]] += 1u;
    }
    return NET_UTIL_ERR_NONE;
}
