/* What the reference's IF/net_if_802x.c links against besides itself, and one entry point that hands
 * NetIF_802x_Rx a single received frame and reports what it did (oracle/Makefile `ref`;
 * tests/golden/make_ether_vectors.py records from it). Our own text: the reference's sources are only
 * named on the compiler line, and its headers are only included.
 *
 * The layers above the interface are recording stubs: NetARP_Rx, NetIPv4_Rx and NetIPv6_Rx note that
 * they ran and the buffer fields the 802.x layer set for them, and return their layer's *_ERR_NONE.
 * They are the seam where the real functions go once their stand-ins exist.
 *
 * NetIF_802x_Rx ends every rejected frame in its discard routine, which frees the buffer and then
 * stores NET_ERR_RX: the NET_IF_ERR_INVALID_* code that names the failed check is in *p_err only until
 * then. NetBuf_FreeBuf here therefore records *p_err as it stands when the buffer is discarded. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "net_if_802x.h"
#include "net_buf.h"
#include "net_ctr.h"
#include "net_err.h"

/* ---------------------------------------------------------------------------- the missing externals */
NET_CTR_STATS Net_StatCtrs;
NET_CTR_ERRS  Net_ErrCtrs;

void Mem_Clr(void *pmem, CPU_SIZE_T size) { memset(pmem, 0, size); }

void Mem_Copy(void *pdest, const void *psrc, CPU_SIZE_T size) { memcpy(pdest, psrc, size); }

CPU_BOOLEAN Mem_Cmp(const void *p1_mem, const void *p2_mem, CPU_SIZE_T size) {
    return memcmp(p1_mem, p2_mem, size) == 0 ? DEF_YES : DEF_NO;
}

void NetCtr_Inc(NET_CTR *pctr) { ++*pctr; }

#define STUB_ARP  1u
#define STUB_IPV4 2u
#define STUB_IPV6 3u

typedef struct {
    int32_t  err;               /* *p_err when NetIF_802x_Rx returned                                    */
    int32_t  err_discard;       /* *p_err when the buffer was discarded (the start value if it was not)  */
    uint32_t discards;          /* NetBuf_FreeBuf calls                                                  */
    uint32_t stub;              /* STUB_*: the upper layer that was called (the last one)                */
    uint32_t stub_calls;
    uint32_t ix;                /* ARP_MsgIx (ARP) / IP_HdrIx, as the stub saw it                        */
    uint32_t if_hdr_len;        /* IF_HdrLen, DataLen, Flags: as the stub saw them, else on return       */
    uint32_t data_len;
    uint32_t flags;
    uint32_t ctr[8];            /* the interface's NET_CTR_IF_802x_ERRS, Ref802x_CtrNames() order         */
    uint32_t ctr_global[8];     /* deltas of Net_ErrCtrs.IFs.IFs_802x, same order                        */
    uint32_t ctr_err_other;     /* increments of Net_ErrCtrs outside IFs.IFs_802x                        */
} REF802X_OUT;

static REF802X_OUT *cur;
static NET_ERR     *cur_err;

static void stub_ran(uint32_t which, NET_BUF *p_buf, uint32_t ix) {
    cur->stub = which;
    ++cur->stub_calls;
    cur->ix = ix;
    cur->if_hdr_len = p_buf->Hdr.IF_HdrLen;
    cur->data_len = p_buf->Hdr.DataLen;
    cur->flags = p_buf->Hdr.Flags;
}

void NetARP_Rx(NET_BUF *p_buf, NET_ERR *p_err) {
    stub_ran(STUB_ARP, p_buf, p_buf->Hdr.ARP_MsgIx);
    *p_err = NET_ARP_ERR_NONE;
}

void NetIPv4_Rx(NET_BUF *p_buf, NET_ERR *p_err) {
    stub_ran(STUB_IPV4, p_buf, p_buf->Hdr.IP_HdrIx);
    *p_err = NET_IPv4_ERR_NONE;
}

void NetIPv6_Rx(NET_BUF *p_buf, NET_ERR *p_err) {
    stub_ran(STUB_IPV6, p_buf, p_buf->Hdr.IP_HdrIx);
    *p_err = NET_IPv6_ERR_NONE;
}

void NetARP_CacheHandler(NET_BUF *p_buf, NET_ERR *p_err) {     /* (transmit path only) */
    (void)p_buf;
    *p_err = NET_ARP_ERR_NONE;
}

/* With IPv6 enabled the file's transmit path also names these two; nothing on the receive path calls them. */
void NetNDP_NeighborCacheHandler(const NET_BUF *p_buf, NET_ERR *p_err) {
    (void)p_buf;
    *p_err = NET_ERR_NONE;
}

void NetIPv6_AddrHW_McastSet(CPU_INT08U *p_addr_mac, void *p_addr, NET_ERR *p_err) {
    (void)p_addr_mac;
    (void)p_addr;
    *p_err = NET_ERR_NONE;
}

NET_BUF_QTY NetBuf_FreeBuf(NET_BUF *p_buf, NET_CTR *p_ctr) {
    (void)p_buf;
    (void)p_ctr;
    ++cur->discards;
    cur->err_discard = (int32_t)*cur_err;
    return 1u;
}

/* ------------------------------------------------------------------------------------- entry points */
const char *Ref802x_CtrNames(void) {
    return "NullPtrCtr RxInvFrameCtr RxInvAddrDestCtr RxInvAddrSrcCtr RxInvProtocolCtr RxPktDisCtr TxPktDisCtr TxInvProtocolCtr";
}

static void ctrs_of(const NET_CTR_IF_802x_ERRS *c, uint32_t out[8]) {
    out[0] = c->NullPtrCtr;
    out[1] = c->RxInvFrameCtr;
    out[2] = c->RxInvAddrDestCtr;
    out[3] = c->RxInvAddrSrcCtr;
    out[4] = c->RxInvProtocolCtr;
    out[5] = c->RxPktDisCtr;
    out[6] = c->TxPktDisCtr;
    out[7] = c->TxInvProtocolCtr;
}

/* The error codes a record can hold, as "NAME value" lines: the recorder stores names, not numbers. */
const char *Ref802x_ErrNames(void) {
#define E_(name) #name " %d\n"
    static char text[1024];
    snprintf(text, sizeof text,
             E_(NET_ERR_NONE) E_(NET_ERR_RX) E_(NET_ERR_INVALID_PROTOCOL) E_(NET_IF_ERR_NONE)
             E_(NET_IF_ERR_INVALID_ADDR_DEST) E_(NET_IF_ERR_INVALID_ADDR_SRC) E_(NET_IF_ERR_INVALID_LEN_FRAME)
             E_(NET_IF_ERR_INVALID_ETHER_TYPE) E_(NET_IF_ERR_INVALID_LLC_DSAP) E_(NET_IF_ERR_INVALID_LLC_SSAP)
             E_(NET_IF_ERR_INVALID_LLC_CTRL) E_(NET_IF_ERR_INVALID_SNAP_CODE) E_(NET_IF_ERR_INVALID_SNAP_TYPE),
             (int)NET_ERR_NONE, (int)NET_ERR_RX, (int)NET_ERR_INVALID_PROTOCOL, (int)NET_IF_ERR_NONE,
             (int)NET_IF_ERR_INVALID_ADDR_DEST, (int)NET_IF_ERR_INVALID_ADDR_SRC, (int)NET_IF_ERR_INVALID_LEN_FRAME,
             (int)NET_IF_ERR_INVALID_ETHER_TYPE, (int)NET_IF_ERR_INVALID_LLC_DSAP, (int)NET_IF_ERR_INVALID_LLC_SSAP,
             (int)NET_IF_ERR_INVALID_LLC_CTRL, (int)NET_IF_ERR_INVALID_SNAP_CODE, (int)NET_IF_ERR_INVALID_SNAP_TYPE);
#undef E_
    return text;
}

/* The configuration this library was compiled under, as the stack's own module switches see it. */
uint32_t Ref802x_Cfg(void) {
    uint32_t c = 0u;
#ifdef NET_IPv4_MODULE_EN
    c |= 0x01u;
#endif
#ifdef NET_IPv6_MODULE_EN
    c |= 0x02u;
#endif
#ifdef NET_MCAST_RX_MODULE_EN
    c |= 0x04u;
#endif
#ifdef NET_ARP_MODULE_EN
    c |= 0x08u;
#endif
#if (NET_CTR_CFG_ERR_EN == DEF_ENABLED)
    c |= 0x10u;
#endif
#if (NET_ERR_CFG_ARG_CHK_DBG_EN == DEF_ENABLED)
    c |= 0x20u;
#endif
    return c;
}

/* One frame through NetIF_802x_Rx: `frame` holds at least `received` octets (the buffer's TotLen and
 * DataLen), hw_addr is the interface's address. The interface is an enabled Ethernet interface whose
 * data area starts with that address, as NET_IF_DATA_802x has it. Returns 0. */
int Ref802x_Rx(const uint8_t *frame, uint16_t received, const uint8_t *hw_addr, REF802X_OUT *out) {
    static NET_IF                if_;
    static NET_BUF               buf;
    static uint8_t               if_data[16];
    static NET_CTR_IF_802x_STATS ctrs_stat;
    NET_CTR_IF_802x_ERRS         ctrs_err, before;
    NET_CTR_ERRS                 all_before;
    NET_ERR                      err = NET_ERR_NONE;
    uint32_t                     after[8], k;
    size_t                       i;

    memset(out, 0, sizeof *out);
    memset(&if_, 0, sizeof if_);
    memset(&buf, 0, sizeof buf);
    memset(if_data, 0, sizeof if_data);
    memset(&ctrs_err, 0, sizeof ctrs_err);
    memcpy(if_data, hw_addr, 6u);
    if_.Type    = NET_IF_TYPE_ETHER;
    if_.Nbr     = 1u;
    if_.Init    = DEF_YES;
    if_.En      = DEF_YES;
    if_.IF_Data = if_data;
    buf.DataPtr         = (CPU_INT08U *)(uintptr_t)frame;
    buf.Hdr.TotLen      = received;
    buf.Hdr.DataLen     = received;
    buf.Hdr.IF_HdrIx    = 0u;
    buf.Hdr.IP_HdrIx    = NET_BUF_IX_NONE;
#ifdef NET_ARP_MODULE_EN
    buf.Hdr.ARP_MsgIx   = NET_BUF_IX_NONE;
#endif
    buf.Hdr.ProtocolHdrType = NET_PROTOCOL_TYPE_NONE;

    before     = Net_ErrCtrs.IFs.IFs_802x;
    all_before = Net_ErrCtrs;
    cur        = out;
    cur_err    = &err;
    out->err_discard = (int32_t)err;
    out->ix          = NET_BUF_IX_NONE;

    NetIF_802x_Rx(&if_, &buf, &ctrs_stat, &ctrs_err, &err);

    out->err = (int32_t)err;
    if (out->stub_calls == 0u) {
        out->if_hdr_len = buf.Hdr.IF_HdrLen;
        out->data_len   = buf.Hdr.DataLen;
        out->flags      = buf.Hdr.Flags;
    }
    ctrs_of(&ctrs_err, out->ctr);
    ctrs_of(&Net_ErrCtrs.IFs.IFs_802x, after);
    ctrs_of(&before, out->ctr_global);
    for (k = 0u; k < 8u; ++k) out->ctr_global[k] = after[k] - out->ctr_global[k];
    /* every other error counter: compare the rest of Net_ErrCtrs word by word */
    Net_ErrCtrs.IFs.IFs_802x = before;
    for (i = 0u; i < sizeof(NET_CTR_ERRS) / sizeof(NET_CTR); ++i) {
        out->ctr_err_other += ((const NET_CTR *)&Net_ErrCtrs)[i] - ((const NET_CTR *)&all_before)[i];
    }
    Net_ErrCtrs = all_before;
    cur     = 0;
    cur_err = 0;
    return 0;
}
