/* What the reference's IPv4 receive family — IP/IPv4/net_ipv4.c, net_icmpv4.c, net_igmp.c, Source/net_udp.c,
 * net_tcp.c, over the untouched Source/net_util.c — links against besides itself, and one entry point
 * that hands NetIPv4_Rx a single datagram and reports what it did (oracle/Makefile `ref`;
 * tests/golden/make_ip_vectors.py records from it). Our own text: the reference's sources are only named
 * on the compiler line, and its headers are only included.
 *
 * The four checksum functions. The five callers are compiled with -D renames of the four names
 * (NetUtil_16BitOnesCplChkSum{Hdr,Data}{Calc,Verify} -> RefIPv4_{Hdr,Data}{Calc,Verify}), so their calls
 * land in the wrappers here, which note the arguments, forward to the real function in net_util.c (this
 * file and net_util.c are compiled without the renames) and note the result.
 *
 * Everything above the transport layer, below the IP layer and beside them (buffers, timers, pools,
 * connections, sockets, interfaces, the global lock) is a stub. A stub that tells something about the
 * datagram sets its bit in `stubs` (RefIPv4_StubNames()). Transmit paths the reference enters while it
 * receives — the echo reply, a TCP reset, an ICMP error message — end where they ask for a transmit buffer:
 * NetBuf_Get gives none for NET_TRANSACTION_TX. It gives the one receive buffer NetIPv4_RxPktValidateOpt
 * copies a datagram's options to.
 *
 * Every datagram starts from the same state: RefIPv4_Rx runs the modules' own Init functions, configures
 * one host address on interface 1 and joins one multicast group there, each time. The fragment lists are
 * therefore empty; a lone fragment's list is discarded after the call through the timeout function that
 * NetTmr_Get was handed, after the counters were read. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "net.h"
#include "net_buf.h"
#include "net_conn.h"
#include "net_ctr.h"
#include "net_err.h"
#include "net_icmp.h"
#include "net_if.h"
#include "net_sock.h"
#include "net_stat.h"
#include "net_tcp.h"
#include "net_tmr.h"
#include "net_udp.h"
#include "net_util.h"
#include "net_icmpv4.h"
#include "net_igmp.h"
#include "net_ipv4.h"

/* ------------------------------------------------------------------------------------ what is reported */
#define MAX_CALLS   8u
#define MAX_CTRS    128u

#define FN_HDR_CALC     0u
#define FN_HDR_VERIFY   1u
#define FN_DATA_CALC    2u
#define FN_DATA_VERIFY  3u

typedef struct {
    uint32_t fn;                /* FN_*                                                                    */
    uint32_t proto;             /* Data*: the buffer's ProtocolHdrType; Hdr*: 0                            */
    uint32_t len;               /* Hdr*: the octet count; Data*: the buffer's DataLen                      */
    uint32_t off;               /* Hdr*: the header's offset in the datagram; Data*: the buffer's index of */
                                /* that protocol type (TransportHdrIx, ICMP_MsgIx, IGMP_MsgIx)             */
    uint32_t result;            /* Verify: DEF_OK / DEF_FAIL; Calc: the checksum                           */
    uint32_t pseudo_len;
    uint8_t  pseudo[40];
} REFIPV4_CALL;

typedef struct {
    int32_t      err;           /* *p_err when NetIPv4_Rx returned                                         */
    uint32_t     stubs;         /* the stubs that ran, RefIPv4_StubNames() order                           */
    uint32_t     discards;      /* NetBuf_FreeBuf / NetBuf_FreeBufList calls on the received buffer        */
    uint32_t     frag_queued;   /* NetTmr_Get was handed the received buffer: it heads a fragment list     */
    uint32_t     ctr_other;     /* increments of Net_ErrCtrs outside the named fields                      */
    uint32_t     n_calls;       /* checksum calls made (the first MAX_CALLS are kept)                      */
    uint32_t     ctr[MAX_CTRS]; /* deltas of the named Net_ErrCtrs fields, RefIPv4_CtrNames() order        */
    REFIPV4_CALL calls[MAX_CALLS];
} REFIPV4_OUT;

static REFIPV4_OUT *cur;
static NET_BUF     *cur_buf;

enum { S_SOCK_RX, S_CONN_SRCH, S_ECHO_REPLY, S_BUF_GET_MAX_SIZE, S_BUF_GET_TX, S_BUF_GET_RX, S_TMR_GET, S_TMR_FREE,
       S_RAND_SEED, S_IF_TX, S_NBR };

const char *RefIPv4_StubNames(void) {
    return "NetSock_Rx NetConn_Srch NetICMP_RxEchoReply NetBuf_GetMaxSize NetBuf_Get/TX NetBuf_Get/RX NetTmr_Get NetTmr_Free "
           "Math_RandSeed NetIF_Tx";
}

static void ran(int s) {
    if (cur) cur->stubs |= 1u << s;
}

/* ------------------------------------------------------------------------- the error counters, by name */
#define CTRS_(X) \
    X(IPv4, CfgInvAddrHostCtr) X(IPv4, CfgInvGatewayCtr) X(IPv4, CfgInvAddrInUseCtr) X(IPv4, CfgAddrStateCtr) \
    X(IPv4, CfgAddrNotFoundCtr) X(IPv4, CfgAddrTblSizeCtr) X(IPv4, CfgAddrTblEmptyCtr) X(IPv4, CfgAddrTblFullCtr) \
    X(IPv4, RxPktDisCtr) X(IPv4, RxInvVerCtr) X(IPv4, RxInvLenCtr) X(IPv4, RxInvTotLenCtr) X(IPv4, RxInvFlagsCtr) \
    X(IPv4, RxInvFragCtr) X(IPv4, RxInvProtocolCtr) X(IPv4, RxInvChkSumCtr) X(IPv4, RxInvAddrSrcCtr) X(IPv4, RxInvOptsCtr) \
    X(IPv4, RxOptsBufNoneAvailCtr) X(IPv4, RxOptsBufWrCtr) X(IPv4, RxDestCtr) X(IPv4, RxDestBcastCtr) X(IPv4, RxFragSizeCtr) \
    X(IPv4, RxFragDisCtr) X(IPv4, RxFragDgramDisCtr) X(IPv4, RxFragDgramTimeoutCtr) X(IPv4, TxPktDisCtr) \
    X(IPv4, TxInvProtocolCtr) X(IPv4, TxInvOptTypeCtr) X(IPv4, TxInvDestCtr) \
    X(ICMPv4, RxPktDiscardedCtr) X(ICMPv4, RxInvTypeCtr) X(ICMPv4, RxInvCodeCtr) X(ICMPv4, RxInvMsgLenCtr) \
    X(ICMPv4, RxInvPtrCtr) X(ICMPv4, RxInvChkSumCtr) X(ICMPv4, RxBcastCtr) X(ICMPv4, RxMcastCtr) X(ICMPv4, TxInvalidLenCtr) \
    X(ICMPv4, TxHdrTypeCtr) X(ICMPv4, TxHdrCodeCtr) X(ICMPv4, TxPktDiscardedCtr) \
    X(IGMP, NoneAvailCtr) X(IGMP, RxHdrTypeCtr) X(IGMP, RxHdrVerCtr) X(IGMP, RxHdrMsgLenCtr) X(IGMP, RxHdrChkSumCtr) \
    X(IGMP, RxPktInvalidAddrDestCtr) X(IGMP, RxPktDiscardedCtr) X(IGMP, TxInvalidBufIxCtr) X(IGMP, TxPktDiscardedCtr) \
    X(UDP, NullPtrCtr) X(UDP, InvalidFlagsCtr) X(UDP, RxHdrDatagramLenCtr) X(UDP, RxHdrPortSrcCtr) X(UDP, RxHdrPortDestCtr) \
    X(UDP, RxHdrChkSumCtr) X(UDP, RxDestCtr) X(UDP, RxPktDiscardedCtr) X(UDP, TxPktDiscardedCtr) \
    X(TCP, NullPtrCtr) X(TCP, NoneAvailCtr) X(TCP, NotUsedCtr) X(TCP, RxHdrLenCtr) X(TCP, RxHdrSegLenCtr) \
    X(TCP, RxHdrPortSrcCtr) X(TCP, RxHdrPortDestCtr) X(TCP, RxHdrFlagsCtr) X(TCP, RxHdrChkSumCtr) X(TCP, RxHdrOptsCtr) \
    X(TCP, RxDestCtr) X(TCP, RxPktDiscardedCtr) X(TCP, RxPktQ_FullCtr) X(TCP, TxOptTypeCtr) X(TCP, TxPktDiscardedCtr) \
    X(TCP, ConnInvalidCtr) X(TCP, ConnInvalidOpCtr) X(TCP, ConnInvalidStateCtr) X(TCP, ConnCloseCtr)

#define X_NAME(mod, f) #mod "." #f " "
#define X_OFF(mod, f)  offsetof(NET_CTR_ERRS, mod.f),
static const size_t ctr_off[] = { CTRS_(X_OFF) };
#define N_CTRS (sizeof ctr_off / sizeof ctr_off[0])
typedef char ctrs_fit[(N_CTRS <= MAX_CTRS) ? 1 : -1];

const char *RefIPv4_CtrNames(void) { return CTRS_(X_NAME); }

/* The error codes a record can hold, as "NAME value" lines: the recorder stores names, not numbers. */
const char *RefIPv4_ErrNames(void) {
#define E_(name) #name " %d\n"
    static char text[512];
    snprintf(text, sizeof text, E_(NET_IPv4_ERR_NONE) E_(NET_ERR_RX) E_(NET_ERR_RX_DEST) E_(NET_ERR_TX) E_(NET_ERR_INVALID_PROTOCOL),
             (int)NET_IPv4_ERR_NONE, (int)NET_ERR_RX, (int)NET_ERR_RX_DEST, (int)NET_ERR_TX, (int)NET_ERR_INVALID_PROTOCOL);
#undef E_
    return text;
}

/* The protocol types a checksum call record can hold, as "NAME value" lines. */
const char *RefIPv4_ProtoNames(void) {
#define P_(name) #name " %d\n"
    static char text[512];
    snprintf(text, sizeof text, P_(NET_PROTOCOL_TYPE_NONE) P_(NET_PROTOCOL_TYPE_IP_V4) P_(NET_PROTOCOL_TYPE_ICMP_V4)
             P_(NET_PROTOCOL_TYPE_IGMP) P_(NET_PROTOCOL_TYPE_UDP_V4) P_(NET_PROTOCOL_TYPE_TCP_V4),
             (int)NET_PROTOCOL_TYPE_NONE, (int)NET_PROTOCOL_TYPE_IP_V4, (int)NET_PROTOCOL_TYPE_ICMP_V4, (int)NET_PROTOCOL_TYPE_IGMP,
             (int)NET_PROTOCOL_TYPE_UDP_V4, (int)NET_PROTOCOL_TYPE_TCP_V4);
#undef P_
    return text;
}

/* The configuration this library was compiled under, as the stack's own switches see it. */
uint32_t RefIPv4_Cfg(void) {
    uint32_t c = 0u;
#ifdef NET_IPv4_MODULE_EN
    c |= 0x01u;
#endif
#ifdef NET_IPv6_MODULE_EN
    c |= 0x02u;
#endif
#ifdef NET_IGMP_MODULE_EN
    c |= 0x04u;
#endif
#ifdef NET_TCP_MODULE_EN
    c |= 0x08u;
#endif
#if (NET_CTR_CFG_ERR_EN == DEF_ENABLED)
    c |= 0x10u;
#endif
#if (NET_ERR_CFG_ARG_CHK_DBG_EN == DEF_ENABLED)
    c |= 0x20u;
#endif
#if (NET_UDP_CFG_RX_CHK_SUM_DISCARD_EN == DEF_ENABLED)
    c |= 0x40u;
#endif
#if defined(NET_IPV4_CHK_SUM_OFFLOAD_RX) || defined(NET_ICMP_CHK_SUM_OFFLOAD_RX) || defined(NET_UDP_CHK_SUM_OFFLOAD_RX) || \
    defined(NET_TCP_CHK_SUM_OFFLOAD_RX)
    c |= 0x80u;
#endif
    return c;
}

/* ------------------------------------------------------------------- the recording checksum wrappers */
static REFIPV4_CALL *call_new(uint32_t fn) {
    static REFIPV4_CALL spare;
    REFIPV4_CALL       *c = &spare;
    if (cur) {
        if (cur->n_calls < MAX_CALLS) c = &cur->calls[cur->n_calls];
        ++cur->n_calls;
    }
    memset(c, 0, sizeof *c);
    c->fn = fn;
    return c;
}

static void call_hdr(REFIPV4_CALL *c, const void *phdr, CPU_INT16U size) {
    c->len = size;
    c->off = (cur_buf && phdr) ? (uint32_t)((const CPU_INT08U *)phdr - cur_buf->DataPtr) : 0xFFFFFFFFu;
}

static void call_data(REFIPV4_CALL *c, const void *pdata_buf, const void *ppseudo, CPU_INT16U pseudo_size) {
    const NET_BUF *b = (const NET_BUF *)pdata_buf;
    if (b) {
        c->proto = (uint32_t)b->Hdr.ProtocolHdrType;
        c->len   = b->Hdr.DataLen;
        switch (b->Hdr.ProtocolHdrType) {
        case NET_PROTOCOL_TYPE_ICMP_V4: c->off = b->Hdr.ICMP_MsgIx; break;
        case NET_PROTOCOL_TYPE_IGMP:    c->off = b->Hdr.IGMP_MsgIx; break;
        default:                        c->off = b->Hdr.TransportHdrIx; break;
        }
    }
    c->pseudo_len = pseudo_size;
    if (ppseudo) memcpy(c->pseudo, ppseudo, pseudo_size < sizeof c->pseudo ? pseudo_size : sizeof c->pseudo);
}

NET_CHK_SUM RefIPv4_HdrCalc(void *phdr, CPU_INT16U hdr_size, NET_ERR *p_err) {
    REFIPV4_CALL *c = call_new(FN_HDR_CALC);
    call_hdr(c, phdr, hdr_size);
    return (NET_CHK_SUM)(c->result = NetUtil_16BitOnesCplChkSumHdrCalc(phdr, hdr_size, p_err));
}

CPU_BOOLEAN RefIPv4_HdrVerify(void *phdr, CPU_INT16U hdr_size, NET_ERR *p_err) {
    REFIPV4_CALL *c = call_new(FN_HDR_VERIFY);
    call_hdr(c, phdr, hdr_size);
    return (CPU_BOOLEAN)(c->result = NetUtil_16BitOnesCplChkSumHdrVerify(phdr, hdr_size, p_err));
}

NET_CHK_SUM RefIPv4_DataCalc(void *pdata_buf, void *ppseudo_hdr, CPU_INT16U pseudo_hdr_size, NET_ERR *p_err) {
    REFIPV4_CALL *c = call_new(FN_DATA_CALC);
    call_data(c, pdata_buf, ppseudo_hdr, pseudo_hdr_size);
    return (NET_CHK_SUM)(c->result = NetUtil_16BitOnesCplChkSumDataCalc(pdata_buf, ppseudo_hdr, pseudo_hdr_size, p_err));
}

CPU_BOOLEAN RefIPv4_DataVerify(void *pdata_buf, void *ppseudo_hdr, CPU_INT16U pseudo_hdr_size, NET_ERR *p_err) {
    REFIPV4_CALL *c = call_new(FN_DATA_VERIFY);
    call_data(c, pdata_buf, ppseudo_hdr, pseudo_hdr_size);
    return (CPU_BOOLEAN)(c->result = NetUtil_16BitOnesCplChkSumDataVerify(pdata_buf, ppseudo_hdr, pseudo_hdr_size, p_err));
}

/* ---------------------------------------------------------------------------- the missing externals */
NET_CTR_STATS Net_StatCtrs;
NET_CTR_ERRS  Net_ErrCtrs;
CPU_BOOLEAN   Net_InitDone;
NET_CONN      NetConn_Tbl[NET_CONN_NBR_CONN];

RAND_NBR         Math_RandSeedCur = 1u;
KAL_TICK_RATE_HZ KAL_TickRate     = 1000u;

void Math_RandSetSeed(RAND_NBR seed) { Math_RandSeedCur = seed; }

RAND_NBR Math_RandSeed(RAND_NBR seed) {
    ran(S_RAND_SEED);
    return seed * 1103515245u + 12345u;
}

RAND_NBR Math_Rand(void) { return Math_RandSeedCur = Math_RandSeedCur * 1103515245u + 12345u; }

KAL_TICK KAL_TickGet(KAL_ERR *p_err) {
    *p_err = KAL_ERR_NONE;
    return 0u;
}

static int kal_obj;

KAL_SEM_HANDLE KAL_SemCreate(const CPU_CHAR *p_name, void *p_cfg, KAL_ERR *p_err) {
    KAL_SEM_HANDLE h = { &kal_obj };
    (void)p_name, (void)p_cfg;
    *p_err = KAL_ERR_NONE;
    return h;
}

void KAL_SemSet(KAL_SEM_HANDLE h, CPU_INT08U cnt, KAL_ERR *p_err) { (void)h, (void)cnt, *p_err = KAL_ERR_NONE; }
void KAL_SemPend(KAL_SEM_HANDLE h, KAL_OPT opt, CPU_INT32U timeout_ms, KAL_ERR *p_err) { (void)h, (void)opt, (void)timeout_ms, *p_err = KAL_ERR_TIMEOUT; }
void KAL_SemPost(KAL_SEM_HANDLE h, KAL_OPT opt, KAL_ERR *p_err) { (void)h, (void)opt, *p_err = KAL_ERR_NONE; }
void KAL_SemPendAbort(KAL_SEM_HANDLE h, KAL_ERR *p_err) { (void)h, *p_err = KAL_ERR_NONE; }

void Mem_Clr(void *pmem, CPU_SIZE_T size) { memset(pmem, 0, size); }
void Mem_Copy(void *pdest, const void *psrc, CPU_SIZE_T size) { memmove(pdest, psrc, size); }
CPU_BOOLEAN Mem_Cmp(const void *p1_mem, const void *p2_mem, CPU_SIZE_T size) { return memcmp(p1_mem, p2_mem, size) == 0 ? DEF_YES : DEF_NO; }

void NetCtr_Inc(NET_CTR *pctr) { ++*pctr; }

void Net_GlobalLockAcquire(void *p_fcnt, NET_ERR *p_err) { (void)p_fcnt, *p_err = NET_ERR_NONE; }
void Net_GlobalLockRelease(void) {}

/* buffers: none to transmit with, one to copy a datagram's IP options to */
static NET_BUF    opt_buf;
static CPU_INT08U opt_data[256];

NET_BUF *NetBuf_Get(NET_IF_NBR if_nbr, NET_TRANSACTION transaction, NET_BUF_SIZE size, NET_BUF_SIZE ix, NET_BUF_SIZE *p_ix_offset,
                    NET_BUF_FLAGS flags, NET_ERR *p_err) {
    (void)if_nbr, (void)flags;
    if (p_ix_offset) *p_ix_offset = 0u;
    if (transaction != NET_TRANSACTION_RX || (size_t)size + ix > sizeof opt_data) {
        ran(S_BUF_GET_TX);
        *p_err = NET_BUF_ERR_NONE_AVAIL;
        return (NET_BUF *)0;
    }
    ran(S_BUF_GET_RX);
    memset(&opt_buf, 0, sizeof opt_buf);
    *p_err = NET_BUF_ERR_NONE;
    return &opt_buf;
}

CPU_INT08U *NetBuf_GetDataPtr(NET_IF *p_if, NET_TRANSACTION transaction, NET_BUF_SIZE size, NET_BUF_SIZE ix_start,
                              NET_BUF_SIZE *p_ix_offset, NET_BUF_SIZE *p_data_size, NET_BUF_TYPE *p_type, NET_ERR *p_err) {
    (void)p_if, (void)transaction, (void)size, (void)ix_start;
    if (p_ix_offset) *p_ix_offset = 0u;
    if (p_data_size) *p_data_size = sizeof opt_data;
    if (p_type) *p_type = NET_BUF_TYPE_RX_LARGE;
    *p_err = NET_BUF_ERR_NONE;
    return opt_data;
}

NET_BUF_SIZE NetBuf_GetMaxSize(NET_IF_NBR if_nbr, NET_TRANSACTION transaction, NET_BUF *p_buf, NET_BUF_SIZE ix_start) {
    (void)if_nbr, (void)transaction, (void)p_buf, (void)ix_start;
    ran(S_BUF_GET_MAX_SIZE);
    return 1518u;
}

void NetBuf_DataRd(NET_BUF *p_buf, NET_BUF_SIZE ix, NET_BUF_SIZE len, CPU_INT08U *p_dest, NET_ERR *p_err) {
    memcpy(p_dest, &p_buf->DataPtr[ix], len);
    *p_err = NET_BUF_ERR_NONE;
}

void NetBuf_DataWr(NET_BUF *p_buf, NET_BUF_SIZE ix, NET_BUF_SIZE len, CPU_INT08U *p_src, NET_ERR *p_err) {
    memcpy(&p_buf->DataPtr[ix], p_src, len);
    *p_err = NET_BUF_ERR_NONE;
}

static void freed(const NET_BUF *p_buf) {
    if (cur && p_buf == cur_buf) ++cur->discards;
}

void NetBuf_Free(NET_BUF *p_buf) { freed(p_buf); }

NET_BUF_QTY NetBuf_FreeBuf(NET_BUF *p_buf, NET_CTR *p_ctr) {
    freed(p_buf);
    if (p_buf && p_ctr) ++*p_ctr;
    return p_buf ? 1u : 0u;
}

NET_BUF_QTY NetBuf_FreeBufList(NET_BUF *p_buf_list, NET_CTR *p_ctr) { return NetBuf_FreeBuf(p_buf_list, p_ctr); }
NET_BUF_QTY NetBuf_FreeBufQ_PrimList(NET_BUF *p_buf_q, NET_CTR *p_ctr) { return NetBuf_FreeBuf(p_buf_q, p_ctr); }
CPU_BOOLEAN NetBuf_IsUsed(NET_BUF *p_buf) { return p_buf ? DEF_YES : DEF_NO; }

/* timers: a small table; the one handed the received buffer is the fragment list's */
static NET_TMR tmrs[8];
static NET_TMR *frag_tmr;

NET_TMR *NetTmr_Get(CPU_FNCT_PTR fnct, void *obj, NET_TMR_TICK time, NET_ERR *p_err) {
    size_t i;
    ran(S_TMR_GET);
    for (i = 0u; i < sizeof tmrs / sizeof tmrs[0]; ++i) {
        if (tmrs[i].Fnct == (CPU_FNCT_PTR)0) {
            tmrs[i].Fnct = fnct, tmrs[i].Obj = obj, tmrs[i].TmrVal = time;
            if (cur && obj == (void *)cur_buf) {
                cur->frag_queued = 1u;
                frag_tmr = &tmrs[i];
            }
            *p_err = NET_TMR_ERR_NONE;
            return &tmrs[i];
        }
    }
    *p_err = NET_TMR_ERR_NONE_AVAIL;
    return (NET_TMR *)0;
}

void NetTmr_Set(NET_TMR *p_tmr, CPU_FNCT_PTR fnct, NET_TMR_TICK time, NET_ERR *p_err) {
    p_tmr->Fnct = fnct, p_tmr->TmrVal = time;
    *p_err = NET_TMR_ERR_NONE;
}

void NetTmr_Free(NET_TMR *p_tmr) {
    ran(S_TMR_FREE);
    if (p_tmr) {
        if (p_tmr == frag_tmr) frag_tmr = (NET_TMR *)0;
        memset(p_tmr, 0, sizeof *p_tmr);
    }
}

/* pools: statistics nobody reads */
void NetStat_PoolInit(NET_STAT_POOL *p, NET_STAT_POOL_QTY nbr_avail, NET_ERR *p_err) { (void)p, (void)nbr_avail, *p_err = NET_STAT_ERR_NONE; }
void NetStat_PoolClr(NET_STAT_POOL *p, NET_ERR *p_err) { (void)p, *p_err = NET_STAT_ERR_NONE; }
void NetStat_PoolResetUsedMax(NET_STAT_POOL *p, NET_ERR *p_err) { (void)p, *p_err = NET_STAT_ERR_NONE; }
void NetStat_PoolEntryUsedInc(NET_STAT_POOL *p, NET_ERR *p_err) { (void)p, *p_err = NET_STAT_ERR_NONE; }
void NetStat_PoolEntryUsedDec(NET_STAT_POOL *p, NET_ERR *p_err) { (void)p, *p_err = NET_STAT_ERR_NONE; }
void NetStat_PoolEntryLostInc(NET_STAT_POOL *p, NET_ERR *p_err) { (void)p, *p_err = NET_STAT_ERR_NONE; }

/* connections: there are none, so every TCP segment that passes NetTCP_RxPktValidate ends in the search */
NET_CONN_ID NetConn_Srch(NET_CONN_FAMILY family, NET_CONN_PROTOCOL_IX protocol_ix, CPU_INT08U *p_addr_local, CPU_INT08U *p_addr_remote,
                         NET_CONN_ADDR_LEN addr_len, NET_CONN_ID *p_conn_id_transport, NET_CONN_ID *p_conn_id_app, NET_ERR *p_err) {
    (void)family, (void)protocol_ix, (void)p_addr_local, (void)p_addr_remote, (void)addr_len;
    ran(S_CONN_SRCH);
    if (p_conn_id_transport) *p_conn_id_transport = NET_CONN_ID_NONE;
    if (p_conn_id_app) *p_conn_id_app = NET_CONN_ID_NONE;
    *p_err = NET_CONN_ERR_CONN_NONE;
    return NET_CONN_ID_NONE;
}

NET_CONN_ID NetConn_Get(NET_CONN_FAMILY family, NET_CONN_PROTOCOL_IX protocol_ix, NET_ERR *p_err) {
    (void)family, (void)protocol_ix;
    *p_err = NET_CONN_ERR_NONE_AVAIL;
    return NET_CONN_ID_NONE;
}

#define NO_CONN_ (*p_err = NET_CONN_ERR_INVALID_CONN)
void NetConn_AddrLocalGet(NET_CONN_ID id, CPU_INT08U *p_addr, NET_CONN_ADDR_LEN *p_len, NET_ERR *p_err) { (void)id, (void)p_addr, (void)p_len, NO_CONN_; }
void NetConn_AddrLocalSet(NET_CONN_ID id, NET_IF_NBR if_nbr, CPU_INT08U *p_addr, NET_CONN_ADDR_LEN len, CPU_BOOLEAN over_wr, NET_ERR *p_err) { (void)id, (void)if_nbr, (void)p_addr, (void)len, (void)over_wr, NO_CONN_; }
void NetConn_AddrRemoteGet(NET_CONN_ID id, CPU_INT08U *p_addr, NET_CONN_ADDR_LEN *p_len, NET_ERR *p_err) { (void)id, (void)p_addr, (void)p_len, NO_CONN_; }
void NetConn_AddrRemoteSet(NET_CONN_ID id, CPU_INT08U *p_addr, NET_CONN_ADDR_LEN len, CPU_BOOLEAN over_wr, NET_ERR *p_err) { (void)id, (void)p_addr, (void)len, (void)over_wr, NO_CONN_; }
void NetConn_CloseAllConnsByAddrHandler(CPU_INT08U *p_addr, NET_CONN_ADDR_LEN len) { (void)p_addr, (void)len; }
void NetConn_CloseFromTransport(NET_CONN_ID id, CPU_BOOLEAN close_conn_app) { (void)id, (void)close_conn_app; }
void NetConn_Copy(NET_CONN_ID dest, NET_CONN_ID src) { (void)dest, (void)src; }
NET_CONN_ID NetConn_ID_AppCloneGet(NET_CONN_ID id, NET_ERR *p_err) { (void)id, NO_CONN_; return NET_CONN_ID_NONE; }
void NetConn_ID_AppCloneSet(NET_CONN_ID id, NET_CONN_ID app, NET_ERR *p_err) { (void)id, (void)app, NO_CONN_; }
NET_CONN_ID NetConn_ID_AppGet(NET_CONN_ID id, NET_ERR *p_err) { (void)id, NO_CONN_; return NET_CONN_ID_NONE; }
void NetConn_ID_TransportSet(NET_CONN_ID id, NET_CONN_ID transport, NET_ERR *p_err) { (void)id, (void)transport, NO_CONN_; }
NET_IF_NBR NetConn_IF_NbrGet(NET_CONN_ID id, NET_ERR *p_err) { (void)id, NO_CONN_; return NET_IF_NBR_NONE; }
void NetConn_IPv4TxParamsGet(NET_CONN_ID id, NET_IPv4_FLAGS *p_flags, NET_IPv4_TOS *p_tos, NET_IPv4_TTL *p_ttl, NET_ERR *p_err) { (void)id, (void)p_flags, (void)p_tos, (void)p_ttl, NO_CONN_; }
void NetConn_ListAdd(NET_CONN_ID id, NET_ERR *p_err) { (void)id, NO_CONN_; }

/* sockets: NetSock_Rx is where a UDP datagram that passed NetUDP_RxPktValidate arrives */
void NetSock_Rx(NET_BUF *pbuf, NET_ERR *p_err) {
    (void)pbuf;
    ran(S_SOCK_RX);
    *p_err = NET_SOCK_ERR_NONE;
}

void NetSock_ConnChildAdd(NET_SOCK_ID s, NET_CONN_ID c, NET_ERR *p_err) { (void)s, (void)c, *p_err = NET_SOCK_ERR_INVALID_SOCK; }
void NetSock_ConnSignalAccept(NET_SOCK_ID s, NET_CONN_ID c, NET_ERR *p_err) { (void)s, (void)c, *p_err = NET_SOCK_ERR_INVALID_SOCK; }
void NetSock_ConnSignalClose(NET_SOCK_ID s, CPU_BOOLEAN data_avail, NET_ERR *p_err) { (void)s, (void)data_avail, *p_err = NET_SOCK_ERR_INVALID_SOCK; }
void NetSock_ConnSignalReq(NET_SOCK_ID s, NET_ERR *p_err) { (void)s, *p_err = NET_SOCK_ERR_INVALID_SOCK; }
NET_SOCK *NetSock_GetObj(NET_SOCK_ID s) { (void)s; return (NET_SOCK *)0; }

/* an echo reply that passed NetICMPv4_RxPktValidate arrives here */
void NetICMP_RxEchoReply(CPU_INT16U id, CPU_INT16U seq, CPU_INT08U *p_data, CPU_INT16U data_len, NET_ERR *p_err) {
    (void)id, (void)seq, (void)p_data, (void)data_len;
    ran(S_ECHO_REPLY);
    *p_err = NET_ICMP_ERR_NONE;
}

/* interfaces: number 1 is a valid, enabled, configured Ethernet interface; nothing can be sent on it */
#define REF_IF_NBR 1u
static NET_IF if_;

static CPU_BOOLEAN if_ok(NET_IF_NBR if_nbr, NET_ERR *p_err) {
    *p_err = (if_nbr == REF_IF_NBR) ? NET_IF_ERR_NONE : NET_IF_ERR_INVALID_IF;
    return (if_nbr == REF_IF_NBR) ? DEF_YES : DEF_NO;
}

CPU_BOOLEAN NetIF_IsValidHandler(NET_IF_NBR if_nbr, NET_ERR *p_err) { return if_ok(if_nbr, p_err); }
CPU_BOOLEAN NetIF_IsValidCfgdHandler(NET_IF_NBR if_nbr, NET_ERR *p_err) { return if_ok(if_nbr, p_err); }
CPU_BOOLEAN NetIF_IsEnHandler(NET_IF_NBR if_nbr, NET_ERR *p_err) { return if_ok(if_nbr, p_err); }
CPU_BOOLEAN NetIF_IsEnCfgdHandler(NET_IF_NBR if_nbr, NET_ERR *p_err) { return if_ok(if_nbr, p_err); }
NET_IF_NBR NetIF_GetDflt(void) { return REF_IF_NBR; }

NET_IF *NetIF_Get(NET_IF_NBR if_nbr, NET_ERR *p_err) { return if_ok(if_nbr, p_err) ? &if_ : (NET_IF *)0; }

NET_MTU NetIF_MTU_GetProtocol(NET_IF_NBR if_nbr, NET_PROTOCOL_TYPE protocol, NET_IF_FLAG opt, NET_ERR *p_err) {
    (void)protocol, (void)opt;
    return if_ok(if_nbr, p_err) ? 1480u : 0u;
}

CPU_INT16U NetIF_GetPayloadTxMax(NET_IF_NBR if_nbr, NET_PROTOCOL_TYPE protocol, NET_ERR *p_err) {
    (void)protocol;
    return if_ok(if_nbr, p_err) ? 1480u : 0u;
}

CPU_INT16U NetIF_GetPktSizeMin(NET_IF_NBR if_nbr, NET_ERR *p_err) { return if_ok(if_nbr, p_err) ? 60u : 0u; }
void NetIF_TxIxDataGet(NET_IF_NBR if_nbr, CPU_INT32U data_size, CPU_INT16U *p_ix, NET_ERR *p_err) { (void)data_size, *p_ix += 14u, (void)if_ok(if_nbr, p_err); }
CPU_BOOLEAN NetIF_RxPktIsAvail(NET_IF_NBR if_nbr, NET_CTR rx_chk_nbr) { (void)if_nbr, (void)rx_chk_nbr; return DEF_NO; }
void NetIF_TxSuspend(NET_IF_NBR if_nbr) { (void)if_nbr; }

void NetIF_Tx(NET_BUF *p_buf_list, NET_ERR *p_err) {
    (void)p_buf_list;
    ran(S_IF_TX);
    *p_err = NET_ERR_TX;
}

void NetIF_AddrMulticastAdd(NET_IF_NBR if_nbr, CPU_INT08U *p_addr, CPU_INT08U len, NET_PROTOCOL_TYPE type, NET_ERR *p_err) { (void)p_addr, (void)len, (void)type, (void)if_ok(if_nbr, p_err); }
void NetIF_AddrMulticastRemove(NET_IF_NBR if_nbr, CPU_INT08U *p_addr, CPU_INT08U len, NET_PROTOCOL_TYPE type, NET_ERR *p_err) { (void)p_addr, (void)len, (void)type, (void)if_ok(if_nbr, p_err); }

/* ------------------------------------------------------------------------------------- entry point */
/* The state every datagram meets. Returns 0, or the step that failed. */
static int start_state(uint32_t host, uint32_t mask, uint32_t group) {
    NET_ERR err;
    memset(&if_, 0, sizeof if_);
    if_.Nbr  = REF_IF_NBR;
    if_.Type = NET_IF_TYPE_ETHER;
    if_.Init = DEF_YES;
    if_.En   = DEF_YES;
    memset(tmrs, 0, sizeof tmrs);
    frag_tmr = (NET_TMR *)0;
    memset(NetConn_Tbl, 0, sizeof NetConn_Tbl);
    Net_InitDone = DEF_YES;
    NetIPv4_Init();
    NetICMPv4_Init(&err);
    if (err != NET_ICMPv4_ERR_NONE) return 1;
    NetIGMP_Init();
    NetUDP_Init();
    NetTCP_Init(&err);
    if (err != NET_TCP_ERR_NONE) return 2;
    if (NetIPv4_CfgAddrAdd(REF_IF_NBR, host, mask, NET_IPv4_ADDR_NONE, &err) != DEF_OK) return 3;
    if (NetIGMP_HostGrpJoinHandler(REF_IF_NBR, group, &err) != DEF_YES) return 4;
    return 0;
}

/* One datagram through NetIPv4_Rx. `dgram` holds `received` octets starting at the IP header; they are
 * copied behind a 14-octet interface header into a buffer set up as NetIF_802x_Rx leaves one for
 * NetIPv4_Rx: IP_HdrIx, DataLen and TotLen without the interface header, the protocol type headers, and
 * the flags of a frame from a remote host, with RX_BROADCAST where `bcast` says the frame's destination
 * was the broadcast or a group address. host / mask / group in host order. Returns 0, or the
 * start-state step that failed. */
int RefIPv4_Rx(const uint8_t *dgram, uint16_t received, uint32_t bcast, uint32_t host, uint32_t mask, uint32_t group,
               REFIPV4_OUT *out) {
    static NET_BUF    buf;
    static CPU_INT08U data[14u + 65535u + 64u];
    NET_CTR_ERRS      before;
    NET_ERR           err = NET_ERR_NONE;
    uint32_t          named = 0u, all = 0u;
    size_t            i;
    int               rc;

    memset(out, 0, sizeof *out);
    cur = (REFIPV4_OUT *)0;
    rc  = start_state(host, mask, group);
    if (rc != 0) return rc;

    memset(&buf, 0, sizeof buf);
    memset(data, 0, 14u);
    memcpy(data + 14u, dgram, received);
    memset(data + 14u + received, 0xA5, 64u);
    buf.DataPtr                = data;
    buf.Hdr.Type               = NET_BUF_TYPE_RX_LARGE;
    buf.Hdr.IF_Nbr             = REF_IF_NBR;
    buf.Hdr.IF_NbrTx           = REF_IF_NBR;
    buf.Hdr.TotLen             = received;
    buf.Hdr.DataLen            = received;
    buf.Hdr.IF_HdrIx           = 0u;
    buf.Hdr.IF_HdrLen          = 14u;
    buf.Hdr.IP_HdrIx           = 14u;
    buf.Hdr.ProtocolHdrType    = NET_PROTOCOL_TYPE_IP_V4;
    buf.Hdr.ProtocolHdrTypeIF  = NET_PROTOCOL_TYPE_IF_ETHER;
    buf.Hdr.ProtocolHdrTypeNet = NET_PROTOCOL_TYPE_IP_V4;
    buf.Hdr.Flags              = NET_BUF_FLAG_RX_REMOTE | (bcast ? NET_BUF_FLAG_RX_BROADCAST : NET_BUF_FLAG_NONE);

    before  = Net_ErrCtrs;
    cur     = out;
    cur_buf = &buf;

    NetIPv4_Rx(&buf, &err);

    out->err = (int32_t)err;
    for (i = 0u; i < N_CTRS; ++i) {
        out->ctr[i] = *(const NET_CTR *)((const char *)&Net_ErrCtrs + ctr_off[i]) - *(const NET_CTR *)((const char *)&before + ctr_off[i]);
        named += out->ctr[i];
    }
    for (i = 0u; i < sizeof(NET_CTR_ERRS) / sizeof(NET_CTR); ++i) {
        all += ((const NET_CTR *)&Net_ErrCtrs)[i] - ((const NET_CTR *)&before)[i];
    }
    out->ctr_other = all - named;
    cur = (REFIPV4_OUT *)0;
    for (i = 0u; i < out->n_calls && i < MAX_CALLS; ++i) {       /* Hdr* offsets: from the IP header */
        if (out->calls[i].fn <= FN_HDR_VERIFY && out->calls[i].off != 0xFFFFFFFFu) out->calls[i].off -= 14u;
        else if (out->calls[i].fn > FN_HDR_VERIFY) out->calls[i].off -= 14u;
    }
    if (frag_tmr != (NET_TMR *)0 && frag_tmr->Fnct != (CPU_FNCT_PTR)0) {   /* the lone fragment's list times out */
        frag_tmr->Fnct(frag_tmr->Obj);
    }
    Net_ErrCtrs = before;
    cur_buf     = (NET_BUF *)0;
    return 0;
}
