/*
 * netcsum_fragsum.c — host side of the fragment payload sums (include/netcsum_mi355x.h (2b''')).
 * Plain C11, host logic only.
 *
 * NetUtil_MI355X_RxBurstSums reports, per fragment, the folded one's-complement sum of its IP
 * payload. Where the stack completes a reassembled datagram (NetIPv4_RxPktFragReasm,
 * net_ipv4.c:6523) these two functions give what NetUtil_16BitOnesCplChkSumDataCalc / DataVerify
 * (net_util.c:344-363, :428-449) would return for the chain of the fragments' NET_BUFs with the
 * transport layer's pseudo-header, from the records alone.
 *
 * The reference sums the chain as one octet stream (net_util.c:1591-1687): big-endian 16-bit words,
 * an odd buffer's last octet carried in front of the next buffer's first (:1385-1393, :1463-1470),
 * the stream's odd last octet padded with zero (:1464-1466). A record's sum is its payload's own
 * word sum (padded), folded, as a host-order value, i.e. byte-swapped on a little-endian host.
 * One's-complement addition commutes with the byte swap (RFC 1071 section 2 (B)), and a piece that
 * starts at an odd stream offset has every octet in the other half of its word, which is the swap
 * again. So the stream's folded sum is the one's-complement sum of the pseudo-header's and the
 * records' sums, each swapped when an odd number of octets precedes it. Folding keeps 0 apart from
 * 0xFFFF (a folded sum is 0 only when every term is 0, and a record's sum is 0 only when every octet
 * is), so the result is the reference's in its all-zero corner too.
 */
#include "../../include/netcsum_mi355x.h"

#include <stddef.h>

#define FS_NEG_ZERO  0xFFFFu                /* NET_UTIL_16_BIT_ONES_CPL_NEG_ZERO (net_util.c:56) */
#define FS_MAX_OCTETS 65535u                /* no IP datagram is longer */

#if defined(__BYTE_ORDER__) && (__BYTE_ORDER__ == __ORDER_BIG_ENDIAN__)
#define FS_HOST_BIG 1
#else
#define FS_HOST_BIG 0
#endif

static uint32_t fs_swap16(uint32_t v)
{
    return ((v & 0xFFu) << 8) | ((v >> 8) & 0xFFu);
}

static uint32_t fs_fold(uint32_t sum)
{
    while (sum >> 16) {
        sum = (sum & 0xFFFFu) + (sum >> 16);
    }
    return sum;
}

/* The stream's folded sum of big-endian words (the reference's `sum` at net_util.c:1694). */
static NET_ERR fs_sum(const NETCSUM_FRAG_SUM *frag, uint32_t n_frag, const void *ppseudo_hdr,
                      CPU_INT16U pseudo_hdr_size, uint32_t *p_sum)
{
    const uint8_t *ph = (const uint8_t *)ppseudo_hdr;
    uint32_t sum = 0u, octets = 0u, pos = 0u, i;

    if ((frag == NULL && n_frag != 0u) || (ppseudo_hdr == NULL && pseudo_hdr_size != 0u)) {
        return NET_ERR_FAULT_NULL_PTR;
    }
    for (i = 0u; i < n_frag; ++i) {
        octets += frag[i].len;
        if (octets > FS_MAX_OCTETS) {
            return (NET_ERR)NET_UTIL_ERR_MI355X_INVALID_ARG;
        }
    }
    if (ph != NULL) {                                         /* :1591-1609 */
        uint32_t len = pseudo_hdr_size;
        if (n_frag == 0u && (len & 1u) != 0u) {
            len -= 1u;                                        /* NULL chain: the carried octet is never summed */
        }
        for (i = 0u; i + 1u < len; i += 2u) {
            sum += ((uint32_t)ph[i] << 8) | ph[i + 1u];
        }
        if (i < len) {
            sum += (uint32_t)ph[i] << 8;                      /* carried (:1468) or padded (:1465) */
        }
        sum = fs_fold(sum);                                   /* (at most 32 768 words: no wrap) */
        pos = len;
    }
    for (i = 0u; i < n_frag; ++i) {
        uint32_t be;
        if (frag[i].len == 0u) {
            continue;                                         /* an empty buffer passes the carry on */
        }
        be = FS_HOST_BIG ? frag[i].sum : fs_swap16(frag[i].sum);
        sum += (pos & 1u) ? fs_swap16(be) : be;
        sum = fs_fold(sum);                                   /* folded per term: no wrap for any n_frag */
        pos += frag[i].len;
    }
    *p_sum = sum;
    return NET_UTIL_ERR_NONE;
}

static uint16_t fs_net_to_host(uint32_t v)
{
    return (uint16_t)(FS_HOST_BIG ? v : fs_swap16(v));
}

NET_ERR NetUtil_MI355X_FragSumCalc(const NETCSUM_FRAG_SUM *frag, uint32_t n_frag, const void *ppseudo_hdr,
                                   CPU_INT16U pseudo_hdr_size, NET_CHK_SUM *p_chk_sum)
{
    uint32_t sum = 0u;
    NET_ERR err;

    if (p_chk_sum == NULL) {
        return NET_ERR_FAULT_NULL_PTR;
    }
    err = fs_sum(frag, n_frag, ppseudo_hdr, pseudo_hdr_size, &sum);
    if (err != NET_UTIL_ERR_NONE) {
        return err;
    }
    *p_chk_sum = (NET_CHK_SUM)~fs_net_to_host(sum);           /* net_util.c:358 */
    return NET_UTIL_ERR_NONE;
}

NET_ERR NetUtil_MI355X_FragSumVerify(const NETCSUM_FRAG_SUM *frag, uint32_t n_frag, const void *ppseudo_hdr,
                                     CPU_INT16U pseudo_hdr_size, CPU_BOOLEAN *p_ok)
{
    uint32_t sum = 0u;
    NET_ERR err;

    if (p_ok == NULL) {
        return NET_ERR_FAULT_NULL_PTR;
    }
    err = fs_sum(frag, n_frag, ppseudo_hdr, pseudo_hdr_size, &sum);
    if (err != NET_UTIL_ERR_NONE) {
        return err;
    }
    *p_ok = (fs_net_to_host(sum) == FS_NEG_ZERO) ? DEF_OK : DEF_FAIL;   /* net_util.c:443-444 */
    return NET_UTIL_ERR_NONE;
}
