/* Prints, from the reference's own net_buf.h under the template configuration, the offset of every
 * NET_BUF field the chain walk of net_util.c reads, and the structure sizes: "name value" lines that
 * tests/golden/make_reference_vectors.py and tests/test_reference_cpu.py compare with the mirror in
 * include/netcsum_netbuf.h and netcsum.NetBuf. */
#include <stddef.h>
#include <stdio.h>

#include "net_buf.h"

#define HDR_FIELD(f) printf("%s %zu\n", #f, offsetof(NET_BUF_HDR, f))

int main(void) {
    HDR_FIELD(NextBufPtr);
    HDR_FIELD(ProtocolHdrType);
    HDR_FIELD(ICMP_MsgIx);
    HDR_FIELD(ICMP_HdrLen);
    HDR_FIELD(TransportHdrIx);
    HDR_FIELD(TransportHdrLen);
    HDR_FIELD(DataLen);
    HDR_FIELD(TotLen);
    printf("DataPtr %zu\n", offsetof(NET_BUF, DataPtr));
    printf("sizeof_NET_BUF_HDR %zu\n", sizeof(NET_BUF_HDR));
    printf("sizeof_NET_BUF %zu\n", sizeof(NET_BUF));
    printf("sizeof_ProtocolHdrType %zu\n", sizeof(((NET_BUF_HDR *)0)->ProtocolHdrType));
    return 0;
}
