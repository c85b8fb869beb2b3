/* Stand-in for the kernel abstraction layer (see ../cpu.h): handle types the stack's structures
 * hold, and the tick interface net_util.c's time helpers call; glue.c defines the latter. */
#ifndef NETCSUM_REF_KAL_H
#define NETCSUM_REF_KAL_H

#include <lib_def.h>

typedef int         KAL_ERR;
#define KAL_ERR_NONE  0

typedef CPU_INT32U  KAL_TICK;
typedef CPU_INT32U  KAL_TICK_RATE_HZ;

typedef struct { void *opaque; } KAL_LOCK_HANDLE;
typedef struct { void *opaque; } KAL_SEM_HANDLE;
typedef struct { void *opaque; } KAL_TMR_HANDLE;
typedef struct { void *opaque; } KAL_Q_HANDLE;
typedef struct { void *opaque; } KAL_TASK_HANDLE;
typedef struct { void *opaque; } KAL_MON_HANDLE;

extern KAL_TICK_RATE_HZ KAL_TickRate;
KAL_TICK KAL_TickGet(KAL_ERR *p_err);

/* the error codes and options net_tcp.c's connection-queue code names, and the two creators whose
 * handles it stores (glue_ipv4.c defines them and the Sem calls; nothing on the receive path of a
 * single datagram pends on one) */
#define KAL_ERR_NULL_PTR     1
#define KAL_ERR_INVALID_ARG  2
#define KAL_ERR_MEM_ALLOC    3
#define KAL_ERR_ISR          4
#define KAL_ERR_CREATE       5
#define KAL_ERR_OS           6
#define KAL_ERR_OVF          7
#define KAL_ERR_TIMEOUT      8
#define KAL_ERR_ABORT        9
#define KAL_ERR_LOCK_OWNER  10

typedef CPU_INT32U  KAL_OPT;
#define KAL_OPT_NONE             0u
#define KAL_OPT_PEND_NONE        0u
#define KAL_OPT_PEND_BLOCKING    0u
#define KAL_OPT_PEND_NON_BLOCKING 1u
#define KAL_OPT_POST_NONE        0u
#define KAL_OPT_CREATE_NONE      0u

KAL_SEM_HANDLE  KAL_SemCreate (const CPU_CHAR *p_name, void *p_cfg, KAL_ERR *p_err);
KAL_LOCK_HANDLE KAL_LockCreate(const CPU_CHAR *p_name, void *p_cfg, KAL_ERR *p_err);

#endif
