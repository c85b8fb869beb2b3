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

#endif
