/* Stand-in for the CPU core services header (see cpu.h here). With 32-bit timestamps disabled the
 * stack uses only the type names below (the core version it asks for is in cpu.h). */
#ifndef NETCSUM_REF_CPU_CORE_H
#define NETCSUM_REF_CPU_CORE_H

#include <cpu.h>
#include <lib_def.h>

typedef int         CPU_ERR;
#define CPU_ERR_NONE         0

typedef CPU_INT32U  CPU_TS32;
typedef CPU_INT64U  CPU_TS64;
typedef CPU_TS32    CPU_TS;
typedef CPU_INT32U  CPU_TS_TMR_FREQ;

/* the stack's "cannot happen" exit (argument checks of the external-call layer): stop the process */
#define CPU_SW_EXCEPTION(ret) __builtin_trap()

#define CPU_CFG_TS_32_EN     DEF_DISABLED
#define CPU_CFG_TS_64_EN     DEF_DISABLED

#endif
