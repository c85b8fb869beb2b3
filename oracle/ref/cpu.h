/* Stand-in for the CPU port header the reference's net_util.c expects (oracle/Makefile `ref`).
 * Our own text: an LP64 little-endian host described in the names net_util.c and the headers it
 * pulls in use, and nothing more. Test infrastructure only; the product never includes it. */
#ifndef NETCSUM_REF_CPU_H
#define NETCSUM_REF_CPU_H

#include <stddef.h>
#include <stdint.h>

typedef void      CPU_VOID;
typedef char      CPU_CHAR;
typedef uint8_t   CPU_BOOLEAN;
typedef uint8_t   CPU_INT08U;
typedef int8_t    CPU_INT08S;
typedef uint16_t  CPU_INT16U;
typedef int16_t   CPU_INT16S;
typedef uint32_t  CPU_INT32U;
typedef int32_t   CPU_INT32S;
typedef uint64_t  CPU_INT64U;
typedef int64_t   CPU_INT64S;
typedef float     CPU_FP32;
typedef double    CPU_FP64;

typedef uintptr_t CPU_ADDR;                 /* an address, as an integer          */
typedef uintptr_t CPU_DATA;                 /* the natural data word              */
typedef CPU_DATA  CPU_ALIGN;                /* the word alignment is counted in   */
typedef size_t    CPU_SIZE_T;
typedef uint32_t  CPU_SR;                   /* saved status word: unused here     */

typedef void (*CPU_FNCT_VOID)(void);
typedef void (*CPU_FNCT_PTR)(void *);

#define CPU_WORD_SIZE_08          1
#define CPU_WORD_SIZE_16          2
#define CPU_WORD_SIZE_32          4
#define CPU_WORD_SIZE_64          8

#define CPU_CFG_ADDR_SIZE         CPU_WORD_SIZE_64
#define CPU_CFG_DATA_SIZE         CPU_WORD_SIZE_64
#define CPU_CFG_DATA_SIZE_MAX     CPU_WORD_SIZE_64

#define CPU_ENDIAN_TYPE_NONE      0
#define CPU_ENDIAN_TYPE_BIG       1
#define CPU_ENDIAN_TYPE_LITTLE    2
#define CPU_CFG_ENDIAN_TYPE       CPU_ENDIAN_TYPE_LITTLE

/* the stack asks for a core version of at least 1.30; net.h checks it with only this header included */
#define CPU_CORE_VERSION          13000u

/* critical sections: one thread, nothing to mask */
#define CPU_SR_ALLOC()
#define CPU_CRITICAL_ENTER()      do { } while (0)
#define CPU_CRITICAL_EXIT()       do { } while (0)

#endif
