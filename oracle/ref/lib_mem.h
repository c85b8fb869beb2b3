/* Stand-in for the library's memory header (see cpu.h here): the pool types the stack's structures
 * hold by value (opaque here) and the host <-> big-endian value macros for a little-endian host. */
#ifndef NETCSUM_REF_LIB_MEM_H
#define NETCSUM_REF_LIB_MEM_H

#include <lib_def.h>

typedef int         LIB_ERR;
typedef CPU_INT32U  MEM_POOL_BLK_QTY;
typedef struct { void *opaque; } MEM_SEG;
typedef struct { void *opaque; } MEM_POOL;
typedef struct { void *opaque; } MEM_DYN_POOL;

#define MEM_VAL_SWAP_16(val)         ((CPU_INT16U)((((CPU_INT16U)(val) & 0x00FFu) << 8) | \
                                                   (((CPU_INT16U)(val) & 0xFF00u) >> 8)))
#define MEM_VAL_SWAP_32(val)         ((CPU_INT32U)((((CPU_INT32U)(val) & 0x000000FFu) << 24) | \
                                                   (((CPU_INT32U)(val) & 0x0000FF00u) <<  8) | \
                                                   (((CPU_INT32U)(val) & 0x00FF0000u) >>  8) | \
                                                   (((CPU_INT32U)(val) & 0xFF000000u) >> 24)))
#define MEM_VAL_HOST_TO_BIG_16(val)  MEM_VAL_SWAP_16(val)
#define MEM_VAL_BIG_TO_HOST_16(val)  MEM_VAL_SWAP_16(val)
#define MEM_VAL_HOST_TO_BIG_32(val)  MEM_VAL_SWAP_32(val)
#define MEM_VAL_BIG_TO_HOST_32(val)  MEM_VAL_SWAP_32(val)

#endif
