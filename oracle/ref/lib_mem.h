/* Stand-in for the library's memory header (see cpu.h here): the pool types the stack's structures
 * hold by value (opaque here), the host <-> big-endian value macros for a little-endian host, the
 * octet-wise value access macros (any alignment) and the memory routines net_if_802x.c
 * calls (defined in glue_802x.c). */
#ifndef NETCSUM_REF_LIB_MEM_H
#define NETCSUM_REF_LIB_MEM_H

#include <lib_def.h>

typedef int         LIB_ERR;
#define LIB_MEM_ERR_NONE  0
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

/* octet-wise access: a big-endian 16-bit value at any address, and plain octet copies */
#define MEM_VAL_GET_INT16U_BIG(addr) ((CPU_INT16U)(((CPU_INT16U)((const CPU_INT08U *)(addr))[0] << 8) | \
                                                   ((CPU_INT16U)((const CPU_INT08U *)(addr))[1])))
#define MEM_VAL_COPY(dest, src, size) do { CPU_SIZE_T mem_val_i_; \
                                           for (mem_val_i_ = 0u; mem_val_i_ < (CPU_SIZE_T)(size); ++mem_val_i_) { \
                                               ((CPU_INT08U *)(dest))[mem_val_i_] = ((const CPU_INT08U *)(src))[mem_val_i_]; \
                                           } } while (0)
#define MEM_VAL_COPY_SWAP_16_(dest, src) do { const CPU_INT08U mem_val_b0_ = ((const CPU_INT08U *)(src))[0]; \
                                              ((CPU_INT08U *)(dest))[0] = ((const CPU_INT08U *)(src))[1]; \
                                              ((CPU_INT08U *)(dest))[1] = mem_val_b0_; } while (0)
#define MEM_VAL_COPY_SWAP_32_(dest, src) do { CPU_INT08U mem_val_t_[4]; MEM_VAL_COPY(mem_val_t_, src, 4u); \
                                              ((CPU_INT08U *)(dest))[0] = mem_val_t_[3]; ((CPU_INT08U *)(dest))[1] = mem_val_t_[2]; \
                                              ((CPU_INT08U *)(dest))[2] = mem_val_t_[1]; ((CPU_INT08U *)(dest))[3] = mem_val_t_[0]; } while (0)
#define MEM_VAL_COPY_16(dest, src)             MEM_VAL_COPY(dest, src, 2u)
#define MEM_VAL_COPY_32(dest, src)             MEM_VAL_COPY(dest, src, 4u)
#define MEM_VAL_COPY_SET_INT32U(dest, src)     MEM_VAL_COPY(dest, src, 4u)     /* host order: little-endian */
#define MEM_VAL_COPY_GET_INT32U_BIG(dest, src) MEM_VAL_COPY_SWAP_32_(dest, src)
#define MEM_VAL_COPY_SET_INT32U_BIG(dest, src) MEM_VAL_COPY_SWAP_32_(dest, src)
#define MEM_VAL_SET_INT16U_BIG(addr, val)      do { ((CPU_INT08U *)(addr))[0] = (CPU_INT08U)((CPU_INT16U)(val) >> 8); \
                                                    ((CPU_INT08U *)(addr))[1] = (CPU_INT08U)(val); } while (0)
#define MEM_VAL_SET_INT32U_BIG(addr, val)      do { ((CPU_INT08U *)(addr))[0] = (CPU_INT08U)((CPU_INT32U)(val) >> 24); \
                                                    ((CPU_INT08U *)(addr))[1] = (CPU_INT08U)((CPU_INT32U)(val) >> 16); \
                                                    ((CPU_INT08U *)(addr))[2] = (CPU_INT08U)((CPU_INT32U)(val) >> 8); \
                                                    ((CPU_INT08U *)(addr))[3] = (CPU_INT08U)(val); } while (0)
#define MEM_VAL_COPY_GET_INT16U_BIG(dest, src) MEM_VAL_COPY_SWAP_16_(dest, src)
#define MEM_VAL_COPY_SET_INT16U_BIG(dest, src) MEM_VAL_COPY_SWAP_16_(dest, src)

void        Mem_Clr(void *pmem, CPU_SIZE_T size);
void        Mem_Copy(void *pdest, const void *psrc, CPU_SIZE_T size);
CPU_BOOLEAN Mem_Cmp(const void *p1_mem, const void *p2_mem, CPU_SIZE_T size);   /* DEF_YES: all octets equal */

#endif
