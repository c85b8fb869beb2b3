/* Stand-in for the library's common definitions (see cpu.h here): the constants and bit / range
 * macros net_util.c and the stack headers it includes use. Everything is a plain integer constant
 * expression, so the range checks work inside #if. */
#ifndef NETCSUM_REF_LIB_DEF_H
#define NETCSUM_REF_LIB_DEF_H

#include <cpu.h>

#define LIB_VERSION               13800u            /* the stack asks for >= 1.38.00 */

#define DEF_NULL                  0
#define DEF_FALSE                 0u
#define DEF_TRUE                  1u
#define DEF_NO                    0u
#define DEF_YES                   1u
#define DEF_DISABLED              0u
#define DEF_ENABLED               1u
#define DEF_OFF                   0u
#define DEF_ON                    1u
#define DEF_FAIL                  0u
#define DEF_OK                    1u

#define DEF_OCTET_NBR_BITS        8u
#define DEF_OCTET_MASK            0xFFu

#define DEF_INT_08U_MAX_VAL       0xFFu
#define DEF_INT_16U_MAX_VAL       0xFFFFu
#define DEF_INT_32U_MAX_VAL       0xFFFFFFFFu
#define DEF_INT_CPU_U_MAX_VAL     0xFFFFFFFFFFFFFFFFu

#define DEF_TIME_NBR_mS_PER_SEC   1000u
#define DEF_TIME_NBR_uS_PER_SEC   1000000u

/* bits and masks */
#define DEF_BIT_NONE              0u
#define DEF_BIT(n)                (1u << (n))
#define DEF_BIT_00                DEF_BIT(0)
#define DEF_BIT_01                DEF_BIT(1)
#define DEF_BIT_02                DEF_BIT(2)
#define DEF_BIT_03                DEF_BIT(3)
#define DEF_BIT_04                DEF_BIT(4)
#define DEF_BIT_05                DEF_BIT(5)
#define DEF_BIT_06                DEF_BIT(6)
#define DEF_BIT_07                DEF_BIT(7)
#define DEF_BIT_12                DEF_BIT(12)
#define DEF_BIT_13                DEF_BIT(13)
#define DEF_BIT_SET(val, mask)    ((val) |= (mask))
#define DEF_BIT_CLR(val, mask)    ((val) &= ~(mask))
#define DEF_BIT_IS_SET(val, mask) (((mask) != 0u && ((val) & (mask)) == (mask)) ? DEF_YES : DEF_NO)
#define DEF_BIT_IS_CLR(val, mask) (((mask) != 0u && ((val) & (mask)) == 0u) ? DEF_YES : DEF_NO)

/* range checks: DEF_OK inside the range, DEF_FAIL outside */
#define DEF_CHK_VAL_MIN(val, lo)  (((val) < (lo)) ? DEF_FAIL : DEF_OK)
#define DEF_CHK_VAL_MAX(val, hi)  (((val) > (hi)) ? DEF_FAIL : DEF_OK)
#define DEF_CHK_VAL(val, lo, hi)  ((((val) < (lo)) || ((val) > (hi))) ? DEF_FAIL : DEF_OK)

#define DEF_MIN(a, b)             (((a) < (b)) ? (a) : (b))
#define DEF_MAX(a, b)             (((a) > (b)) ? (a) : (b))

#endif
