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
#define DEF_CLR                   0u
#define DEF_SET                   1u
#define DEF_FAIL                  0u
#define DEF_OK                    1u

#define DEF_OCTET_NBR_BITS        8u
#define DEF_OCTET_MASK            0xFFu
#define DEF_NIBBLE_MASK           0x0Fu

#define DEF_INT_08U_MAX_VAL       0xFFu
#define DEF_INT_16U_MAX_VAL       0xFFFFu
#define DEF_INT_32U_MAX_VAL       0xFFFFFFFFu
#define DEF_INT_CPU_U_MAX_VAL     0xFFFFFFFFFFFFFFFFu
#define DEF_INT_08U_MIN_VAL       0u
#define DEF_INT_16U_MIN_VAL       0u
#define DEF_INT_32U_MIN_VAL       0u
#define DEF_INT_08S_MIN_VAL       (-128)
#define DEF_INT_08S_MAX_VAL       127
#define DEF_INT_16S_MIN_VAL       (-32768)
#define DEF_INT_16S_MAX_VAL       32767
#define DEF_INT_32S_MIN_VAL       (-2147483647 - 1)
#define DEF_INT_32S_MAX_VAL       2147483647

#define DEF_TIME_NBR_mS_PER_SEC   1000u
#define DEF_TIME_NBR_uS_PER_SEC   1000000u
#define DEF_TIME_NBR_SEC_PER_MIN  60u
#define DEF_TIME_NBR_SEC_PER_HR   3600u

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
#define DEF_BIT_08                DEF_BIT(8)
#define DEF_BIT_09                DEF_BIT(9)
#define DEF_BIT_10                DEF_BIT(10)
#define DEF_BIT_11                DEF_BIT(11)
#define DEF_BIT_12                DEF_BIT(12)
#define DEF_BIT_13                DEF_BIT(13)
#define DEF_BIT_14                DEF_BIT(14)
#define DEF_BIT_15                DEF_BIT(15)
#define DEF_BIT_16                DEF_BIT(16)
#define DEF_BIT_17                DEF_BIT(17)
#define DEF_BIT_18                DEF_BIT(18)
#define DEF_BIT_19                DEF_BIT(19)
#define DEF_BIT_20                DEF_BIT(20)
#define DEF_BIT_21                DEF_BIT(21)
#define DEF_BIT_22                DEF_BIT(22)
#define DEF_BIT_23                DEF_BIT(23)
#define DEF_BIT_24                DEF_BIT(24)
#define DEF_BIT_25                DEF_BIT(25)
#define DEF_BIT_26                DEF_BIT(26)
#define DEF_BIT_27                DEF_BIT(27)
#define DEF_BIT_28                DEF_BIT(28)
#define DEF_BIT_29                DEF_BIT(29)
#define DEF_BIT_30                DEF_BIT(30)
#define DEF_BIT_31                DEF_BIT(31)
#define DEF_BIT_SET(val, mask)    ((val) |= (mask))
#define DEF_BIT_CLR(val, mask)    ((val) &= ~(mask))
#define DEF_BIT_IS_SET(val, mask) (((mask) != 0u && ((val) & (mask)) == (mask)) ? DEF_YES : DEF_NO)
#define DEF_BIT_IS_CLR(val, mask) (((mask) != 0u && ((val) & (mask)) == 0u) ? DEF_YES : DEF_NO)

#define DEF_BIT_IS_SET_ANY(val, mask) ((((val) & (mask)) != 0u) ? DEF_YES : DEF_NO)

/* range checks: DEF_OK inside the range, DEF_FAIL outside */
#define DEF_CHK_VAL_MIN(val, lo)  (((val) < (lo)) ? DEF_FAIL : DEF_OK)
#define DEF_CHK_VAL_MAX(val, hi)  (((val) > (hi)) ? DEF_FAIL : DEF_OK)
#define DEF_CHK_VAL(val, lo, hi)  ((((val) < (lo)) || ((val) > (hi))) ? DEF_FAIL : DEF_OK)

#define DEF_ABS(a)                (((a) < 0) ? -(a) : (a))
#define DEF_MIN(a, b)             (((a) < (b)) ? (a) : (b))
#define DEF_MAX(a, b)             (((a) > (b)) ? (a) : (b))

#endif
