/* Stand-in for the library's random-number interface (see cpu.h here); glue.c defines it. */
#ifndef NETCSUM_REF_LIB_MATH_H
#define NETCSUM_REF_LIB_MATH_H

#include <lib_def.h>

typedef CPU_INT32U RAND_NBR;

extern RAND_NBR Math_RandSeedCur;
void     Math_RandSetSeed(RAND_NBR seed);
RAND_NBR Math_Rand(void);
RAND_NBR Math_RandSeed(RAND_NBR seed);                /* the number that follows `seed` */

#endif
