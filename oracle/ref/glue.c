/* The few symbols the reference's net_util.c links against besides itself: a fixed-step generator
 * and a still clock. None of them is on the path of a checksum or CRC routine. */
#include <lib_math.h>
#include <KAL/kal.h>

RAND_NBR         Math_RandSeedCur = 1u;
KAL_TICK_RATE_HZ KAL_TickRate     = 1000u;

void Math_RandSetSeed(RAND_NBR seed) { Math_RandSeedCur = seed; }

RAND_NBR Math_Rand(void) {
    Math_RandSeedCur = Math_RandSeedCur * 1103515245u + 12345u;
    return Math_RandSeedCur;
}

RAND_NBR Math_RandSeed(RAND_NBR seed) { return seed * 1103515245u + 12345u; }

KAL_TICK KAL_TickGet(KAL_ERR *p_err) {
    *p_err = KAL_ERR_NONE;
    return 0u;
}
