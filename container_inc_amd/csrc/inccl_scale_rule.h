/* inccl_scale_rule.h -- the INCCL_SCALE_AUTO rule, stated once for the host and
 * the device, in integer arithmetic on an absmax WORD.  Pure C: the public
 * inccl_choose_scale / inccl_choose_scale_word (api.c), the single-scale
 * kernels' prologue (resolve_k, inccl_stream.h) and the per-block kernels
 * (block_mul, inccl_block.h: one exponent per 256-element block) all call it,
 * and a stand-alone program walks it against the oracle's double-precision
 * rule (tests/c/scale_rule.c).
 *
 * The rule (inccl_choose_scale): amax = 0 or NaN -> INCCL_SCALE_MAX, Inf ->
 * INCCL_SCALE_MIN, else with t = amax * R = m * 2^e, m in [0.5, 1):
 * k = 30 - e, or 31 - e when m == 0.5, clamped.  Here amax = M * 2^(E - 150)
 * with M the 24-bit significand (no hidden bit for a subnormal, E = 1) and
 * P = M * R an exact 64-bit product (M < 2^24, R < 2^31), so with h the index
 * of P's highest set bit e = h + E - 149, and m == 0.5 iff P is a power of two. */
#ifndef INCCL_SCALE_RULE_H
#define INCCL_SCALE_RULE_H

#include <stdint.h>

#include "inccl_amd.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define INCCL_HD __host__ __device__ __forceinline__
#else
#define INCCL_HD static inline
#endif

/* the exponent of an absmax word; bit 31 (INCCL_ABSMAX_FLAG_NONFINITE) is ignored */
INCCL_HD int inccl_scale_of_word(uint32_t word, int R)
{
    const uint32_t bits = word & 0x7fffffffu;
    if (bits == 0u || bits > 0x7f800000u) return INCCL_SCALE_MAX;
    if (bits == 0x7f800000u) return INCCL_SCALE_MIN;
    const uint32_t be = bits >> 23;
    const uint64_t M = (uint64_t)((bits & 0x7fffffu) | (be ? 0x800000u : 0u));
    const int E = be ? (int)be : 1;
    const uint64_t P = M * (uint64_t)(uint32_t)(R > 0 ? R : 1);
    const int h = 63 - __builtin_clzll(P);
    int k = 30 - (h + E - 149) + ((P & (P - 1)) == 0 ? 1 : 0);
    k = k < INCCL_SCALE_MIN ? INCCL_SCALE_MIN : k;
    k = k > INCCL_SCALE_MAX ? INCCL_SCALE_MAX : k;
    return k;
}

/* The exponent the single-scale kernels resolve from the device's absmax word
 * (resolve_k, inccl_stream.h): a word that carries bit 31 gives INCCL_SCALE_MAX,
 * any other word the rule above.  The float results of a flagged call are NaN
 * whatever the exponent (deq_scale), and its int32 wire words were always
 * quantised at INCCL_SCALE_MAX: the flagged word read as a float is negative,
 * "not greater than 0", which is the oracle's rule on it.  The per-block modes
 * (block_mul) and the host's inccl_choose_scale_word scale the magnitude
 * instead. */
INCCL_HD int inccl_scale_of_device_word(uint32_t word, int R)
{
    return (word >> 31) ? INCCL_SCALE_MAX : inccl_scale_of_word(word, R);
}

/* the rule on a float absmax (inccl_choose_scale): not greater than 0 -- a
 * negative value carries bit 31 -- or NaN -> INCCL_SCALE_MAX, +Inf -> INCCL_SCALE_MIN */
INCCL_HD int inccl_scale_of_float(float amax, int R)
{
    uint32_t bits;
    __builtin_memcpy(&bits, &amax, sizeof(bits));
    return inccl_scale_of_device_word(bits, R);
}

/* Packed 16-bit lanes (INCCL_KIND_P16): 16 bits less than the 32-bit rule, so
 * that R contributions of |q| <= ceil(2^14 / R) sum inside a signed 16-bit
 * lane; a zero block gets INCCL_SCALE_MAX - 16. */
INCCL_HD int inccl_p16_scale_of_word(uint32_t word, int R)
{
    const int k = inccl_scale_of_word(word, R) - 16;
    return k < INCCL_SCALE_MIN ? INCCL_SCALE_MIN : k;
}

/* the largest contribution one of R contributors may add to a lane: the clamp
 * binds only where the exponent was clamped at INCCL_SCALE_MIN and for +-Inf,
 * and keeps a lane's sum inside [-32767, 32767] whatever the inputs */
#define INCCL_P16_LANE_MAX 32767
INCCL_HD int inccl_p16_clamp(int R) { return INCCL_P16_LANE_MAX / (R > 0 ? R : 1); }

#endif
