/* inccl_scale_rule.h -- the INCCL_SCALE_AUTO rule on an absmax WORD, in integer
 * arithmetic.  Pure C, host and device: the per-block kernels (inccl_block.hip)
 * resolve one exponent per 256-element block with it instead of a
 * double-precision frexp, and a stand-alone program walks it against the
 * oracle's rule (tests/c/scale_rule.c).
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
