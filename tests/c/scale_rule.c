/* scale_rule.c -- the integer form of the auto scale rule that every kernel
 * and the host run (csrc/inccl_scale_rule.h) against the oracle's
 * double-precision one (oracle/inccl_oracle.c orc_choose_scale), which is the
 * spec: inccl_scale_of_word on the word's magnitude (the per-block kernels),
 * inccl_scale_of_float on the magnitude as a float (inccl_choose_scale), and
 * inccl_scale_of_device_word against the oracle on the WHOLE word read as a
 * float, flagged words included (what the single-scale kernels resolve).  Words: every exponent field with the significands where the
 * rule can turn (all zeros, all ones, one bit, the patterns next to a power of
 * two and to 2^j / R), the zero, the subnormals, Inf and NaNs, each with and
 * without bit 31, then a fixed pseudo-random sweep; R: 1..64 and larger worlds.
 * Host code only:
 *   gcc -std=gnu11 -I include -I container_inc_amd/csrc -I oracle tests/c/scale_rule.c oracle/inccl_oracle.c -lm */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "inccl_oracle.h"
#include "inccl_scale_rule.h"

static long cases, bad;

static void check(uint32_t word, int R)
{
    const uint32_t bits = word & 0x7fffffffu;
    float amax;
    memcpy(&amax, &bits, sizeof(amax));
    const int want = orc_choose_scale(amax, R), got = inccl_scale_of_word(word, R);
    ++cases;
    if (want != got && ++bad <= 20) printf("MISMATCH word %08x R %d: %d, the oracle says %d\n", word, R, got, want);
    const int gotf = inccl_scale_of_float(amax, R);
    if (want != gotf && ++bad <= 20) printf("MISMATCH float %08x R %d: %d, the oracle says %d\n", bits, R, gotf, want);
    float whole;
    memcpy(&whole, &word, sizeof(whole));
    const int wantd = orc_choose_scale(whole, R), gotd = inccl_scale_of_device_word(word, R);
    if (wantd != gotd && ++bad <= 20)
        printf("MISMATCH device word %08x R %d: %d, the oracle says %d\n", word, R, gotd, wantd);
}

/* the float entry where no absmax word goes: -0, negative values, -Inf, NaNs */
static void check_float(float amax, int R)
{
    const int want = orc_choose_scale(amax, R), got = inccl_scale_of_float(amax, R);
    ++cases;
    if (want != got && ++bad <= 20) printf("MISMATCH float %g R %d: %d, the oracle says %d\n", (double)amax, R, got, want);
}

/* R <= 0 counts as one contributor */
static void check_r_floor(uint32_t word)
{
    float amax;
    memcpy(&amax, &word, sizeof(amax));
    for (int R = -3; R <= 0; R += 3) {
        ++cases;
        if ((inccl_scale_of_float(amax, R) != inccl_scale_of_float(amax, 1) ||
             inccl_scale_of_device_word(word, R) != inccl_scale_of_device_word(word, 1) ||
             inccl_scale_of_word(word, R) != inccl_scale_of_word(word, 1)) &&
            ++bad <= 20)
            printf("MISMATCH word %08x: R %d is not R 1\n", word, R);
    }
}

int main(void)
{
    static const int Rs[] = {1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12,  13,  15,  16,  17,   24,   31,
                             32, 33, 40, 48, 56, 63, 64, 65, 96, 127, 128, 129, 255, 256, 1000, 4096, 65535, 1 << 20};
    static const uint32_t sig[] = {0x000000, 0x000001, 0x000002, 0x400000, 0x3fffff, 0x400001, 0x7fffff, 0x7ffffe,
                                   0x200000, 0x600000, 0x555555, 0x2aaaaa, 0x555556, 0x2aaaab, 0x199999, 0x19999a,
                                   0x4ccccc, 0x4ccccd, 0x124924, 0x124925, 0x492492, 0x492493, 0x638e38, 0x638e39};
    for (size_t ri = 0; ri < sizeof(Rs) / sizeof(Rs[0]); ++ri) {
        const int R = Rs[ri];
        for (uint32_t e = 0; e < 256; ++e)
            for (size_t si = 0; si < sizeof(sig) / sizeof(sig[0]); ++si)
                for (uint32_t flag = 0; flag < 2; ++flag) check(flag << 31 | e << 23 | sig[si], R);
        for (int b = 0; b < 23; ++b) {   /* subnormals: one bit, and the run of ones below it */
            check(1u << b, R);
            check((1u << b) - 1u, R);
        }
        /* 2^j / R exactly, where R allows it (the m == 0.5 branch), and its neighbours */
        for (int j = -140; j <= 127; ++j) {
            const float x = (float)(ldexp(1.0, j) / (double)R);
            uint32_t w;
            memcpy(&w, &x, sizeof(w));
            for (int d = -2; d <= 2; ++d)
                if (w + (uint32_t)d < 0x7f800000u) check(w + (uint32_t)d, R);
        }
        uint32_t s = 0x9e3779b9u ^ (uint32_t)R;
        for (int i = 0; i < 200000; ++i) {
            s = s * 1664525u + 1013904223u;
            check(s ^ (s >> 15), R);
        }
        static const float odd[] = {-0.0f, -1.0f, -1e-45f, -3e38f, -0.75f, -INFINITY, NAN, -NAN};
        for (size_t i = 0; i < sizeof(odd) / sizeof(odd[0]); ++i) check_float(odd[i], R);
    }
    for (uint32_t e = 0; e < 256; ++e)
        for (size_t si = 0; si < sizeof(sig) / sizeof(sig[0]); ++si)
            for (uint32_t flag = 0; flag < 2; ++flag) check_r_floor(flag << 31 | e << 23 | sig[si]);
    printf("scale rule %s: %ld cases, %ld mismatches\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
