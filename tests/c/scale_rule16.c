/* scale_rule16.c -- the exponent and the clamp of packed 16-bit lanes
 * (csrc/inccl_scale_rule.h inccl_p16_scale_of_word, inccl_p16_clamp) against the
 * spec written on the oracle's rule: k = max(orc_choose_scale(amax, R) - 16,
 * INCCL_SCALE_MIN), a zero block 48, L = 32767 / R with R * L <= 32767 <
 * R * (L + 1); and where neither clamp of the exponent bound, the largest
 * contribution rne(amax * 2^k) is at most ceil(2^14 / R) <= L, so the lane
 * clamp binds on no finite element.  The words and the R values are those of
 * scale_rule.c.  Host code only:
 *   gcc -std=gnu11 -I include -I container_inc_amd/csrc -I oracle tests/c/scale_rule16.c oracle/inccl_oracle.c -lm */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "inccl_oracle.h"
#include "inccl_scale_rule.h"

static long cases, bad;

static void fail(const char *what, uint32_t word, int R, long got, long want)
{
    if (++bad <= 20) printf("MISMATCH %s word %08x R %d: %ld, expected %ld\n", what, word, R, got, want);
}

static void check(uint32_t word, int R)
{
    const uint32_t bits = word & 0x7fffffffu;
    float amax;
    memcpy(&amax, &bits, sizeof(amax));
    const int K = orc_choose_scale(amax, R);
    const int want = K - 16 < INCCL_SCALE_MIN ? INCCL_SCALE_MIN : K - 16, got = inccl_p16_scale_of_word(word, R);
    ++cases;
    if (want != got) fail("k", word, R, got, want);
    if (got < INCCL_SCALE_MIN || got > INCCL_SCALE_MAX - 16) fail("k range", word, R, got, INCCL_SCALE_MAX - 16);
    if (bits == 0u && got != 48) fail("zero block", word, R, got, 48);
    if (R > INCCL_P16_LANE_MAX || !(amax <= 3.4028234663852886e38f) || K == INCCL_SCALE_MIN) return;
    /* neither exponent clamp bound (K > -64 is the rule's own value or INCCL_SCALE_MAX;
     * K - 16 >= -64 is checked): the largest contribution fits the lane's share */
    if (K - 16 < INCCL_SCALE_MIN) return;
    const long q = (long)rint(ldexp((double)amax, got)), cap = (16384 + R - 1) / R, L = inccl_p16_clamp(R);
    if (q > cap) fail("largest contribution", word, R, q, cap);
    if (cap > L) fail("ceil(2^14 / R) against L", word, R, cap, L);
}

int main(void)
{
    static const int Rs[] = {1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12,  13,  15,  16,  17,   24,   31,
                             32, 33, 40, 48, 56, 63, 64, 65, 96, 127, 128, 129, 255, 256, 1000, 4096, 65535, 1 << 20};
    static const uint32_t sig[] = {0x000000, 0x000001, 0x000002, 0x400000, 0x3fffff, 0x400001, 0x7fffff, 0x7ffffe,
                                   0x200000, 0x600000, 0x555555, 0x2aaaaa, 0x555556, 0x2aaaab, 0x199999, 0x19999a,
                                   0x4ccccc, 0x4ccccd, 0x124924, 0x124925, 0x492492, 0x492493, 0x638e38, 0x638e39};
    /* L: every R a lane can serve, and the first it cannot */
    for (int R = 1; R <= INCCL_P16_LANE_MAX + 1; ++R) {
        const long L = inccl_p16_clamp(R);
        ++cases;
        if (L != INCCL_P16_LANE_MAX / R || L * R > INCCL_P16_LANE_MAX || (L + 1) * R <= INCCL_P16_LANE_MAX)
            fail("L", 0, R, L, INCCL_P16_LANE_MAX / R);
        if ((R <= INCCL_P16_LANE_MAX) != (L >= 1)) fail("L >= 1", 0, R, L, 1);
    }
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
    }
    printf("scale rule 16 %s: %ld cases, %ld mismatches\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
