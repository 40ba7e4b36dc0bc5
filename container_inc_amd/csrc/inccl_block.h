// inccl_block.h -- what the per-block kernels of inccl_block.hip (32-bit lanes),
// inccl_pack.hip (packed 16-bit lanes) and inccl_ef.hip (those with error
// feedback) share: a block's multipliers from its
// word, a contribution's quantise-and-clamp and the clamped word lookup.
#ifndef INCCL_BLOCK_H
#define INCCL_BLOCK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inccl_launch.h"
#include "inccl_scale_rule.h"
#include "inccl_stream.h"

namespace inccl_dev {

// one block's multipliers from its word: 2^k_b to quantise, 2^-(k_b + out_shift)
// to dequantise -- NaN when the word carries bit 31 (that block's results are NaN).
// P16: the exponent of a packed 16-bit lane (inccl_p16_scale_of_word).
struct BlockMul {
    float scale, inv;
};
template <bool P16 = false>
__device__ __forceinline__ BlockMul block_mul(uint32_t word, int scale_R, int out_shift)
{
    int k;
    if constexpr (P16) k = inccl_p16_scale_of_word(word, scale_R);
    else k = inccl_scale_of_word(word, scale_R);
    BlockMul b;
    b.scale = pow2f(k);
    b.inv = (word >> 31) ? __builtin_nanf("") : pow2f(-k - out_shift);
    return b;
}

// one contribution: sat_i32(rne(x * scale)), NaN -> 0; P16: clamped to [-L, L],
// so that the sum of scale_R contributions stays inside a 16-bit lane
template <bool P16>
__device__ __forceinline__ uint32_t quantb(float x, float scale, int L)
{
    const uint32_t q = quant1(x, scale);
    if constexpr (P16) {
        const int32_t v = (int32_t)q;
        return (uint32_t)(v < -L ? -L : (v > L ? L : v));
    } else {
        return q;
    }
}

// the word of the bucket's block `blk`, clamped to the words the caller holds
__device__ __forceinline__ uint32_t word_at(const uint32_t* __restrict__ words, int64_t blk, int64_t nb)
{
    return words[blk < nb ? blk : nb - 1];
}

}  // namespace inccl_dev

#endif
