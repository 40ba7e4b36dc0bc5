// inccl_block.h -- what the per-block kernels of inccl_block.hip (32-bit lanes)
// and inccl_pack.hip (packed 16-bit lanes) share: a block's multipliers from its
// word, the clamped word lookup and the host-side launch helpers.
#ifndef INCCL_BLOCK_H
#define INCCL_BLOCK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inccl_kernels.h"
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

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int grid_cap()
{
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
            cus = v;
        else
            cus = 256;
    }
    return cus * 8;
}

inline int grid_of(int64_t items, int per_group)
{
    const int64_t g = (items + per_group - 1) / per_group, cap = grid_cap();
    return (int)(g < 1 ? 1 : (g < cap ? g : cap));
}

inline int fill_srcs(const void* const* srcs, int R, SrcPtrs* s, bool* vec)
{
    if (srcs == nullptr || R < 1 || R > kMaxR) return INCCL_ERR_ARG;
    *s = SrcPtrs{};
    for (int r = 0; r < R; ++r) {
        if (srcs[r] == nullptr) return INCCL_ERR_ARG;
        s->p[r] = srcs[r];
        *vec = *vec && aligned16(srcs[r]);
    }
    return 0;
}

#define INCCL_R_SWITCH(R, CALL) \
    switch (R) {                \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        case 4: CALL(4); break; \
        case 5: CALL(5); break; \
        case 6: CALL(6); break; \
        case 7: CALL(7); break; \
        default: CALL(8); break; \
    }

}  // namespace inccl_dev

#endif
