// inccl_block.h -- what the per-block kernels of inccl_block.hip (32-bit lanes)
// and inccl_pack.hip (packed 16-bit lanes) share: a block's multipliers from its
// word, a contribution's quantise-and-clamp, the clamped word lookup and what
// error feedback (EF) adds to a kernel of the packed lanes.
//
// Error feedback (tests/block16_ef_ref.py): every local bucket r has an fp32
// residual e_r, the part of its last contribution the 16-bit lane could not
// carry; it is added to this call's contribution and rewritten.
//
//   v     fl32(x + e)                     one IEEE add, denormals kept
//   w_b   the absmax word of block b over every v (NF: a NaN or +-Inf in v sets bit 31)
//   q     clamp(sat_i32(rne(v * 2^k_b)), -L, L), NaN -> 0   (the P16 rule on v)
//   d     fl32(v - (float)q * 2^-k_b)     the product is exact (|q| <= 2^15), so an
//                                         fma gives the same bits; no out_shift
//   e'    d if finite, else 0; 0 for every element of a block whose word has bit 31
//
// A kernel with EF differs from the one without in three places, the helpers
// below: the load (ld_quad, ld1), the contribution (contrib, contrib_quad) and
// the residual store (st_quad, st1).  A lane reads and writes the same elements
// of a residual and nothing else of it, so a residual is updated in place (its
// pointers are not __restrict__); x and e are summed into v as they land, the
// kernel never holds both.
#ifndef INCCL_BLOCK_H
#define INCCL_BLOCK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "inccl_launch.h"
#include "inccl_scale_rule.h"
#include "inccl_stream.h"

namespace inccl_dev {

constexpr int kBlkWaves = kBlock / 64;   // waves = blocks per workgroup and step of the per-block kernels

// the residuals of the R buckets; a kernel body without error feedback takes NoRes
struct ResPtrs {
    float* p[kMaxR];
};
struct NoRes {};
template <bool EF>
using Res = std::conditional_t<EF, ResPtrs, NoRes>;
__device__ __forceinline__ NoRes res_of() { return {}; }
__device__ __forceinline__ const ResPtrs& res_of(const ResPtrs& r) { return r; }

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

// EF: what a contribution and its residual take of the block's word: 2^k_b of
// the packed lanes to quantise, 2^-k_b for the residual (never NaN, no
// out_shift) and whether the word carries bit 31 (the residual is dropped)
struct EfMul {
    float scale, rinv;
    bool drop;
};
__device__ __forceinline__ EfMul ef_mul(uint32_t word, int scale_R)
{
    const int k = inccl_p16_scale_of_word(word, scale_R);
    return EfMul{pow2f(k), pow2f(-k), (word >> 31) != 0};
}
// the multipliers of a contribution: the block's without EF, ef_mul of its word
// with EF.  That resolves the exponent from the word once more, as the kernels
// with feedback always did: one exponent for both makes block_mul's NaN select
// a per-lane one, 2 more VGPRs in most fused kernels (profiles/block_kernel_fold/)
template <bool EF>
__device__ __forceinline__ std::conditional_t<EF, EfMul, BlockMul> contrib_mul(const BlockMul& bm, uint32_t word,
                                                                               int scale_R)
{
    if constexpr (EF) return ef_mul(word, scale_R);
    else return bm;
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

// the contribution q of v (returned); EF: *e = the residual v - q * 2^-k_b it
// leaves, 0 where that is not finite or the block is flagged (untouched otherwise)
template <bool P16, bool EF, class MUL>
__device__ __forceinline__ uint32_t contrib(uint32_t v, const MUL& m, int L, uint32_t* e)
{
    const uint32_t q = quantb<P16>(__uint_as_float(v), m.scale, L);
    if constexpr (EF) {
        const uint32_t d = __float_as_uint(__uint_as_float(v) - (float)(int32_t)q * m.rinv);
        *e = (m.drop || (d & 0x7f800000u) == 0x7f800000u) ? 0u : d;
    }
    return q;
}
template <bool P16, bool EF, class MUL>
__device__ __forceinline__ void contrib_quad(u32x4& acc, u32x4 v, const MUL& m, int L, u32x4* e)
{
    uint32_t ex, ey, ez, ew;
    acc.x += contrib<P16, EF>(v.x, m, L, &ex);
    acc.y += contrib<P16, EF>(v.y, m, L, &ey);
    acc.z += contrib<P16, EF>(v.z, m, L, &ez);
    acc.w += contrib<P16, EF>(v.w, m, L, &ew);
    if constexpr (EF) *e = u32x4{ex, ey, ez, ew};
}

// v of bucket r (src = its pointer): quad i (nontemporal) or element i; EF:
// fl32(x + e) on raw bits
__device__ __forceinline__ uint32_t add1(uint32_t x, uint32_t e)
{
    return __float_as_uint(__uint_as_float(x) + __uint_as_float(e));
}
template <bool EF>
__device__ __forceinline__ u32x4 ld_quad(const void* src, const Res<EF>& res, int r, int64_t i)
{
    const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src) + i);
    if constexpr (EF) {
        const u32x4 e = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(res.p[r]) + i);
        return u32x4{add1(x.x, e.x), add1(x.y, e.y), add1(x.z, e.z), add1(x.w, e.w)};
    } else {
        return x;
    }
}
template <bool EF>
__device__ __forceinline__ uint32_t ld1(const void* src, const Res<EF>& res, int r, int64_t i)
{
    const uint32_t x = reinterpret_cast<const uint32_t*>(src)[i];
    if constexpr (EF) return add1(x, reinterpret_cast<const uint32_t*>(res.p[r])[i]);
    else return x;
}

// EF: the residual of bucket r back to where it was read.  A quad goes
// nontemporal: a plain store leaves the line dirty in L2 beside the streamed
// inputs, and at R = 2 x 256 MiB the pack kernel then took 334-336 us against
// 287-293 and the fused one 344 against 279-283 (tools/ef_bench.py, alternating
// runs, profiles/pack16_ef/)
template <bool EF>
__device__ __forceinline__ void st_quad(const Res<EF>& res, int r, int64_t i, const u32x4& e)
{
    if constexpr (EF) __builtin_nontemporal_store(e, reinterpret_cast<u32x4*>(res.p[r]) + i);
}
template <bool EF>
__device__ __forceinline__ void st1(const Res<EF>& res, int r, int64_t i, const uint32_t& e)
{
    if constexpr (EF) reinterpret_cast<uint32_t*>(res.p[r])[i] = e;
}

// two 16-bit lanes in one wire word
__device__ __forceinline__ uint32_t pack2(uint32_t lo, uint32_t hi) { return hi * 65536u + lo; }

// the word of the bucket's block `blk`, clamped to the words the caller holds
__device__ __forceinline__ uint32_t word_at(const uint32_t* __restrict__ words, int64_t blk, int64_t nb)
{
    return words[blk < nb ? blk : nb - 1];
}

}  // namespace inccl_dev

#endif
