// inccl_pack.hip -- packed 16-bit lanes (INCCL_KIND_P16): the wire form of a
// per-block scaled fp32 bucket (INCCL_SCALE_BLOCK) at 2 bytes per element, on
// CDNA4 (gfx950).  Blocks and words are inccl_block.hip's; semantics
// (tests/block16_ref.py):
//
//   k_b   max(inccl_scale_of_word(w_b, R_total) - 16, INCCL_SCALE_MIN)
//   L     32767 / R_total
//   q     clamp(sat_i32(rne(x * 2^k_b)), -L, L), NaN -> 0
//   word  j of a bucket = q[2j + 1] * 65536 + q[2j] mod 2^32 (n odd: the last
//         word's high lane is 0); the wrap-around int32 sum of such words adds
//         both lanes at once, exactly, while each lane's sum is in [-32767, 32767]
//   lo = sign_extend16(s), hi = (s - lo) >> 16, y = (float)lane * 2^-(k_b + out_shift)
//
// Kernels:
//   k_pack_block<R>        F32 -> P16: quantise + local sum + pack.  A wave
//                          takes 512 elements = two blocks per step as two
//                          contiguous wave-wide dwordx4 loads per input; lanes
//                          pair up (one __shfl_xor) so that each stores one
//                          dwordx4; (4R + 2) n + n / 64 bytes
//   k_unpack_block<R>      P16 -> F32: sum of R packed sources + unpack +
//                          dequantise; one dwordx4 load per input, two dwordx4
//                          stores; (2R + 4) n + n / 64 bytes
//                          (a lane takes 8 consecutive elements, inside one
//                          block since elem_base % 8 == 0; lanes 0-31 and 32-63
//                          of a wave read different words)
//   k_pack_block_elem      per word (tails, elem_base % 4 != 0, unaligned pointers)
//   k_unpack_block_elem    per element; also an odd elem_base: the sources point
//                          at the word that holds element elem_base, whose low
//                          lane is then skipped
// The one-pass world-1 form is k_stream_block_fused<.., P16 = true> of inccl_block.hip.
//
// Error feedback (EF, inccl_block.h) is a compile-time switch of the two pack
// kernels: the residuals are a parameter pack RES..., empty or one ResPtrs,
// right after the sources (inccl_block.hip says why).  With EF they pack v = x + e:
//   k_pack_block<R, B, ResPtrs>     e read by the same two rows, e' written by
//                                   two dwordx4 stores per input;
//                                   (12 R + 2) n + n / 64 bytes
//   k_pack_block_elem<R, ResPtrs>   per word
// The unpack kernels have no such form.
//
// Nontemporal loads, vector stores (nontemporal for the residual quads) and
// plain C++.  Every lane of a wave reaches k_pack_block's __shfl_xor: the loop
// around it is wave-uniform.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inccl_block.h"

namespace {

using namespace inccl_dev;

__device__ __forceinline__ int32_t lane_lo(uint32_t s) { return (int32_t)(int16_t)(uint16_t)s; }
__device__ __forceinline__ int32_t lane_hi(uint32_t s) { return (int32_t)(s - (uint32_t)lane_lo(s)) >> 16; }

__device__ __forceinline__ uint32_t deq1(int32_t lane, float inv) { return __float_as_uint((float)lane * inv); }

// A wave takes 128 consecutive quads (512 elements) per step: lane l loads quads
// wb + l (row A) and wb + 64 + l (row B) of every input, two wave-wide
// contiguous 1-KiB accesses, and packs each quad into two words.  The even lane
// 2u then takes row A's words of lanes 2u, 2u + 1 and the odd lane row B's (one
// __shfl_xor of two dwords), so that every lane stores one dwordx4 and a wave's
// store covers two contiguous 512-B runs.  Quad q holds the bucket's elements
// elem_base + 4 q .. + 3, inside one block since elem_base % 4 == 0.  The loop
// is over whole waves (ntiles tiles of 128 quads): wave-uniform around the shuffles.
// EF: each lane also writes back the two residual quads it read.
template <int R, int BLOCK, class... RES>
__global__ __launch_bounds__(BLOCK) void k_pack_block(SrcPtrs src, RES... res_arg, void* __restrict__ dst,
                                                      int64_t ntiles, const uint32_t* __restrict__ words, int64_t nb,
                                                      int64_t elem_base, int scale_R, int L)
{
    constexpr bool EF = sizeof...(RES) != 0;
    const Res<EF> res = res_of(res_arg...);
    constexpr int WAVES = BLOCK / 64;
    const int lane = threadIdx.x & 63;
    u32x4* __restrict__ out = reinterpret_cast<u32x4*>(dst);
    for (int64_t t = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < ntiles; t += (int64_t)gridDim.x * WAVES) {
        const int64_t qa = (t << 7) + lane, qb = qa + 64;
        u32x4 a[R], b[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            a[r] = ld_quad<EF>(src.p[r], res, r, qa);
            b[r] = ld_quad<EF>(src.p[r], res, r, qb);
        }
        const uint32_t wa = word_at(words, (elem_base + (qa << 2)) >> 8, nb);
        const auto ma = contrib_mul<EF>(block_mul<true>(wa, scale_R, 0), wa, scale_R);
        const uint32_t wb = word_at(words, (elem_base + (qb << 2)) >> 8, nb);
        const auto mb = contrib_mul<EF>(block_mul<true>(wb, scale_R, 0), wb, scale_R);
        u32x4 sa = {0u, 0u, 0u, 0u}, sb = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            u32x4 ea, eb;
            contrib_quad<true, EF>(sa, a[r], ma, L, &ea);
            contrib_quad<true, EF>(sb, b[r], mb, L, &eb);
            st_quad<EF>(res, r, qa, ea);
            st_quad<EF>(res, r, qb, eb);
        }
        const uint32_t a0 = pack2(sa.x, sa.y), a1 = pack2(sa.z, sa.w);
        const uint32_t b0 = pack2(sb.x, sb.y), b1 = pack2(sb.z, sb.w);
        const bool odd = lane & 1;
        const uint32_t r0 = (uint32_t)__shfl_xor((int)(odd ? a0 : b0), 1, 64);
        const uint32_t r1 = (uint32_t)__shfl_xor((int)(odd ? a1 : b1), 1, 64);
        // the tile's 256 words are u32x4 [64 t, 64 t + 64): row A the first 32, row B the last
        out[(t << 6) + (odd ? 32 : 0) + (lane >> 1)] = odd ? u32x4{r0, r1, b0, b1} : u32x4{a0, a1, r0, r1};
    }
}

// words [begin, m) of the call, m = ceil(n / 2); elem_base is even, so both
// elements of a word are in one block
template <int R, class... RES>
__global__ __launch_bounds__(kBlock) void k_pack_block_elem(SrcPtrs src, RES... res_arg, void* __restrict__ dst,
                                                            int64_t begin, int64_t n,
                                                            const uint32_t* __restrict__ words, int64_t nb,
                                                            int64_t elem_base, int scale_R, int L)
{
    constexpr bool EF = sizeof...(RES) != 0;
    const Res<EF> res = res_of(res_arg...);
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(dst);
    const int64_t m = (n + 1) >> 1;
    for (int64_t j = begin + (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (int64_t)gridDim.x * kBlock) {
        const uint32_t w = word_at(words, (elem_base + 2 * j) >> 8, nb);
        const auto mul = contrib_mul<EF>(block_mul<true>(w, scale_R, 0), w, scale_R);
        const bool pair = 2 * j + 1 < n;
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            uint32_t e;
            lo += contrib<true, EF>(ld1<EF>(src.p[r], res, r, 2 * j), mul, L, &e);
            st1<EF>(res, r, 2 * j, e);
            if (pair) {
                hi += contrib<true, EF>(ld1<EF>(src.p[r], res, r, 2 * j + 1), mul, L, &e);
                st1<EF>(res, r, 2 * j + 1, e);
            }
        }
        out[j] = pack2(lo, hi);
    }
}

template <int R, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_unpack_block(SrcPtrs src, void* __restrict__ dst, int64_t n8,
                                                        const uint32_t* __restrict__ words, int64_t nb,
                                                        int64_t elem_base, int scale_R, int out_shift)
{
    u32x4* __restrict__ out = reinterpret_cast<u32x4*>(dst);
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n8; i += (int64_t)gridDim.x * BLOCK) {
        u32x4 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src.p[r]) + i);
        const float inv = block_mul<true>(word_at(words, (elem_base + (i << 3)) >> 8, nb), scale_R, out_shift).inv;
        u32x4 s = v[0];
#pragma unroll
        for (int r = 1; r < R; ++r) s += v[r];
        out[2 * i] = u32x4{deq1(lane_lo(s.x), inv), deq1(lane_hi(s.x), inv), deq1(lane_lo(s.y), inv),
                           deq1(lane_hi(s.y), inv)};
        out[2 * i + 1] = u32x4{deq1(lane_lo(s.z), inv), deq1(lane_hi(s.z), inv), deq1(lane_lo(s.w), inv),
                               deq1(lane_hi(s.w), inv)};
    }
}

// elements [begin, n) of the call; element i is lane (odd + i) & 1 of the
// sources' word (odd + i) >> 1, odd = elem_base & 1
template <int R>
__global__ __launch_bounds__(kBlock) void k_unpack_block_elem(SrcPtrs src, void* __restrict__ dst, int64_t begin,
                                                              int64_t n, const uint32_t* __restrict__ words,
                                                              int64_t nb, int64_t elem_base, int scale_R,
                                                              int out_shift)
{
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(dst);
    const int64_t odd = elem_base & 1;
    for (int64_t i = begin + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const float inv = block_mul<true>(word_at(words, (elem_base + i) >> 8, nb), scale_R, out_shift).inv;
        const int64_t p = odd + i;
        uint32_t s = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) s += reinterpret_cast<const uint32_t*>(src.p[r])[p >> 1];
        out[i] = deq1((p & 1) ? lane_hi(s) : lane_lo(s), inv);
    }
}

// e: the residuals (error feedback) or NULL
template <int R>
void launch_pack(const SrcPtrs& s, const ResPtrs* e, void* dst, int64_t n, const uint32_t* words, int64_t nb,
                 int64_t elem_base, int scale_R, bool vec, hipStream_t st)
{
    constexpr int B = 512;
    const int L = inccl_p16_clamp(scale_R);
    const int64_t m = (n + 1) >> 1;
    int64_t done = 0;   // words
    if (vec && (elem_base & 3) == 0) {
        const int64_t ntiles = n >> 9;   // whole waves of 512 elements
        const dim3 grid(grid_of(ntiles, B / 64, 8));
        if (ntiles > 0 && e)
            hipLaunchKernelGGL((k_pack_block<R, B, ResPtrs>), grid, dim3(B), 0, st, s, *e, dst, ntiles, words, nb, elem_base,
                               scale_R, L);
        else if (ntiles > 0)
            hipLaunchKernelGGL((k_pack_block<R, B>), grid, dim3(B), 0, st, s, dst, ntiles, words, nb, elem_base, scale_R,
                               L);
        done = ntiles << 8;
    }
    if (done < m) {
        const dim3 grid(grid_of(m - done, kBlock, 8));
        if (e)
            hipLaunchKernelGGL((k_pack_block_elem<R, ResPtrs>), grid, dim3(kBlock), 0, st, s, *e, dst, done, n, words, nb,
                               elem_base, scale_R, L);
        else
            hipLaunchKernelGGL((k_pack_block_elem<R>), grid, dim3(kBlock), 0, st, s, dst, done, n, words, nb, elem_base,
                               scale_R, L);
    }
}

template <int R>
void launch_unpack(const SrcPtrs& s, void* dst, int64_t n, const uint32_t* words, int64_t nb, int64_t elem_base,
                   int scale_R, int out_shift, bool vec, hipStream_t st)
{
    constexpr int B = 512;
    int64_t done = 0;   // elements
    if (vec && (elem_base & 7) == 0) {
        const int64_t n8 = n >> 3;
        if (n8 > 0)
            hipLaunchKernelGGL((k_unpack_block<R, B>), dim3(grid_of(n8, B, 8)), dim3(B), 0, st, s, dst, n8, words, nb,
                               elem_base, scale_R, out_shift);
        done = n8 << 3;
    }
    if (done < n)
        hipLaunchKernelGGL((k_unpack_block_elem<R>), dim3(grid_of(n - done, kBlock, 8)), dim3(kBlock), 0, st, s, dst,
                           done, n, words, nb, elem_base, scale_R, out_shift);
}

}  // namespace

extern "C" {

int inccl_k_stream_block16(int in_kind, int out_kind, const void* const* srcs, float* const* res, int R, void* dst,
                           size_t n, const uint32_t* words_dev, size_t nb, size_t elem_base, int scale_R,
                           int out_shift, void* stream)
{
    SrcPtrs s;
    ResPtrs e;
    bool vec = aligned16(dst);
    const bool pack = in_kind == F32 && out_kind == P16, unpack = in_kind == P16 && out_kind == F32;
    if (fill_srcs(srcs, R, &s, &vec) || (res != nullptr && (!pack || fill_srcs(res, R, &e, &vec))) ||
        (!pack && !unpack) || (dst == nullptr && n > 0) || out_shift < 0 || out_shift > 8 ||
        ((words_dev == nullptr || nb == 0) && n > 0) || (pack && (elem_base & 1)))
        return INCCL_ERR_ARG;
    if (scale_R <= 0) scale_R = R;
    if (scale_R > INCCL_P16_LANE_MAX) return INCCL_ERR_ARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define INCCL_CALL(RR)                                                                                             \
    if (pack)                                                                                                      \
        launch_pack<RR>(s, res ? &e : nullptr, dst, (int64_t)n, words_dev, (int64_t)nb, (int64_t)elem_base, scale_R, \
                        vec, st);                                                                                  \
    else launch_unpack<RR>(s, dst, (int64_t)n, words_dev, (int64_t)nb, (int64_t)elem_base, scale_R, out_shift, vec, st)
    INCCL_R_SWITCH(R, INCCL_CALL)
#undef INCCL_CALL
    return (int)hipGetLastError();
}

}  // extern "C"
