// inccl_block.hip -- per-block auto scaling (INCCL_SCALE_BLOCK) for fp32 buckets
// on CDNA4 (gfx950).  One block is INCCL_BLOCK_ELEMS = 256 elements of the
// bucket: lane t of a wave64 loads quad base + t, so one wave-wide dwordx4
// access is one block when the base is a multiple of 64 quads.  Semantics
// (tests/block_ref.py):
//
//   w_b   bits of max |x| over block b of every bucket of every rank (NaN
//         ignored; with the non-finite flag a NaN or +-Inf sets bit 31)
//   k_b   the auto scale rule on w_b (inccl_scale_of_word of inccl_scale_rule.h,
//         a dozen integer ops; bit 31 of w_b is ignored for the exponent)
//   q = sat_i32(rne(x * 2^k_b)),  s = sum q mod 2^32,  y = (float)s * 2^-(k_b + out_shift)
//
// Kernels:
//   k_stream_block_fused<R>      world 1, one HBM pass: the wave reduces its
//                                block's absmax (six __shfl_xor steps), resolves
//                                k_b and quantises + sums + dequantises the
//                                quads it already holds; (R + 1) * 4 * n bytes
//                                (+ n / 64 when the words are written out)
//   k_block_fused_elem<R>        the same on buckets that are not 16-B aligned
//                                (both with P16: the exponent and the clamp of
//                                packed 16-bit lanes, inccl_pack.hip, so that
//                                world 1 gives what N ranks would give)
//   k_block_absmax<R, NF>        the words of R local buckets: one wave per block
//                                and step, plain stores, overwrites
//   k_stream_block<IN, OUT, R>   F32 -> Q32 (quantise + local sum) and Q32 -> F32
//                                (sum + dequantise) at the agreed words; element i
//                                of the call is element elem_base + i of the bucket
//   k_stream_block_elem          the same per element (tails, elem_base % 4 != 0,
//                                pointers not 16-B aligned)
//   k_words_max                  element-wise unsigned max of W rows of words
//
// Error feedback (EF, inccl_block.h) is a compile-time switch of the packed
// lanes' kernels, not a copy of them: k_stream_block_fused, k_block_fused_elem
// (both with P16 only) and k_block_absmax take the residuals as a parameter
// pack RES..., empty or one ResPtrs, right after the sources.  An empty pack
// leaves the kernel's arguments as they are without EF; a parameter of an
// empty type would take a slot and move every later one.  With EF they work on
// v = x + e:
//   k_block_absmax<R, NF, ResPtrs>              the words of v, the residuals
//                                               only read; 8 R n bytes
//   k_stream_block_fused<R, NF, true, ResPtrs>  plus e', (12 R + 4) n bytes; the
//                                               flagged-block rule uses the word
//                                               the wave computed
//   k_block_fused_elem<R, NF, true, ResPtrs>    the same per element
//
// Nontemporal loads of quads, vector stores (nontemporal for the residual
// quads) and plain C++.  Every lane of a wave reaches every __shfl_xor: the
// loops and branches around them are wave-uniform.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inccl_block.h"

namespace {

using namespace inccl_dev;

// EF: every lane also writes the residual quads (and tail elements) it read
template <int R, bool NF, bool P16, int BLOCK, int U, class... RES>
__global__ __launch_bounds__(BLOCK) void k_stream_block_fused(SrcPtrs src, RES... res_arg, void* __restrict__ dst,
                                                              int64_t n, uint32_t* __restrict__ words, int scale_R,
                                                              int out_shift)
{
    constexpr bool EF = sizeof...(RES) != 0;
    const Res<EF> res = res_of(res_arg...);
    static_assert(P16 || !EF, "error feedback belongs to the packed 16-bit lanes");
    const int64_t n4 = n >> 2;
    const int tail = (int)(n & 3);                    // elements after the last quad: lane i == n4 takes them
    const int64_t nq = ((n + 255) >> 8) << 6;         // quads of whole blocks: a wave for every block
    const int64_t tile = (int64_t)BLOCK * U;
    const int lane = threadIdx.x & 63;
    const int L = P16 ? inccl_p16_clamp(scale_R) : 0;   // the packed lanes' clamp, unused otherwise
    u32x4* __restrict__ out = reinterpret_cast<u32x4*>(dst);
    uint32_t* __restrict__ out1 = reinterpret_cast<uint32_t*>(dst);

    for (int64_t base = (int64_t)blockIdx.x * tile; base < nq; base += (int64_t)gridDim.x * tile) {
        const bool full = base + tile <= n4;
        // every load of the tile in flight before the first compare
        u32x4 v[R][U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = base + threadIdx.x + (int64_t)u * BLOCK;
#pragma unroll
            for (int r = 0; r < R; ++r) v[r][u] = (full || i < n4) ? ld_quad<EF>(src.p[r], res, r, i) : u32x4{0u, 0u, 0u, 0u};
        }
        __amdgpu_buffer_rsrc_t orsrc;
        if (full) orsrc = __builtin_amdgcn_make_buffer_rsrc(out + base, 0, (int)(tile * 16), 0x00020000);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = base + threadIdx.x + (int64_t)u * BLOCK;
            if (i - lane >= nq) continue;             // wave-uniform: this wave's block is past the bucket
            uint32_t m = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t a = amax_quad<NF>(v[r][u]);
                m = m > a ? m : a;
            }
            const bool tl = tail != 0 && i == n4;
            uint32_t t[R][3];
            if (tl) {
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        t[r][j] = j < tail ? ld1<EF>(src.p[r], res, r, n4 * 4 + j) : 0u;
                        const uint32_t a = abs_bits<NF>(t[r][j]);
                        m = m > a ? m : a;
                    }
            }
            // the block's word, wave-uniform: the exponent is resolved once per wave
            const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(m));
            const BlockMul bm = block_mul<P16>(w, scale_R, out_shift);
            const auto cm = contrib_mul<EF>(bm, w, scale_R);
            if (words != nullptr && lane == 0) words[i >> 6] = w;
            u32x4 acc = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int r = 0; r < R; ++r) {
                u32x4 e;
                contrib_quad<P16, EF>(acc, v[r][u], cm, L, &e);
                if (full || i < n4) st_quad<EF>(res, r, i, e);
            }
            const u32x4 o = xform_quad<F32>(acc, bm.inv);
            if (full)
                __builtin_amdgcn_raw_buffer_store_b128(o, orsrc, (int)((threadIdx.x + u * BLOCK) * 16), 0, kAuxSc1);
            else if (i < n4)
                out[i] = o;
            if (tl) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (j < tail) {
                        uint32_t a = 0;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            uint32_t e;
                            a += contrib<P16, EF>(t[r][j], cm, L, &e);
                            st1<EF>(res, r, n4 * 4 + j, e);
                        }
                        out1[n4 * 4 + j] = store_xform<F32>(a, bm.inv);
                    }
            }
        }
    }
}

// the fused kernel per element: lane t of the block's wave takes elements
// 256 b + t + 64 j, j < 4 (coalesced dword accesses)
template <int R, bool NF, bool P16, class... RES>
__global__ __launch_bounds__(kBlock) void k_block_fused_elem(SrcPtrs src, RES... res_arg, void* __restrict__ dst,
                                                             int64_t n, uint32_t* __restrict__ words, int scale_R,
                                                             int out_shift)
{
    constexpr bool EF = sizeof...(RES) != 0;
    const Res<EF> res = res_of(res_arg...);
    static_assert(P16 || !EF, "error feedback belongs to the packed 16-bit lanes");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nb = (n + 255) >> 8;
    const int L = P16 ? inccl_p16_clamp(scale_R) : 0;
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(dst);
    for (int64_t b = (int64_t)blockIdx.x * kBlkWaves + wave; b < nb; b += (int64_t)gridDim.x * kBlkWaves) {
        uint32_t x[R][4];
        uint32_t m = 0;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t e = (b << 8) + j * 64 + lane;
                x[r][j] = e < n ? ld1<EF>(src.p[r], res, r, e) : 0u;
            }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t a = abs_bits<NF>(x[r][j]);
                m = m > a ? m : a;
            }
        const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(m));
        const BlockMul bm = block_mul<P16>(w, scale_R, out_shift);
        const auto cm = contrib_mul<EF>(bm, w, scale_R);
        if (words != nullptr && lane == 0) words[b] = w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t e = (b << 8) + j * 64 + lane;
            if (e < n) {
                uint32_t a = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    uint32_t d;
                    a += contrib<P16, EF>(x[r][j], cm, L, &d);
                    st1<EF>(res, r, e, d);
                }
                out[e] = store_xform<F32>(a, bm.inv);
            }
        }
    }
}

// words[b] = max |v| bits over block b of the R buckets; vec: every pointer is
// 16-B aligned.  EF: the residuals are only read
template <int R, bool NF, class... RES>
__global__ __launch_bounds__(kBlock) void k_block_absmax(SrcPtrs src, RES... res_arg, int64_t n,
                                                         uint32_t* __restrict__ words, int vec)
{
    constexpr bool EF = sizeof...(RES) != 0;
    const Res<EF> res = res_of(res_arg...);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nb = (n + 255) >> 8, n4 = n >> 2;
    const int tail = (int)(n & 3);
    for (int64_t b = (int64_t)blockIdx.x * kBlkWaves + wave; b < nb; b += (int64_t)gridDim.x * kBlkWaves) {
        uint32_t m = 0;
        if (vec) {
            const int64_t i = (b << 6) + lane;
            if (i < n4) {
                u32x4 v[R];
#pragma unroll
                for (int r = 0; r < R; ++r) v[r] = ld_quad<EF>(src.p[r], res, r, i);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t a = amax_quad<NF>(v[r]);
                    m = m > a ? m : a;
                }
            } else if (i == n4) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    for (int j = 0; j < tail; ++j) {
                        const uint32_t a = abs_bits<NF>(ld1<EF>(src.p[r], res, r, n4 * 4 + j));
                        m = m > a ? m : a;
                    }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t e = (b << 8) + j * 64 + lane;
                    const uint32_t a = e < n ? abs_bits<NF>(ld1<EF>(src.p[r], res, r, e)) : 0u;
                    m = m > a ? m : a;
                }
        }
        m = wave_max_u32(m);
        if (lane == 0) words[b] = m;
    }
}

// out = OUT(sum_r IN(src_r)) over quads, <F32, Q32> or <Q32, F32>; quad i holds
// the bucket's elements elem_base + 4 i .. + 3, inside one block since
// elem_base % 4 == 0
template <int IN, int OUT, int R, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_stream_block(SrcPtrs src, void* __restrict__ dst, int64_t n4,
                                                        const uint32_t* __restrict__ words, int64_t nb,
                                                        int64_t elem_base, int scale_R, int out_shift)
{
    u32x4* __restrict__ out = reinterpret_cast<u32x4*>(dst);
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n4; i += (int64_t)gridDim.x * BLOCK) {
        u32x4 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src.p[r]) + i);
        const BlockMul bm = block_mul(word_at(words, (elem_base + (i << 2)) >> 8, nb), scale_R, out_shift);
        u32x4 acc = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < R; ++r) accum_quad<IN>(acc, v[r], bm.scale);
        out[i] = xform_quad<OUT>(acc, bm.inv);
    }
}

template <int IN, int OUT, int R>
__global__ __launch_bounds__(kBlock) void k_stream_block_elem(SrcPtrs src, void* __restrict__ dst, int64_t begin,
                                                              int64_t n, const uint32_t* __restrict__ words,
                                                              int64_t nb, int64_t elem_base, int scale_R,
                                                              int out_shift)
{
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(dst);
    for (int64_t i = begin + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const BlockMul bm = block_mul(word_at(words, (elem_base + i) >> 8, nb), scale_R, out_shift);
        uint32_t acc = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) acc += load_xform<IN>(reinterpret_cast<const uint32_t*>(src.p[r])[i], bm.scale);
        out[i] = store_xform<OUT>(acc, bm.inv);
    }
}

// out[b] = max_j rows[j * nb + b]
__global__ __launch_bounds__(kBlock) void k_words_max(const uint32_t* __restrict__ rows, int W, int64_t nb,
                                                      uint32_t* __restrict__ out)
{
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < nb; b += (int64_t)gridDim.x * kBlock) {
        uint32_t m = 0;
        for (int j = 0; j < W; ++j) {
            const uint32_t w = rows[(int64_t)j * nb + b];
            m = m > w ? m : w;
        }
        out[b] = m;
    }
}

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------
// e: the residuals or NULL; they imply the packed lanes (the shim refuses them otherwise)
template <int R, bool NF, bool P16>
void launch_fused(const SrcPtrs& s, const ResPtrs* e, void* dst, int64_t n, uint32_t* words, int scale_R,
                  int out_shift, bool vec, hipStream_t st)
{
    const int64_t nb = (n + 255) >> 8;
    if (vec) {
        constexpr int B = Geometry<R>::BLOCK, U = Geometry<R>::U;
        // one workgroup per tile, as the single-scale fused kernel
        const dim3 grid(grid_capped(nb * 64, B * U, kNoCap));
        if (e)
            hipLaunchKernelGGL((k_stream_block_fused<R, NF, true, B, U, ResPtrs>), grid, dim3(B), 0, st, s, *e, dst, n,
                               words, scale_R, out_shift);
        else
            hipLaunchKernelGGL((k_stream_block_fused<R, NF, P16, B, U>), grid, dim3(B), 0, st, s, dst, n, words, scale_R,
                               out_shift);
    } else {
        const dim3 grid(grid_of(nb, kBlkWaves, 8));
        if (e)
            hipLaunchKernelGGL((k_block_fused_elem<R, NF, true, ResPtrs>), grid, dim3(kBlock), 0, st, s, *e, dst, n, words,
                               scale_R, out_shift);
        else
            hipLaunchKernelGGL((k_block_fused_elem<R, NF, P16>), grid, dim3(kBlock), 0, st, s, dst, n, words, scale_R,
                               out_shift);
    }
}

template <int R, bool NF>
void launch_absmax(const SrcPtrs& s, const ResPtrs* e, int64_t n, uint32_t* words, bool vec, hipStream_t st)
{
    const dim3 grid(grid_of((n + 255) >> 8, kBlkWaves, 8));
    if (e) hipLaunchKernelGGL((k_block_absmax<R, NF, ResPtrs>), grid, dim3(kBlock), 0, st, s, *e, n, words, vec ? 1 : 0);
    else hipLaunchKernelGGL((k_block_absmax<R, NF>), grid, dim3(kBlock), 0, st, s, n, words, vec ? 1 : 0);
}

template <int IN, int OUT, int R>
void launch_stream(const SrcPtrs& s, void* dst, int64_t n, const uint32_t* words, int64_t nb, int64_t elem_base,
                   int scale_R, int out_shift, bool vec, hipStream_t st)
{
    constexpr int B = 512;
    int64_t done = 0;
    if (vec && (elem_base & 3) == 0) {
        const int64_t n4 = n >> 2;
        if (n4 > 0)
            hipLaunchKernelGGL((k_stream_block<IN, OUT, R, B>), dim3(grid_of(n4, B, 8)), dim3(B), 0, st, s, dst, n4, words,
                               nb, elem_base, scale_R, out_shift);
        done = n4 << 2;
    }
    if (done < n)
        hipLaunchKernelGGL((k_stream_block_elem<IN, OUT, R>), dim3(grid_of(n - done, kBlock, 8)), dim3(kBlock), 0, st, s,
                           dst, done, n, words, nb, elem_base, scale_R, out_shift);
}

}  // namespace

extern "C" {

int inccl_k_block_absmax(const void* const* srcs, const float* const* res, int R, size_t n, uint32_t* words_dev,
                         int flags, void* stream)
{
    SrcPtrs s;
    ResPtrs e;   // only read here
    bool vec = true;
    if (fill_srcs(srcs, R, &s, &vec) || (res != nullptr && fill_srcs(const_cast<float* const*>(res), R, &e, &vec)) ||
        (flags & ~INCCL_ABSMAX_FLAG_NONFINITE) || (words_dev == nullptr && n > 0))
        return INCCL_ERR_ARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define INCCL_CALL(RR)                                                                            \
    if (flags) launch_absmax<RR, true>(s, res ? &e : nullptr, (int64_t)n, words_dev, vec, st);    \
    else launch_absmax<RR, false>(s, res ? &e : nullptr, (int64_t)n, words_dev, vec, st)
    INCCL_R_SWITCH(R, INCCL_CALL)
#undef INCCL_CALL
    return (int)hipGetLastError();
}

int inccl_k_block_fused(const void* const* srcs, float* const* res, int R, void* dst, size_t n,
                        uint32_t* words_out_dev, int flags, int scale_R, int out_shift, int p16, void* stream)
{
    SrcPtrs s;
    ResPtrs e;
    bool vec = aligned16(dst);
    if (fill_srcs(srcs, R, &s, &vec) || (res != nullptr && (!p16 || fill_srcs(res, R, &e, &vec))) ||
        (flags & ~INCCL_ABSMAX_FLAG_NONFINITE) || (dst == nullptr && n > 0) || out_shift < 0 || out_shift > 8)
        return INCCL_ERR_ARG;
    if (scale_R <= 0) scale_R = R;
    if (p16 && scale_R > INCCL_P16_LANE_MAX) return INCCL_ERR_ARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define INCCL_FUSED(RR, NF, P)                                                                            \
    launch_fused<RR, NF, P>(s, res ? &e : nullptr, dst, (int64_t)n, words_out_dev, scale_R, out_shift, vec, st)
#define INCCL_CALL(RR)                                                                                    \
    if (p16) {                                                                                            \
        if (flags) INCCL_FUSED(RR, true, true);                                                           \
        else INCCL_FUSED(RR, false, true);                                                                \
    } else if (flags) INCCL_FUSED(RR, true, false);                                                       \
    else INCCL_FUSED(RR, false, false)
    INCCL_R_SWITCH(R, INCCL_CALL)
#undef INCCL_CALL
#undef INCCL_FUSED
    return (int)hipGetLastError();
}

int inccl_k_stream_block(int in_kind, int out_kind, const void* const* srcs, int R, void* dst, size_t n,
                         const uint32_t* words_dev, size_t nb, size_t elem_base, int scale_R, int out_shift,
                         void* stream)
{
    if (in_kind == P16 || out_kind == P16)   // packed 16-bit lanes: inccl_pack.hip
        return inccl_k_stream_block16(in_kind, out_kind, srcs, nullptr, R, dst, n, words_dev, nb, elem_base, scale_R,
                                      out_shift, stream);
    SrcPtrs s;
    bool vec = aligned16(dst);
    const bool quant = in_kind == F32 && out_kind == Q32, deq = in_kind == Q32 && out_kind == F32;
    if (fill_srcs(srcs, R, &s, &vec) || (!quant && !deq) || (dst == nullptr && n > 0) || out_shift < 0 ||
        out_shift > 8 || ((words_dev == nullptr || nb == 0) && n > 0))
        return INCCL_ERR_ARG;
    if (n == 0) return 0;
    if (scale_R <= 0) scale_R = R;
    hipStream_t st = (hipStream_t)stream;
#define INCCL_CALL(RR)                                                                                        \
    if (quant)                                                                                                \
        launch_stream<F32, Q32, RR>(s, dst, (int64_t)n, words_dev, (int64_t)nb, (int64_t)elem_base, scale_R,   \
                                    out_shift, vec, st);                                                      \
    else                                                                                                      \
        launch_stream<Q32, F32, RR>(s, dst, (int64_t)n, words_dev, (int64_t)nb, (int64_t)elem_base, scale_R,   \
                                    out_shift, vec, st)
    INCCL_R_SWITCH(R, INCCL_CALL)
#undef INCCL_CALL
    return (int)hipGetLastError();
}

int inccl_k_words_max(const uint32_t* rows_dev, int W, size_t nb, uint32_t* out_dev, void* stream)
{
    if (W < 1 || ((rows_dev == nullptr || out_dev == nullptr) && nb > 0)) return INCCL_ERR_ARG;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(k_words_max, dim3(grid_of((int64_t)nb, kBlock, 8)), dim3(kBlock), 0, (hipStream_t)stream, rows_dev,
                       W, (int64_t)nb, out_dev);
    return (int)hipGetLastError();
}

}  // extern "C"
