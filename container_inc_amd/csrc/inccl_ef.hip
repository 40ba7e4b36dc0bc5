// inccl_ef.hip -- error feedback for packed 16-bit lanes (INCCL_KIND_P16) on
// CDNA4 (gfx950): every local bucket r has an fp32 residual e_r, the part of
// its last contribution the 16-bit lane could not carry; it is added to this
// call's contribution and rewritten.  Blocks, words, k_b, L, packing, sum and
// unpack are inccl_block.hip's and inccl_pack.hip's; semantics
// (tests/block16_ef_ref.py):
//
//   v     fl32(x + e)                     one IEEE add, denormals kept
//   w_b   the absmax word of block b over every v (NF: a NaN or +-Inf in v sets bit 31)
//   q     clamp(sat_i32(rne(v * 2^k_b)), -L, L), NaN -> 0   (the P16 rule on v)
//   d     fl32(v - (float)q * 2^-k_b)     the product is exact (|q| <= 2^15), so an
//                                         fma gives the same bits; no out_shift
//   e'    d if finite, else 0; 0 for every element of a block whose word has bit 31
//
// Kernels:
//   k_block_absmax_ef<R, NF>        the words of v: k_block_absmax with the
//                                   residual added after the load; 8 R n bytes
//   k_pack_block_ef<R>              F32 -> P16 in k_pack_block's layout (two
//                                   wave-wide dwordx4 rows per input, one
//                                   __shfl_xor pairing); e read by the same two
//                                   rows, e' written by two dwordx4 stores per
//                                   input; (12 R + 2) n + n / 64 bytes
//   k_pack_block_elem_ef<R>         per word (tails, elem_base % 4 != 0, unaligned pointers)
//   k_stream_block_fused_ef<R, NF>  world 1, one pass: k_stream_block_fused<.., P16>
//                                   on v, plus e'; (12 R + 4) n bytes.  The
//                                   flagged-block rule uses the word the wave computed
//   k_block_fused_elem_ef<R, NF>    the same on buckets that are not 16-B aligned
//
// A lane reads and writes the same elements of a residual and of nothing else
// of it, so a residual is updated in place; x and e are summed into v as they
// land, the kernel never holds both.  Nontemporal loads, vector stores
// (nontemporal for the residual quads) and plain C++.  Every lane of a wave reaches every __shfl_xor: the loops and
// branches around them are wave-uniform.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inccl_block.h"

namespace {

using namespace inccl_dev;

struct ResPtrs {
    float* p[kMaxR];
};

__device__ __forceinline__ uint32_t pack2(uint32_t lo, uint32_t hi) { return hi * 65536u + lo; }

// v = fl32(x + e) on raw bits
__device__ __forceinline__ uint32_t add1(uint32_t x, uint32_t e)
{
    return __float_as_uint(__uint_as_float(x) + __uint_as_float(e));
}
__device__ __forceinline__ u32x4 add_quad(u32x4 x, u32x4 e)
{
    return u32x4{add1(x.x, e.x), add1(x.y, e.y), add1(x.z, e.z), add1(x.w, e.w)};
}
__device__ __forceinline__ u32x4 ld_quad(const void* p, int64_t i)
{
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + i);
}
// A residual quad back to where it was read, nontemporal: a plain store leaves
// the line dirty in L2 beside the streamed inputs, and at R = 2 x 256 MiB the
// pack kernel then took 334-336 us against 287-293 and the fused one 344 against
// 279-283 (tools/ef_bench.py, alternating runs, profiles/pack16_ef/)
__device__ __forceinline__ void st_quad(float* p, int64_t i, u32x4 e)
{
    __builtin_nontemporal_store(e, reinterpret_cast<u32x4*>(p) + i);
}
__device__ __forceinline__ uint32_t ld1(const void* p, int64_t i) { return reinterpret_cast<const uint32_t*>(p)[i]; }

// one block's multipliers: 2^k_b to quantise, 2^-k_b for the residual (never
// NaN, no out_shift) and whether the word carries bit 31 (the residual is dropped)
struct EfMul {
    float scale, rinv;
    bool drop;
};
__device__ __forceinline__ EfMul ef_mul(uint32_t word, int scale_R)
{
    const int k = inccl_p16_scale_of_word(word, scale_R);
    return EfMul{pow2f(k), pow2f(-k), (word >> 31) != 0};
}

// the contribution q of v (returned) and the residual v - q * 2^-k_b it leaves (*e)
__device__ __forceinline__ uint32_t quant_ef(uint32_t v, const EfMul& m, int L, uint32_t* e)
{
    const uint32_t q = quantb<true>(__uint_as_float(v), m.scale, L);
    const uint32_t d = __float_as_uint(__uint_as_float(v) - (float)(int32_t)q * m.rinv);
    *e = (m.drop || (d & 0x7f800000u) == 0x7f800000u) ? 0u : d;
    return q;
}
__device__ __forceinline__ void quant_ef_quad(u32x4& acc, u32x4 v, const EfMul& m, int L, u32x4* e)
{
    uint32_t ex, ey, ez, ew;
    acc.x += quant_ef(v.x, m, L, &ex);
    acc.y += quant_ef(v.y, m, L, &ey);
    acc.z += quant_ef(v.z, m, L, &ez);
    acc.w += quant_ef(v.w, m, L, &ew);
    *e = u32x4{ex, ey, ez, ew};
}

constexpr int kBlkWaves = kBlock / 64;   // waves = blocks per workgroup and step of the per-block kernels

// words[b] = max |x + e| bits over block b of the R buckets; vec: every pointer is 16-B aligned
template <int R, bool NF>
__global__ __launch_bounds__(kBlock) void k_block_absmax_ef(SrcPtrs src, SrcPtrs res, int64_t n,
                                                            uint32_t* __restrict__ words, int vec)
{
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
                for (int r = 0; r < R; ++r) v[r] = add_quad(ld_quad(src.p[r], i), ld_quad(res.p[r], i));
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t a = amax_quad<NF>(v[r]);
                    m = m > a ? m : a;
                }
            } else if (i == n4) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    for (int j = 0; j < tail; ++j) {
                        const uint32_t a = abs_bits<NF>(add1(ld1(src.p[r], n4 * 4 + j), ld1(res.p[r], n4 * 4 + j)));
                        m = m > a ? m : a;
                    }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t e = (b << 8) + j * 64 + lane;
                    const uint32_t a = e < n ? abs_bits<NF>(add1(ld1(src.p[r], e), ld1(res.p[r], e))) : 0u;
                    m = m > a ? m : a;
                }
        }
        m = wave_max_u32(m);
        if (lane == 0) words[b] = m;
    }
}

// k_pack_block of inccl_pack.hip on v = x + e: a wave takes 128 consecutive
// quads per step, lane l quads wb + l (row A) and wb + 64 + l (row B) of every
// input and of its residual; each lane writes back the two residual quads it
// read and, after the pairing shuffle, one dwordx4 of packed words.
template <int R, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_pack_block_ef(SrcPtrs src, ResPtrs res, void* __restrict__ dst,
                                                         int64_t ntiles, const uint32_t* __restrict__ words,
                                                         int64_t nb, int64_t elem_base, int scale_R, int L)
{
    constexpr int WAVES = BLOCK / 64;
    const int lane = threadIdx.x & 63;
    u32x4* __restrict__ out = reinterpret_cast<u32x4*>(dst);
    for (int64_t t = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < ntiles; t += (int64_t)gridDim.x * WAVES) {
        const int64_t qa = (t << 7) + lane, qb = qa + 64;
        u32x4 a[R], b[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            a[r] = add_quad(ld_quad(src.p[r], qa), ld_quad(res.p[r], qa));
            b[r] = add_quad(ld_quad(src.p[r], qb), ld_quad(res.p[r], qb));
        }
        const EfMul ma = ef_mul(word_at(words, (elem_base + (qa << 2)) >> 8, nb), scale_R);
        const EfMul mb = ef_mul(word_at(words, (elem_base + (qb << 2)) >> 8, nb), scale_R);
        u32x4 sa = {0u, 0u, 0u, 0u}, sb = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            u32x4 ea, eb;
            quant_ef_quad(sa, a[r], ma, L, &ea);
            quant_ef_quad(sb, b[r], mb, L, &eb);
            st_quad(res.p[r], qa, ea);
            st_quad(res.p[r], qb, eb);
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
template <int R>
__global__ __launch_bounds__(kBlock) void k_pack_block_elem_ef(SrcPtrs src, ResPtrs res, void* __restrict__ dst,
                                                               int64_t begin, int64_t n,
                                                               const uint32_t* __restrict__ words, int64_t nb,
                                                               int64_t elem_base, int scale_R, int L)
{
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(dst);
    const int64_t m = (n + 1) >> 1;
    for (int64_t j = begin + (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (int64_t)gridDim.x * kBlock) {
        const EfMul mul = ef_mul(word_at(words, (elem_base + 2 * j) >> 8, nb), scale_R);
        const bool pair = 2 * j + 1 < n;
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            uint32_t* e = reinterpret_cast<uint32_t*>(res.p[r]);
            uint32_t e0, e1;
            lo += quant_ef(add1(ld1(src.p[r], 2 * j), e[2 * j]), mul, L, &e0);
            e[2 * j] = e0;
            if (pair) {
                hi += quant_ef(add1(ld1(src.p[r], 2 * j + 1), e[2 * j + 1]), mul, L, &e1);
                e[2 * j + 1] = e1;
            }
        }
        out[j] = pack2(lo, hi);
    }
}

// k_stream_block_fused<R, NF, P16 = true> of inccl_block.hip on v = x + e; every
// lane also writes the residual quads (and tail elements) it read
template <int R, bool NF, int BLOCK, int U>
__global__ __launch_bounds__(BLOCK) void k_stream_block_fused_ef(SrcPtrs src, ResPtrs res, void* __restrict__ dst,
                                                                 int64_t n, uint32_t* __restrict__ words,
                                                                 int scale_R, int out_shift)
{
    const int64_t n4 = n >> 2;
    const int tail = (int)(n & 3);                    // elements after the last quad: lane i == n4 takes them
    const int64_t nq = ((n + 255) >> 8) << 6;         // quads of whole blocks: a wave for every block
    const int64_t tile = (int64_t)BLOCK * U;
    const int lane = threadIdx.x & 63;
    const int L = inccl_p16_clamp(scale_R);
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
            for (int r = 0; r < R; ++r)
                v[r][u] = (full || i < n4) ? add_quad(ld_quad(src.p[r], i), ld_quad(res.p[r], i))
                                           : u32x4{0u, 0u, 0u, 0u};
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
                        t[r][j] = j < tail ? add1(ld1(src.p[r], n4 * 4 + j), ld1(res.p[r], n4 * 4 + j)) : 0u;
                        const uint32_t a = abs_bits<NF>(t[r][j]);
                        m = m > a ? m : a;
                    }
            }
            // the block's word, wave-uniform: the exponent is resolved once per wave
            const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(m));
            const EfMul mul = ef_mul(w, scale_R);
            const float inv = block_mul<true>(w, scale_R, out_shift).inv;
            if (words != nullptr && lane == 0) words[i >> 6] = w;
            u32x4 acc = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int r = 0; r < R; ++r) {
                u32x4 e;
                quant_ef_quad(acc, v[r][u], mul, L, &e);
                if (full || i < n4) st_quad(res.p[r], i, e);
            }
            const u32x4 o = xform_quad<F32>(acc, inv);
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
                            a += quant_ef(t[r][j], mul, L, &e);
                            reinterpret_cast<uint32_t*>(res.p[r])[n4 * 4 + j] = e;
                        }
                        out1[n4 * 4 + j] = store_xform<F32>(a, inv);
                    }
            }
        }
    }
}

// the fused kernel per element: lane t of the block's wave takes elements
// 256 b + t + 64 j, j < 4 (coalesced dword accesses)
template <int R, bool NF>
__global__ __launch_bounds__(kBlock) void k_block_fused_elem_ef(SrcPtrs src, ResPtrs res, void* __restrict__ dst,
                                                                int64_t n, uint32_t* __restrict__ words,
                                                                int scale_R, int out_shift)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nb = (n + 255) >> 8;
    const int L = inccl_p16_clamp(scale_R);
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(dst);
    for (int64_t b = (int64_t)blockIdx.x * kBlkWaves + wave; b < nb; b += (int64_t)gridDim.x * kBlkWaves) {
        uint32_t v[R][4];
        uint32_t m = 0;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t e = (b << 8) + j * 64 + lane;
                v[r][j] = e < n ? add1(ld1(src.p[r], e), ld1(res.p[r], e)) : 0u;
            }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t a = abs_bits<NF>(v[r][j]);
                m = m > a ? m : a;
            }
        const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(m));
        const EfMul mul = ef_mul(w, scale_R);
        const float inv = block_mul<true>(w, scale_R, out_shift).inv;
        if (words != nullptr && lane == 0) words[b] = w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t e = (b << 8) + j * 64 + lane;
            if (e < n) {
                uint32_t a = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    uint32_t ee;
                    a += quant_ef(v[r][j], mul, L, &ee);
                    reinterpret_cast<uint32_t*>(res.p[r])[e] = ee;
                }
                out[e] = store_xform<F32>(a, inv);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------
// r = the R residual pointers, none NULL; *vec stays true while all are 16-B aligned
int fill_res(const float* const* res, int R, ResPtrs* r, bool* vec)
{
    if (res == nullptr || R < 1 || R > kMaxR) return INCCL_ERR_ARG;
    *r = ResPtrs{};
    for (int i = 0; i < R; ++i) {
        if (res[i] == nullptr) return INCCL_ERR_ARG;
        r->p[i] = const_cast<float*>(res[i]);
        *vec = *vec && aligned16(res[i]);
    }
    return 0;
}

template <int R, bool NF>
void launch_absmax_ef(const SrcPtrs& s, const SrcPtrs& e, int64_t n, uint32_t* words, bool vec, hipStream_t st)
{
    hipLaunchKernelGGL((k_block_absmax_ef<R, NF>), dim3(grid_of((n + 255) >> 8, kBlkWaves, 8)), dim3(kBlock), 0, st, s, e,
                       n, words, vec ? 1 : 0);
}

template <int R>
void launch_pack_ef(const SrcPtrs& s, const ResPtrs& e, void* dst, int64_t n, const uint32_t* words, int64_t nb,
                    int64_t elem_base, int scale_R, bool vec, hipStream_t st)
{
    constexpr int B = 512;
    const int L = inccl_p16_clamp(scale_R);
    const int64_t m = (n + 1) >> 1;
    int64_t done = 0;   // words
    if (vec && (elem_base & 3) == 0) {
        const int64_t ntiles = n >> 9;   // whole waves of 512 elements
        if (ntiles > 0)
            hipLaunchKernelGGL((k_pack_block_ef<R, B>), dim3(grid_of(ntiles, B / 64, 8)), dim3(B), 0, st, s, e, dst, ntiles,
                               words, nb, elem_base, scale_R, L);
        done = ntiles << 8;
    }
    if (done < m)
        hipLaunchKernelGGL((k_pack_block_elem_ef<R>), dim3(grid_of(m - done, kBlock, 8)), dim3(kBlock), 0, st, s, e, dst,
                           done, n, words, nb, elem_base, scale_R, L);
}

template <int R, bool NF>
void launch_fused_ef(const SrcPtrs& s, const ResPtrs& e, void* dst, int64_t n, uint32_t* words, int scale_R,
                     int out_shift, bool vec, hipStream_t st)
{
    const int64_t nb = (n + 255) >> 8;
    if (vec) {
        constexpr int B = Geometry<R>::BLOCK, U = Geometry<R>::U;
        // one workgroup per tile, as the fused kernel without feedback
        hipLaunchKernelGGL((k_stream_block_fused_ef<R, NF, B, U>), dim3(grid_capped(nb * 64, B * U, kNoCap)), dim3(B), 0,
                           st, s, e, dst, n, words, scale_R, out_shift);
    } else {
        hipLaunchKernelGGL((k_block_fused_elem_ef<R, NF>), dim3(grid_of(nb, kBlkWaves, 8)), dim3(kBlock), 0, st, s, e, dst,
                           n, words, scale_R, out_shift);
    }
}

}  // namespace

extern "C" {

int inccl_k_block_absmax_ef(const void* const* srcs, const float* const* res, int R, size_t n, uint32_t* words_dev,
                            int flags, void* stream)
{
    SrcPtrs s, e;   // the residuals are only read here
    bool vec = true;
    if (fill_srcs(srcs, R, &s, &vec) || fill_srcs(reinterpret_cast<const void* const*>(res), R, &e, &vec) || (flags & ~INCCL_ABSMAX_FLAG_NONFINITE) ||
        (words_dev == nullptr && n > 0))
        return INCCL_ERR_ARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define INCCL_CALL(RR)                                                             \
    if (flags) launch_absmax_ef<RR, true>(s, e, (int64_t)n, words_dev, vec, st);   \
    else launch_absmax_ef<RR, false>(s, e, (int64_t)n, words_dev, vec, st)
    INCCL_R_SWITCH(R, INCCL_CALL)
#undef INCCL_CALL
    return (int)hipGetLastError();
}

int inccl_k_pack_block16_ef(const void* const* srcs, float* const* res, int R, void* dst, size_t n,
                            const uint32_t* words_dev, size_t nb, size_t elem_base, int scale_R, void* stream)
{
    SrcPtrs s;
    ResPtrs e;
    bool vec = aligned16(dst);
    if (fill_srcs(srcs, R, &s, &vec) || fill_res(res, R, &e, &vec) || (dst == nullptr && n > 0) ||
        ((words_dev == nullptr || nb == 0) && n > 0) || (elem_base & 1))
        return INCCL_ERR_ARG;
    if (scale_R <= 0) scale_R = R;
    if (scale_R > INCCL_P16_LANE_MAX) return INCCL_ERR_ARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define INCCL_CALL(RR) \
    launch_pack_ef<RR>(s, e, dst, (int64_t)n, words_dev, (int64_t)nb, (int64_t)elem_base, scale_R, vec, st)
    INCCL_R_SWITCH(R, INCCL_CALL)
#undef INCCL_CALL
    return (int)hipGetLastError();
}

int inccl_k_block_fused_ef(const void* const* srcs, float* const* res, int R, void* dst, size_t n,
                           uint32_t* words_out_dev, int flags, int scale_R, int out_shift, void* stream)
{
    SrcPtrs s;
    ResPtrs e;
    bool vec = aligned16(dst);
    if (fill_srcs(srcs, R, &s, &vec) || fill_res(res, R, &e, &vec) || (flags & ~INCCL_ABSMAX_FLAG_NONFINITE) ||
        (dst == nullptr && n > 0) || out_shift < 0 || out_shift > 8)
        return INCCL_ERR_ARG;
    if (scale_R <= 0) scale_R = R;
    if (scale_R > INCCL_P16_LANE_MAX) return INCCL_ERR_ARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define INCCL_CALL(RR)                                                                                 \
    if (flags) launch_fused_ef<RR, true>(s, e, dst, (int64_t)n, words_out_dev, scale_R, out_shift, vec, st);   \
    else launch_fused_ef<RR, false>(s, e, dst, (int64_t)n, words_out_dev, scale_R, out_shift, vec, st)
    INCCL_R_SWITCH(R, INCCL_CALL)
#undef INCCL_CALL
    return (int)hipGetLastError();
}

}  // extern "C"
