/* inccl_kernels.h -- the thin C-ABI shim between the C host code and the HIP
 * kernels of the seven .hip files (inccl_kernels, _block, _pack, _peer, _ll,
 * _mesh; inccl_frames.hip has inccl_frames.h).  Internal to libinccl_amd.so. */
#ifndef INCCL_KERNELS_H
#define INCCL_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#include "inccl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[i] = OUT(sum_r IN(srcs[r][i])), kinds INCCL_KIND_*; the dequantise is scaled by 2^-out_shift
 * (inccl_comm_set_average; 0: the plain sum).  Returns 0 or a hipError_t / INCCL_ERR_ARG. */
int inccl_k_stream(int in_kind, int out_kind, const void *const *srcs, int R, void *dst, size_t n, int scale_exp,
                   const uint32_t *amax_bits_dev, int scale_R, int out_shift, void *stream);
/* absmax word of R buckets of kind F32 / BF16 / F16 (include/inccl_amd.h inccl_absmax_*) */
int inccl_k_absmax(int kind, const void *const *srcs, int R, size_t n, uint32_t *amax_bits_dev, int zero_first,
                   void *stream);
int inccl_k_checksum(const int32_t *q, size_t n, uint64_t index_base, uint32_t *out_dev, int zero_first,
                     void *stream);
/* per-block auto scaling of fp32 buckets (inccl_block.hip; include/inccl_amd.h INCCL_SCALE_BLOCK).
 * flags: 0 or INCCL_ABSMAX_FLAG_NONFINITE.
 *   block_absmax  words[b] = the absmax word of block b of the R buckets, ceil(n / 256) words, overwritten
 *   block_fused   dst = dequant(sum_r quant(srcs[r])) at each block's own exponent, resolved in the
 *                 kernel for scale_R contributors; words_out (NULL ok) receives the words
 *   stream_block  F32 -> Q32 or Q32 -> F32 at the agreed words: element i is element elem_base + i of
 *                 the bucket whose block 0 words_dev points at; a block index past nb - 1 reads word nb - 1
 *   words_max     out[b] = max_j rows[j * nb + b] (unsigned)
 * Packed 16-bit lanes (INCCL_KIND_P16; inccl_pack.hip): block_fused with p16 != 0 takes the lanes'
 * exponent and clamp; stream_block also takes F32 -> P16 (dst: ceil(n / 2) words, elem_base even) and
 * P16 -> F32 (n: elements of dst; srcs point at the word that holds element elem_base) and hands them
 * to stream_block16.  scale_R above INCCL_P16_LANE_MAX is INCCL_ERR_ARG.
 * Error feedback for the packed lanes (include/inccl_amd.h inccl_*_ef): res is NULL (none) or R fp32
 * residuals, res[r] n elements beside srcs[r], none NULL; the kernel then works on v = srcs[r] + res[r].
 * A res that is not NULL belongs to the packed lanes only (block_fused: p16 != 0; stream_block16:
 * F32 -> P16), INCCL_ERR_ARG otherwise.
 *   block_absmax    of v; the residuals are only read
 *   block_fused     of v; res[r][i] becomes what the lane did not carry, 0 in a block whose word has bit 31
 *   stream_block16  F32 -> P16 of v at the agreed words, the residuals rewritten alike */
int inccl_k_block_absmax(const void *const *srcs, const float *const *res, int R, size_t n, uint32_t *words_dev,
                         int flags, void *stream);
int inccl_k_block_fused(const void *const *srcs, float *const *res, int R, void *dst, size_t n,
                        uint32_t *words_out_dev, int flags, int scale_R, int out_shift, int p16, void *stream);
int inccl_k_stream_block16(int in_kind, int out_kind, const void *const *srcs, float *const *res, int R, void *dst,
                           size_t n, const uint32_t *words_dev, size_t nb, size_t elem_base, int scale_R,
                           int out_shift, void *stream);
int inccl_k_stream_block(int in_kind, int out_kind, const void *const *srcs, int R, void *dst, size_t n,
                         const uint32_t *words_dev, size_t nb, size_t elem_base, int scale_R, int out_shift,
                         void *stream);
int inccl_k_words_max(const uint32_t *rows_dev, int W, size_t nb, uint32_t *out_dev, void *stream);
void inccl_k_set_tuning(int grid_cap, int nt_loads);
/* p2p engine kernels reading peer memory with system-coherent loads (inccl_peer.hip).
 * The pull-reduce, n % 4 == 0, by out_kind:
 *   F32          dst[i] = dequant(sum_j peers[j][i]), dst 16-B aligned
 *   BF16 / F16   the same narrowed round to nearest even, dst 8-B aligned
 *   Q32          dst[i] = sum_j peers[j][i] (int32, wrapping; the scale is unused), dst 16-B aligned */
int inccl_k_peer_reduce(int out_kind, const void *const *peers, int W, void *dst, size_t n, int scale_exp,
                        const uint32_t *amax_bits_dev, int scale_R, int out_shift, void *stream);
/* dst[off[j] .. off[j]+cnt[j]) = src[j][0 .. cnt[j]) for j < nseg in one launch; es-byte elements, es 4 or
 * 2 (counts and even offsets in elements; dst 4-B aligned) */
int inccl_k_peer_gather(int es, const void *const *src, const int64_t *off, const int64_t *cnt, int nseg, void *dst,
                        void *stream);

/* the one-kernel small-bucket allreduce (inccl_ll.hip) */
#define INCCL_LL_MAX_BLOCKS 256   /* workgroups per call = flags per rank in a signal array */
struct inccl_ll_launch {
    const float *src[INCCL_MAX_LOCAL_INPUTS];
    int R;
    float *dst;
    size_t n;
    uint32_t *own_data;                                /* own data slot 0; slot 1 at + slot_elems */
    const uint32_t *peer_data[INCCL_MAX_LOCAL_INPUTS]; /* every rank's slot 0, [me] = own_data */
    size_t slot_elems;
    uint32_t *peer_sig[INCCL_MAX_LOCAL_INPUTS];        /* per rank signal arrays (W x MAX_BLOCKS words) */
    const uint32_t *own_sig;
    uint32_t *ctr;                                     /* own device words: [0] calls done, [1] workgroups retired */
    uint32_t *err;                                     /* device view of a host-mapped word */
    int W, me;
    uint64_t timeout_ticks;
    int scale_exp;
    const uint32_t *amax_bits;
    int scale_R;
    int out_shift;                                     /* dequantise with 2^-(k + out_shift) */
    size_t rs_lo, rs_n;                                /* rs_n > 0: reduce-scatter -- dst = elements
                                                        * [rs_lo, rs_lo + rs_n) of the result (both % 4 == 0) */
    int grid;                                          /* workgroups: inccl_k_ll_grid(n), the same on every rank */
};
int inccl_k_ll_grid(size_t n);
int inccl_k_ll_protocol_wt(void);   /* 1: the wt protocol, 0: fence ($INCCL_LL_PROTOCOL) */
int inccl_k_ll_oneshot(const struct inccl_ll_launch *l, void *stream);

/* the one-kernel large-bucket allreduce (inccl_mesh.hip): push reduce-scatter,
 * per-chunk arrival flags, pull all-gather */
#define INCCL_MESH_MAX_CHUNKS 1024   /* chunks per shard = flags per source rank */
struct inccl_mesh_launch {
    const float *src[INCCL_MAX_LOCAL_INPUTS];
    int R;
    float *dst;
    size_t n;
    size_t shard;                                      /* elements per rank's shard, multiple of 64 */
    size_t chunk;                                      /* elements per chunk, multiple of 64 */
    size_t inbox_stride;                               /* elements per source slot of an inbox */
    int nchunks, lag, grid;
    uint32_t *peer_inbox[INCCL_MAX_LOCAL_INPUTS];      /* every rank's inbox ([me] = own) */
    const uint32_t *own_inbox;
    uint32_t *own_res;
    const uint32_t *peer_res[INCCL_MAX_LOCAL_INPUTS];  /* every rank's result shard */
    uint32_t *peer_resin[INCCL_MAX_LOCAL_INPUTS];      /* every rank's result inbox (push_res) */
    const uint32_t *own_resin;
    int push_res;                                      /* 1: reduce pushes results, gather copies locally */
    int rs;                                            /* 1: reduce-scatter -- dst is this rank's shard */
    int kind16;                                        /* 0: fp32 src / dst; INCCL_KIND_BF16 / _F16: 2-byte ones */
    uint32_t *peer_sig[INCCL_MAX_LOCAL_INPUTS];        /* every rank's signal array */
    const uint32_t *own_sig;
    uint32_t *ctr;                                     /* own words: calls, retired, ticket, abort */
    uint32_t *err;                                     /* device view of a host-mapped word */
    int W, me;
    uint64_t timeout_ticks;
    int scale_exp;
    const uint32_t *amax_bits;
    int scale_R;
    int out_shift;                                     /* dequantise with 2^-(k + out_shift) */
    /* region sizes for the kernel's per-item bounds check (every rank's regions
     * have the same sizes): a work item whose buffer range falls outside its
     * region stores INCCL_MESH_ERR_BOUNDS | item << 8 | peer << 4 into *err
     * and aborts the call instead of touching memory */
    size_t src_bytes, dst_bytes, inbox_bytes, res_bytes, resin_bytes;
};
#define INCCL_MESH_ERR_TIMEOUT 1u
#define INCCL_MESH_ERR_BOUNDS 2u
int inccl_k_mesh(const struct inccl_mesh_launch *l, void *stream);

#ifdef __cplusplus
}
#endif
#endif
