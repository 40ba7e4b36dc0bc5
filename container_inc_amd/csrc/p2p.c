/* p2p.c -- the "p2p" exchange engine: reduce-scatter and all-gather as direct
 * peer reads over xGMI with this library's own kernels (no RCCL on the data path).
 *
 * Every rank owns two library-allocated device buffers that every peer maps over
 * HIP IPC (one buffer set, created and regrown by ipc.c):
 *   part  int32 [W * shard]  this rank's quantised local sums (W shards)
 *   res   fp32  [W * shard]  this rank's dequantised result shard at rank * shard
 * One bucket piece:
 *   1. quant + local sum of the R buckets -> part            (HBM, local)
 *   2. stream sync + group barrier                            (all parts ready)
 *   3. res[me] = dequant( sum_j part_j[me] )  -- one kernel reading the W
 *      peers' shard me concurrently (W-1 of them over xGMI): the reference's
 *      switch aggregate (non_termination_switch.c:361-363) fused with the new
 *      dequantise stage
 *   4. stream sync + group barrier                            (all shards ready)
 *   5. dst[j] = res_j[j] for every j -- one gather kernel pulling all W shards
 * Buffer reuse is safe without a third barrier: a rank reaches the next
 * call's step-2 barrier only after its own step 5 has drained (the sync in 2),
 * so nobody still reads a `part` or `res` that the next call overwrites.
 * Host barriers cost tens of microseconds; the step moves hundreds of MB.
 * Steps 3 and 5 read peer memory with system-coherent loads (inccl_peer.hip):
 * IPC-mapped remote VRAM may sit non-coherently in this GPU's L2 from the
 * previous call. */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "inccl_internal.h"
#include "inccl_kernels.h"

void inccl_p2p_release(struct inccl_communicator *c)
{
    inccl_ipc_set_release(c->group, &c->p2p_ipc);
    c->p2p_cap = 0;
}

/* collective: every rank calls it with the same `elems` */
static int p2p_ensure(struct inccl_communicator *c, size_t elems)
{
    struct inccl_group *g = c->group;
    if (c->p2p_cap >= elems && c->p2p_ipc.own[0]) return 0;
    if (elems * sizeof(int32_t) > g->ipc_max_bytes)   /* same sizes and bound on every rank: all refuse alike */
        return inccl_set_error(INCCL_ERR_ARG, "p2p: a %zu-element bucket needs %zu-byte IPC buffers; this group's stay "
                               "below %zu bytes (under PyTorch's bundled HSA runtime, importing a larger one hangs; "
                               "runtime.c)", elems, elems * sizeof(int32_t), g->ipc_max_bytes);
    int rc = inccl_boot_shm_init(g);   /* same-node fast barrier for the per-call syncs */
    if (rc) return rc;
    const size_t cap = (elems + (1u << 19) - 1) & ~(size_t)((1u << 19) - 1);   /* 2 MiB granules */
    /* read after a kernel boundary and a barrier, never polled: plain hipMalloc */
    const struct inccl_ipc_region regions[2] = {{cap * sizeof(int32_t), 0, 0}, {cap * sizeof(float), 0, 0}};
    rc = inccl_ipc_set_replace(g, &c->p2p_ipc, regions, 2, 0, "p2p");
    c->p2p_cap = rc ? 0 : cap;
    return rc;
}

static int sync_and_barrier(struct inccl_communicator *c, hipStream_t st)
{
    INCCL_HIP(hipStreamSynchronize(st));
    return inccl_group_barrier(c->group);
}

/* The one exchange every p2p call is (steps 1-5 of the header comment):
 *   fill    in_kind F32 / BF16 / F16: quant + local sum of the R buckets -> part;
 *           in_kind Q32: srcs[0] copied into part (the int32 allreduce)
 *   reduce  shard `me` pulled from every peer and summed; out_kind F32 / BF16 /
 *           F16 dequantises (and narrows: 2 bytes per element over xGMI instead
 *           of 4), Q32 leaves the int32 sum (the reference's switch add,
 *           nts.c:361-363, and nothing else)
 *   gather  != 0: the allreduce -- shards padded (inccl_shard_elems), the reduce
 *           lands in res at me * shard and every rank's shard is gathered into
 *           dst (2-byte kinds: dst 4-byte aligned);
 *           0: reduce-scatter -- n = W * shard, shard % 4 == 0, the reduce lands
 *           straight in dst; the closing barrier keeps every rank from rewriting
 *           its part (the next call's fill) while a peer still reads it. */
static int p2p_exchange(struct inccl_communicator *c, int in_kind, const void *const *srcs, int R, int out_kind,
                        void *dst, size_t n, const struct inccl_scale *sc, int gather, hipStream_t st)
{
    const int W = c->group->world_size, me = c->group->rank;
    if (W > INCCL_MAX_LOCAL_INPUTS) return inccl_set_error(INCCL_ERR_ARG, "p2p engine supports up to %d GPUs",
                                                          INCCL_MAX_LOCAL_INPUTS);
    if (n == 0) return 0;
    const int half = out_kind == INCCL_KIND_BF16 || out_kind == INCCL_KIND_F16;
    const size_t es = half ? sizeof(uint16_t) : sizeof(float);   /* result element bytes */
    const char *what = !gather ? "" : out_kind == INCCL_KIND_Q32 ? "int32 " : half ? "16-bit " : "";
    const size_t shard = gather ? inccl_shard_elems(n, W) : n / (size_t)W, total = shard * (size_t)W;
    if (!gather && (total != n || (shard & 3))) return inccl_set_error(INCCL_ERR_ARG, "p2p reduce-scatter: bad shard");
    int rc = p2p_ensure(c, total);
    if (rc) return rc;
    int32_t *part = (int32_t *)c->p2p_ipc.own[0];
    /* the previous call's gather may still be reading the peers' result shards,
     * which the peers rewrite once this call's first barrier has passed: order
     * it before that barrier's host sync when the caller switches streams */
    if (c->p2p_last_stream && c->p2p_last_stream != st) INCCL_HIP(hipStreamWaitEvent(st, c->ev[8], 0));
    /* 1. fill part */
    if (in_kind == INCCL_KIND_Q32) {
        INCCL_HIP(hipMemcpyAsync(part, srcs[0], n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    } else {
        rc = inccl_k_stream(in_kind, INCCL_KIND_Q32, srcs, R, part, n, sc->k, sc->amax, sc->R, 0, st);
        if (rc) return inccl_set_error(INCCL_ERR_HIP, "p2p %squant+sum launch failed (%d)",
                                       gather ? what : "reduce-scatter ", rc);
    }
    if (total > n) INCCL_HIP(hipMemsetAsync(part + n, 0, (total - n) * sizeof(int32_t), st));
    rc = sync_and_barrier(c, st);
    if (rc) return rc;
    /* 3. pull shard `me` from every peer, sum, dequantise */
    const void *peer[INCCL_MAX_LOCAL_INPUTS];
    for (int j = 0; j < W; ++j) peer[j] = (const int32_t *)c->p2p_ipc.peer[0][j] + (size_t)me * shard;
    rc = inccl_k_peer_reduce(out_kind, peer, W, gather ? (void *)(c->p2p_ipc.own[1] + (size_t)me * shard * es) : dst,
                             shard, sc->k, sc->amax, sc->R, out_kind == INCCL_KIND_Q32 ? 0 : c->out_shift, st);
    if (rc) return inccl_set_error(INCCL_ERR_HIP, "p2p %sreduce-scatter launch failed (%d)", what, rc);
    rc = sync_and_barrier(c, st);
    if (rc) return rc;
    if (gather) {
        /* 5. gather every shard into dst (ragged last shard clamped to n) */
        const void *src[INCCL_MAX_LOCAL_INPUTS];
        int64_t off[INCCL_MAX_LOCAL_INPUTS], cnt[INCCL_MAX_LOCAL_INPUTS];
        for (int j = 0; j < W; ++j) {
            const size_t lo = (size_t)j * shard;
            src[j] = c->p2p_ipc.peer[1][j] + lo * es;
            off[j] = (int64_t)lo;
            cnt[j] = lo >= n ? 0 : (int64_t)((n - lo) < shard ? (n - lo) : shard);
        }
        rc = inccl_k_peer_gather((int)es, src, off, cnt, W, dst, st);
        if (rc) return inccl_set_error(INCCL_ERR_HIP, "p2p %sgather launch failed (%d)", what, rc);
    }
    INCCL_HIP(hipEventRecord(c->ev[8], st));
    c->p2p_last_stream = st;
    return 0;
}

int inccl_p2p_allreduce(struct inccl_communicator *c, int kind, const void *const *srcs, int R, void *dst, size_t n,
                        const struct inccl_scale *sc, hipStream_t st)
{
    return p2p_exchange(c, kind, srcs, R, kind, dst, n, sc, 1, st);
}

int inccl_p2p_reduce_scatter(struct inccl_communicator *c, int kind, const void *const *srcs, int R, void *dst,
                             size_t n, const struct inccl_scale *sc, hipStream_t st)
{
    return p2p_exchange(c, kind, srcs, R, kind, dst, n, sc, 0, st);
}

/* send may alias recv */
int inccl_p2p_allreduce_q32(struct inccl_communicator *c, const int32_t *send, int32_t *recv, size_t n,
                            hipStream_t st)
{
    static const struct inccl_scale none = {0, NULL, 0};
    const void *s1[1] = {send};
    return p2p_exchange(c, INCCL_KIND_Q32, s1, 1, INCCL_KIND_Q32, recv, n, &none, 1, st);
}
