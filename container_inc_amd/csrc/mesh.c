/* mesh.c -- host side of the "mesh" engine: a large-bucket allreduce as one
 * persistent kernel per rank (work items, schedule and protocol in
 * inccl_mesh.hip).
 *
 * The p2p engine (p2p.c) runs quantise -> barrier -> pull reduce-scatter ->
 * barrier -> pull all-gather, with two host stream synchronisations per call
 * and no overlap between the phases.  Here one kernel does the whole call: its
 * push / reduce / gather items of different chunks meet through flags in HBM,
 * so quantisation, the local sums and the xGMI traffic in both directions
 * overlap, and the host never waits.
 *
 * Per rank, four device allocations shared over HIP IPC (separate, so that no
 * single export needs to exceed the group's IPC bound; see runtime.c):
 *   sig    [0, 64 KiB) signal array: arrive[8][1024] and ready[8][1024] words;
 *          [64 KiB, +256) call counter, retired workgroups, ticket, abort word,
 *          started workgroups, pushes finished per destination, clock
 *          readings (inccl_mesh.hip MeshArgs::ctr)
 *   inbox  W * cap int32: slot j holds rank j's partial of my shard
 *   res    cap fp32: my dequantised result shard
 *   resin  W * cap fp32 ("meshw"): slot j holds rank j's result shard
 * Created collectively on the first call, regrown collectively when a larger
 * bucket arrives (all ranks make the same calls, as with RCCL). */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "inccl_internal.h"
#include "inccl_kernels.h"

#define MESH_SIG_BYTES ((size_t)2 * INCCL_MAX_LOCAL_INPUTS * INCCL_MESH_MAX_CHUNKS * sizeof(uint32_t))
#define MESH_CTR_OFFSET MESH_SIG_BYTES
#define MESH_DATA_OFFSET (MESH_SIG_BYTES + (size_t)65536)

/* $INCCL_TRACE: one timestamped line per launch (debugging aid) */
#define MTRACE(...)                                                                      \
    do {                                                                                 \
        if (getenv("INCCL_TRACE")) {                                                     \
            struct timespec ts_;                                                         \
            clock_gettime(CLOCK_MONOTONIC, &ts_);                                        \
            fprintf(stderr, "[inccl %d %ld.%06ld] ", c->group->rank, (long)ts_.tv_sec,   \
                    ts_.tv_nsec / 1000);                                                 \
            fprintf(stderr, __VA_ARGS__);                                                \
            fputc('\n', stderr);                                                         \
        }                                                                                \
    } while (0)

typedef struct {
    int32_t ok, pci_domain, pci_bus, pci_dev;   /* ranks sharing a GPU split its workgroup slots */
} mesh_where;

void inccl_mesh_release(struct inccl_communicator *c)
{
    inccl_ipc_set_release(c->group, &c->mesh_ipc);
    inccl_err_words_destroy(&c->mesh_err_host, &c->mesh_err_dev);
    c->mesh_cap = 0;
}

/* bytes of region r for W ranks and `cap` elements per slot */
static size_t mesh_region_bytes(int r, int W, size_t cap)
{
    switch (r) {
        case 0: return MESH_DATA_OFFSET;                          /* signals + counters */
        case 2: return cap * sizeof(uint32_t);                    /* my result shard */
        default: return (size_t)W * cap * sizeof(uint32_t);       /* inbox / result inbox */
    }
}

/* collective: every rank calls it with the same shard size */
static int mesh_ensure(struct inccl_communicator *c, size_t shard)
{
    struct inccl_group *g = c->group;
    const int W = g->world_size;
    if (c->mesh_ipc.own[0] && c->mesh_cap >= shard) return 0;
    if (W > INCCL_MAX_LOCAL_INPUTS)
        return inccl_set_error(INCCL_ERR_ARG, "mesh engine supports up to %d GPUs", INCCL_MAX_LOCAL_INPUTS);
    const size_t cap = (shard + ((size_t)1 << 19) - 1) & ~(((size_t)1 << 19) - 1);   /* 2 MiB granules */
    /* every rank computes the same sizes, so every rank refuses alike */
    if (mesh_region_bytes(1, W, cap) > g->ipc_max_bytes)
        return inccl_set_error(INCCL_ERR_ARG, "mesh: a %zu-element shard needs a %zu-byte inbox; this group's IPC "
                               "buffers stay below %zu bytes (under PyTorch's bundled HSA runtime, importing a larger "
                               "one hangs; runtime.c)", shard, mesh_region_bytes(1, W, cap), g->ipc_max_bytes);
    const int dev = g->device >= 0 ? g->device : 0;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    /* where everyone is: ranks sharing a GPU size their grids together.  Every
     * rank sees the same gathered rows, so a bad one makes all of them fail alike */
    mesh_where mine, all[INCCL_MAX_LOCAL_INPUTS];
    memset(&mine, 0, sizeof(mine));
    mine.ok = hipDeviceGetAttribute(&mine.pci_domain, hipDeviceAttributePciDomainID, dev) == hipSuccess &&
              hipDeviceGetAttribute(&mine.pci_bus, hipDeviceAttributePciBusId, dev) == hipSuccess &&
              hipDeviceGetAttribute(&mine.pci_dev, hipDeviceAttributePciDeviceId, dev) == hipSuccess;
    int rc = inccl_boot_allgather(g, &mine, all, sizeof(mesh_where));
    if (rc) return rc;
    int sharing = 0;
    for (int j = 0; j < W; ++j) {
        if (!all[j].ok) return inccl_set_error(INCCL_ERR_HIP, "mesh: rank %d could not read its GPU's PCI ids", j);
        sharing += all[j].pci_domain == mine.pci_domain && all[j].pci_bus == mine.pci_bus &&
                   all[j].pci_dev == mine.pci_dev;
    }
    /* two workgroups per CU; ranks sharing one GPU split those slots, so that
     * their grids co-reside (every k_mesh<R> fits two 256-lane workgroups per CU;
     * the schedule's progress argument needs each rank to keep one running) */
    const char *ge = getenv("INCCL_MESH_GRID");
    int grid = ge ? atoi(ge) : 0;
    if (grid <= 0) grid = 2 * cus / (sharing > 0 ? sharing : 1);
    if (grid < 4) grid = 4;
    /* four separate regions, so that no single IPC export reaches 2 GiB for
     * buckets up to ~2 GiB at any W; all polled by the running kernel, the flags
     * and counters of region 0 start at zero */
    struct inccl_ipc_region regions[INCCL_MESH_REGIONS];
    for (int r = 0; r < INCCL_MESH_REGIONS; ++r)
        regions[r] = (struct inccl_ipc_region){mesh_region_bytes(r, W, cap), 1, r == 0 ? MESH_DATA_OFFSET : 0};
    /* a regrow replaces the error words (mesh_piece has read the old ones) */
    rc = inccl_err_words_create(&c->mesh_err_host, &c->mesh_err_dev, 32);
    rc = inccl_ipc_set_replace(g, &c->mesh_ipc, regions, INCCL_MESH_REGIONS, rc, "mesh");
    if (rc) {
        inccl_mesh_release(c);   /* back to a clean state: the next call starts over */
        return rc;
    }
    c->mesh_cap = cap;
    c->mesh_grid = grid;
    c->mesh_last_stream = NULL;
    if (c->mesh_timeout_ticks == 0) c->mesh_timeout_ticks = inccl_wait_ticks(g);
    return 0;
}

/* Chunk size: about 256 chunks per shard for overlap, 16-256 KiB each
 * ($INCCL_MESH_CHUNK elements overrides; agreed over the group, api.c). */
static size_t mesh_chunk(const struct inccl_communicator *c, size_t shard)
{
    size_t ch = c->mesh_chunk_env;
    if (ch == 0) {
        ch = (shard + 255) / 256;
        ch = (ch + 4095) & ~(size_t)4095;
        if (ch > 65536) ch = 65536;
    }
    ch = (ch + 63) & ~(size_t)63;
    if ((shard + ch - 1) / ch > INCCL_MESH_MAX_CHUNKS)
        ch = ((shard + INCCL_MESH_MAX_CHUNKS - 1) / INCCL_MESH_MAX_CHUNKS + 63) & ~(size_t)63;
    if (ch > shard) ch = shard;
    return ch;
}

/* After a timed-out call (epoch e, nchunks chunks): how many of its flags are
 * raised, counted by the host through both mappings of each signal array --
 * this rank's own allocation, and its IPC mapping of every peer's.  "arrived
 * from" j = my arrive[j][*] >= e; "mine at" j = arrive[me][*] in rank j's array
 * as read through my mapping of it (what my pushes wrote there); "ready" the
 * same for ready flags.  A push counted as finished whose flag is missing from
 * the receiver's own view but present through the sender's mapping would mean
 * the two mappings do not reach the same memory. */
static void mesh_flag_census(struct inccl_communicator *c, uint32_t e, uint32_t nchunks, char *out, size_t len)
{
    const int W = c->group->world_size, me = c->group->rank;
    if (nchunks == 0 || nchunks > INCCL_MESH_MAX_CHUNKS) {
        snprintf(out, len, "no flag census");
        return;
    }
    static uint32_t buf[INCCL_MESH_MAX_CHUNKS];
    int cnt[4][INCCL_MAX_LOCAL_INPUTS];
    memset(cnt, 0xff, sizeof(cnt));   /* -1: not read */
    for (int j = 0; j < W && j < INCCL_MAX_LOCAL_INPUTS; ++j) {
        const uint32_t *own = (const uint32_t *)c->mesh_ipc.own[0], *peer = (const uint32_t *)c->mesh_ipc.peer[0][j];
        const uint32_t *src[4] = {own + (size_t)j * INCCL_MESH_MAX_CHUNKS,
                                  own + (size_t)(INCCL_MAX_LOCAL_INPUTS + j) * INCCL_MESH_MAX_CHUNKS,
                                  peer ? peer + (size_t)me * INCCL_MESH_MAX_CHUNKS : NULL,
                                  peer ? peer + (size_t)(INCCL_MAX_LOCAL_INPUTS + me) * INCCL_MESH_MAX_CHUNKS : NULL};
        for (int k = 0; k < 4; ++k) {
            if (!src[k] || hipMemcpy(buf, src[k], nchunks * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
                continue;
            cnt[k][j] = 0;
            for (uint32_t i = 0; i < nchunks; ++i) cnt[k][j] += (int32_t)(buf[i] - e) >= 0;
        }
    }
    static const char *const names[4] = {"arrived from", "ready from", "mine at", "my ready at"};
    size_t o = 0;
    for (int k = 0; k < 4 && o < len; ++k) {
        o += (size_t)snprintf(out + o, len - o, "%s%s [", k ? "; " : "", names[k]);
        for (int j = 0; j < W && j < INCCL_MAX_LOCAL_INPUTS && o < len; ++j)
            o += (size_t)snprintf(out + o, len - o, "%s%d", j ? "," : "", cnt[k][j]);
        if (o < len) o += (size_t)snprintf(out + o, len - o, "] of %u", nchunks);
    }
}

static int mesh_piece(struct inccl_communicator *c, int kind16, const void *const *srcs, int R, void *dst, size_t n,
                      const struct inccl_scale *sc, int rs, hipStream_t st)
{
    const int W = c->group->world_size, me = c->group->rank;
    const size_t shard = inccl_shard_elems(n, W);
    if (rs && shard * (size_t)W != n)
        return inccl_set_error(INCCL_ERR_ARG, "mesh reduce-scatter: %zu elements are not %d shards of 64k", n, W);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    INCCL_HIP(hipStreamIsCapturing(st, &cap));
    const int capturing = cap != hipStreamCaptureStatusNone;
    if (capturing && (!c->mesh_ipc.own[0] || c->mesh_cap < shard))   /* collective setup cannot run in a capture */
        return inccl_set_error(INCCL_ERR_STATE, "mesh: make one call of this size outside graph capture first");
    /* an earlier call's failure is reported before anything else, a regrow
     * included (it would replace the error words) */
    const uint32_t err = c->mesh_err_host ? *(volatile uint32_t *)c->mesh_err_host : 0;
    if (err & INCCL_MESH_ERR_BOUNDS)   /* the kernel's per-item bounds check (inccl_mesh.hip inside()) */
        return inccl_set_error(INCCL_ERR_STATE, "mesh: an earlier call stopped at its bounds check (item %u, peer %u; "
                               "results invalid)", (err >> 8) & 0xffu, (err >> 4) & 0xfu);
    if (err) {   /* which wait expired, and this rank's progress (inccl_mesh.hip wait_flag) */
        const volatile uint32_t *e4 = (const volatile uint32_t *)c->mesh_err_host;
        char pushes[96], flags[320], clock[160];
        int o = 0;
        for (int j = 0; j < W && j < INCCL_MAX_LOCAL_INPUTS; ++j)
            o += snprintf(pushes + o, sizeof(pushes) - (size_t)o, "%s%u", j ? "," : "", e4[6 + j]);
        /* GPU clock (100 MHz / 16) in ms: timeout, call start, last push per destination */
        o = snprintf(clock, sizeof(clock), "clock ms: timeout %.3f, start %.3f, last push to", e4[15] * 1.6e-4,
                     e4[16] * 1.6e-4);
        for (int j = 0; j < W && j < INCCL_MAX_LOCAL_INPUTS && o < (int)sizeof(clock); ++j)
            o += snprintf(clock + o, sizeof(clock) - (size_t)o, "%s%.3f", j ? "," : " ", e4[17 + j] * 1.6e-4);
        mesh_flag_census(c, e4[2], e4[13], flags, sizeof(flags));
        return inccl_set_error(INCCL_ERR_STATE, "mesh: an earlier call timed out waiting for a peer (results invalid; "
                               "rank %d, %s of chunk %u, peer %u: flag %u, waited for epoch %u, re-read %u; "
                               "%u tickets taken, %u workgroups started, %u retired of %d; pushes finished per "
                               "destination [%s]; %s; %s)",
                               me, ((err >> 8) & 0xffu) == 3 ? "reduce's arrival flag" : "gather's ready flag",
                               err >> 16, (err >> 4) & 0xfu, e4[1], e4[2], e4[14], e4[3], e4[4], e4[5], c->mesh_grid,
                               pushes, flags, clock);
    }
    int rc = mesh_ensure(c, shard);
    if (rc) return rc;
    const size_t chunk = mesh_chunk(c, shard);
    const int nchunks = (int)((shard + chunk - 1) / chunk);
    /* a reduce / gather starts `lag` slots after what it waits for.  Default: the
     * whole shard, i.e. every push is taken before the first reduce and every
     * reduce before the first gather -- a workgroup waiting on a flag holds its
     * CU slot idle, and on one GPU (256 MiB, R = 2) lag = 1 / 171 / 400 / all
     * chunks ran 823 / 668 / 474 / 402 us.  Phases still overlap at their
     * seams, and both xGMI directions are busy in the push and gather phases.
     * ($INCCL_MESH_LAG slots overrides; agreed over the group, api.c.) */
    int lag = c->mesh_lag_env ? c->mesh_lag_env : nchunks;
    if (lag < 1) lag = 1;
    if (lag > nchunks) lag = nchunks;
    struct inccl_mesh_launch l;
    memset(&l, 0, sizeof(l));
    for (int r = 0; r < R; ++r) l.src[r] = (const float *)srcs[r];
    l.R = R;
    l.dst = (float *)dst;
    l.kind16 = kind16;
    l.n = n;
    l.shard = shard;
    l.chunk = chunk;
    l.inbox_stride = c->mesh_cap;
    l.nchunks = nchunks;
    l.lag = lag;
    l.grid = c->mesh_grid;
    for (int j = 0; j < W; ++j) {
        l.peer_sig[j] = (uint32_t *)c->mesh_ipc.peer[0][j];
        l.peer_inbox[j] = (uint32_t *)c->mesh_ipc.peer[1][j];
        l.peer_res[j] = (const uint32_t *)c->mesh_ipc.peer[2][j];
        l.peer_resin[j] = (uint32_t *)c->mesh_ipc.peer[3][j];
    }
    l.own_resin = l.peer_resin[me];
    l.push_res = c->mesh_push;
    l.rs = rs;
    l.own_inbox = l.peer_inbox[me];
    l.own_res = (uint32_t *)l.peer_res[me];
    l.own_sig = (const uint32_t *)c->mesh_ipc.own[0];
    l.ctr = (uint32_t *)(c->mesh_ipc.own[0] + MESH_CTR_OFFSET);
    l.err = c->mesh_err_dev;
    l.W = W;
    l.me = me;
    l.timeout_ticks = c->mesh_timeout_ticks;
    l.scale_exp = sc->k;
    l.amax_bits = sc->amax;
    l.scale_R = sc->R;
    l.out_shift = c->out_shift;
    const size_t es = kind16 ? sizeof(uint16_t) : sizeof(float);   /* source and result element bytes */
    l.src_bytes = n * es;
    l.dst_bytes = (rs ? shard : n) * es;
    l.inbox_bytes = mesh_region_bytes(1, W, c->mesh_cap);
    l.res_bytes = mesh_region_bytes(2, W, c->mesh_cap);
    l.resin_bytes = mesh_region_bytes(3, W, c->mesh_cap);
    /* the buffer-reuse argument needs this rank's calls in order: chain across
     * streams (inside a capture the caller's capture stream orders them) */
    if (!capturing && c->mesh_last_stream && c->mesh_last_stream != st) INCCL_HIP(hipStreamWaitEvent(st, c->ev[6], 0));
    MTRACE("mesh launch n %zu shard %zu chunk %zu nchunks %d lag %d grid %d", n, shard, chunk, nchunks, lag, l.grid);
    rc = inccl_k_mesh(&l, st);
    if (rc) return inccl_set_error(rc == INCCL_ERR_ARG ? INCCL_ERR_ARG : INCCL_ERR_HIP, "mesh kernel launch failed (%d)", rc);
    if (!capturing) {
        INCCL_HIP(hipEventRecord(c->ev[6], st));
        c->mesh_last_stream = st;
    }
    return 0;
}

/* the allreduce of kind F32, BF16 or F16 buckets; the 2-byte kinds run the same
 * kernel with 2-byte sources, int32 partials and a 2-byte result, so the xGMI
 * bytes are 4 + 2 per element instead of 4 + 4 */
int inccl_mesh_allreduce(struct inccl_communicator *c, int kind, const void *const *srcs, int R, void *dst, size_t n,
                         const struct inccl_scale *sc, hipStream_t st)
{
    if (kind != INCCL_KIND_F32 && kind != INCCL_KIND_BF16 && kind != INCCL_KIND_F16)
        return inccl_set_error(INCCL_ERR_ARG, "mesh: bad kind %d", kind);
    return mesh_piece(c, kind == INCCL_KIND_F32 ? 0 : kind, srcs, R, dst, n, sc, 0, st);
}

/* reduce-scatter (inccl_reduce_scatter_*): the same kernel and the same
 * instructions as the allreduce, with the gathers of other ranks' chunks reduced
 * to their flag waits and gather(c, me) copying this rank's own result chunk
 * into dst (its n / W elements, n % (64 W) == 0); kind INCCL_KIND_F32, BF16 or
 * F16 */
int inccl_mesh_reduce_scatter(struct inccl_communicator *c, int kind, const void *const *srcs, int R, void *dst,
                              size_t n, const struct inccl_scale *sc, hipStream_t st)
{
    return mesh_piece(c, kind == INCCL_KIND_F32 ? 0 : kind, srcs, R, dst, n, sc, 1, st);
}
