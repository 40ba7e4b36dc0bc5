/* ipc.c -- the device buffers an engine shares with every peer over HIP IPC
 * (the p2p, ll and mesh engines): one set of regions per engine and one
 * collective protocol that creates, regrows and drops it.
 *
 * Make before break: the new buffers are allocated, exported and mapped by
 * every peer while the old ones are still alive, and the old ones go only
 * after a group-wide synchronisation point.  Freeing first lets a new export
 * reuse the old one's identity (a dmabuf fd number) while a peer's runtime may
 * still resolve it to the old import: a regrowth then, intermittently, left one
 * rank reading a peer's old buffer on every later call. */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "inccl_internal.h"

/* Device memory that peers map over HIP IPC and that a running kernel polls or
 * reads after a flag (the ll and mesh engines).  Default "uncached"
 * (hipDeviceMallocUncached): every access bypasses the L2, so a remote GPU's
 * xGMI store into this HBM cannot hide behind a line this GPU's L2 cached
 * before it.  Coarse-grained hipMalloc memory is only guaranteed coherent with
 * other agents at kernel boundaries.  $INCCL_IPC_MEM = uncached | finegrained |
 * coarse selects the kind (same on every rank). */
unsigned inccl_ipc_mem_flags(void)
{
    const char *e = getenv("INCCL_IPC_MEM");
    if (e && strcmp(e, "coarse") == 0) return hipDeviceMallocDefault;
    if (e && strcmp(e, "finegrained") == 0) return hipDeviceMallocFinegrained;
    return hipDeviceMallocUncached;
}

hipError_t inccl_ipc_malloc(void **p, size_t bytes)
{
    const unsigned f = inccl_ipc_mem_flags();
    if (f == hipDeviceMallocDefault) return hipMalloc(p, bytes);
    return hipExtMallocWithFlags(p, bytes, f);
}

/* host-mapped words a kernel reports a failure in (ll: 1, mesh: 32), zeroed;
 * an existing pair is replaced once this rank's kernels have drained */
int inccl_err_words_create(uint32_t **host, uint32_t **dev, int words)
{
    if (*host) hipDeviceSynchronize();
    inccl_err_words_destroy(host, dev);
    hipError_t e = hipHostMalloc((void **)host, (size_t)words * sizeof(uint32_t), hipHostMallocMapped);
    if (e == hipSuccess) {
        for (int i = 0; i < words; ++i) ((volatile uint32_t *)*host)[i] = 0;
        e = hipHostGetDevicePointer((void **)dev, *host, 0);
    }
    return e == hipSuccess ? 0 : inccl_hip_check(e, "error words: hipHostMalloc");
}

void inccl_err_words_destroy(uint32_t **host, uint32_t **dev)
{
    if (*host) hipHostFree(*host);
    *host = NULL;
    *dev = NULL;
}

void inccl_ipc_set_release(struct inccl_group *g, struct inccl_ipc_set *s)
{
    if (!s->n) return;
    hipDeviceSynchronize();
    for (int r = 0; r < INCCL_MESH_REGIONS; ++r) {
        for (int j = 0; j < INCCL_MAX_LOCAL_INPUTS; ++j)
            if (j != g->rank && s->peer[r][j]) hipIpcCloseMemHandle(s->peer[r][j]);
        if (s->own[r]) hipFree(s->own[r]);
    }
    memset(s, 0, sizeof(*s));
}

typedef struct {
    hipIpcMemHandle_t h[INCCL_MESH_REGIONS];
} ipc_handles;

/* $INCCL_TRACE: every (re)growth logs, per rank, its own bases and, per peer,
 * the FNV-1a hash of each exported handle and the base it mapped to, so that a
 * mapping that resolves to an earlier export (same base as before while the
 * handle changed) is visible in the log */
static void ipc_trace(const struct inccl_group *g, const struct inccl_ipc_set *s, const ipc_handles *all,
                      const char *who)
{
    if (!getenv("INCCL_TRACE")) return;
    char line[4096];
    int k = snprintf(line, sizeof(line), "[inccl %s rank %d] mapped, own", who, g->rank);
    for (int r = 0; r < s->n && (size_t)k < sizeof(line); ++r)
        k += snprintf(line + k, sizeof(line) - (size_t)k, " %p", (void *)s->own[r]);
    for (int j = 0; j < g->world_size; ++j) {
        if ((size_t)k < sizeof(line)) k += snprintf(line + k, sizeof(line) - (size_t)k, " | peer %d", j);
        for (int r = 0; r < s->n && (size_t)k < sizeof(line); ++r) {
            const unsigned char *b = (const unsigned char *)&all[j].h[r];
            uint64_t x = 1469598103934665603ull;
            for (size_t i = 0; i < sizeof(hipIpcMemHandle_t); ++i) x = (x ^ b[i]) * 1099511628211ull;
            k += snprintf(line + k, sizeof(line) - (size_t)k, " %016llx -> %p", (unsigned long long)x,
                          (void *)s->peer[r][j]);
        }
    }
    fprintf(stderr, "%s\n", line);   /* one write per line: ranks share the log */
}

int inccl_ipc_set_replace(struct inccl_group *g, struct inccl_ipc_set *s, const struct inccl_ipc_region *regions,
                          int n, int local_rc, const char *who)
{
    const int W = g->world_size, me = g->rank;
    if (W > INCCL_MAX_LOCAL_INPUTS || n < 1 || n > INCCL_MESH_REGIONS)   /* the same on every rank */
        return inccl_set_error(INCCL_ERR_ARG, "%s: %d IPC regions over %d ranks", who, n, W);
    int rc = local_rc;
    char what[64];
    hipError_t e = hipSuccess;
    if (s->n) {
        /* every rank's queued accesses to the peers' old buffers drain before
         * anyone may drop them */
        e = hipDeviceSynchronize();
        int rc_b = inccl_boot_barrier(g);
        if (rc_b) return rc_b;
    }
    struct inccl_ipc_set old = *s;
    memset(s, 0, sizeof(*s));
    s->n = n;
    /* a local failure is carried to the agreement below: a rank that failed
     * must not leave its peers waiting in a collective step it never reaches */
    ipc_handles mine, all[INCCL_MAX_LOCAL_INPUTS];
    memset(&mine, 0, sizeof(mine));
    for (int r = 0; r < n && e == hipSuccess; ++r) {
        e = regions[r].polled ? inccl_ipc_malloc((void **)&s->own[r], regions[r].bytes)
                              : hipMalloc((void **)&s->own[r], regions[r].bytes);
        if (e == hipSuccess && regions[r].zero_bytes) {   /* zeroed before any peer maps it */
            e = hipMemset(s->own[r], 0, regions[r].zero_bytes);
            if (e == hipSuccess) e = hipDeviceSynchronize();
        }
        if (e == hipSuccess) e = hipIpcGetMemHandle(&mine.h[r], s->own[r]);
    }
    snprintf(what, sizeof(what), "%s: buffer setup", who);
    if (e != hipSuccess && !rc) rc = inccl_hip_check(e, what);
    int rc_x = inccl_boot_allgather(g, &mine, all, sizeof(ipc_handles));
    for (int j = 0; !rc_x && j < W; ++j)
        for (int r = 0; r < n; ++r) {
            if (j == me) {
                s->peer[r][j] = s->own[r];
            } else if (!rc) {
                e = hipIpcOpenMemHandle((void **)&s->peer[r][j], all[j].h[r], hipIpcMemLazyEnablePeerAccess);
                if (e == hipSuccess) continue;
                snprintf(what, sizeof(what), "%s: hipIpcOpenMemHandle", who);
                rc = inccl_hip_check(e, what);
            }
        }
    if (!rc_x) ipc_trace(g, s, all, who);
    /* agree on the outcome, so that every rank sees a failure and the caller
     * can fall back on every rank alike */
    int failed = -1;
    if (!rc_x) rc_x = inccl_boot_agree(g, rc != 0, &failed);
    if (rc_x) rc = rc_x;
    else if (failed >= 0 && !rc)
        rc = inccl_set_error(INCCL_ERR_HIP, "%s: rank %d could not map the peer buffers", who, failed);
    if (rc) inccl_ipc_set_release(g, s);   /* back to empty: the engine's next call starts over */
    /* On success every peer has mapped the new buffers and the old ones can go:
     * the agreement is the synchronisation point.  A rank sends its outcome only
     * after its opens, and rank 0 sends nothing back until it has received from
     * every rank (inccl_boot_allgather), so no rank gets here earlier. */
    inccl_ipc_set_release(g, &old);
    return rc;
}
