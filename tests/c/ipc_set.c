/* ipc_set.c -- the IPC buffer set protocol (container_inc_amd/csrc/ipc.c) and
 * inccl_boot_agree (bootstrap.c) without a GPU: this program stands in for the
 * HIP entry points ipc.c uses, and W = 3 forked ranks meet over the real TCP
 * bootstrap on 127.0.0.1.  Every allocation, export, free, open and close is
 * recorded in a table all ranks share, one entry per (rank, generation,
 * region); a handle carries exactly those three numbers.
 *
 *     ipc_set <case 1..7>      prints "ipc_set case N ok" and exits 0
 *
 * Linked from ipc.c, bootstrap.c and this file alone, no HIP library. */
#define _GNU_SOURCE
#include <arpa/inet.h>
#include <signal.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/socket.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include "inccl_internal.h"

enum { W = 3, MAXGEN = 6, MAGIC = 0x1bc5e7 };

struct buf {
    int alloc, freed, polled, exported;
    size_t bytes, lead_zero;   /* lead_zero: leading zero bytes at the export (memory starts as 0xab) */
    int opened[W], closed[W];  /* by rank i */
};
struct table {
    struct buf b[W][MAXGEN][INCCL_MESH_REGIONS];
    int violations;            /* an old buffer dropped before every rank had mapped the new set */
};
struct tag { int magic, rank, gen, region; };   /* a handle's payload, and what a mapping points at */

static struct table *T;
static int me, cur_gen = -1, cur_region, expect_next = -1, next_n, calls, fails;
static int fail_alloc_in, fail_open_in;   /* k > 0: the k-th call from now fails */
static struct { void *p; int gen, region; } owns[MAXGEN * INCCL_MESH_REGIONS];
static int n_owns;
static char g_err[512];

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            fprintf(stderr, "rank %d line %d: %s (last error: %s)\n", me, __LINE__, #cond, g_err); \
            fails++;                                                                           \
        }                                                                                      \
    } while (0)

int inccl_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int inccl_hip_check(hipError_t e, const char *what)
{
    return inccl_set_error(INCCL_ERR_HIP, "%s: hip error %d", what, (int)e);
}

/* ---- the HIP stand-ins ---- */

/* a generation-`gen` buffer is about to go: while a grow to gen + 1 runs, every
 * rank must already have mapped every region of every peer's gen + 1 */
static void dropping(int gen)
{
    if (gen + 1 != expect_next) return;
    for (int i = 0; i < W; ++i)
        for (int j = 0; j < W; ++j)
            for (int r = 0; r < next_n; ++r)
                if (i != j && __atomic_load_n(&T->b[j][gen + 1][r].opened[i], __ATOMIC_SEQ_CST) != 1)
                    __atomic_fetch_add(&T->violations, 1, __ATOMIC_SEQ_CST);
}

static hipError_t alloc_region(void **p, size_t bytes, int polled)
{
    calls++;
    if (fail_alloc_in && --fail_alloc_in == 0) return hipErrorOutOfMemory;
    if (cur_gen < 0 || cur_gen >= MAXGEN || cur_region >= INCCL_MESH_REGIONS) return hipErrorInvalidValue;
    *p = malloc(bytes);
    memset(*p, 0xab, bytes);
    struct buf *b = &T->b[me][cur_gen][cur_region];
    b->alloc++;
    b->polled = polled;
    b->bytes = bytes;
    owns[n_owns].p = *p;
    owns[n_owns].gen = cur_gen;
    owns[n_owns++].region = cur_region++;
    return hipSuccess;
}

hipError_t hipMalloc(void **p, size_t bytes) { return alloc_region(p, bytes, 0); }
hipError_t hipExtMallocWithFlags(void **p, size_t bytes, unsigned int flags)
{
    return alloc_region(p, bytes, flags == hipDeviceMallocUncached);
}

static int own_of(const void *p)
{
    for (int i = 0; i < n_owns; ++i)
        if (owns[i].p == p) return i;
    return -1;
}

hipError_t hipFree(void *p)
{
    calls++;
    const int i = own_of(p);
    if (i < 0) return hipErrorInvalidValue;
    dropping(owns[i].gen);
    T->b[me][owns[i].gen][owns[i].region].freed++;
    owns[i].p = NULL;
    free(p);
    return hipSuccess;
}

hipError_t hipMemset(void *dst, int value, size_t bytes)
{
    calls++;
    memset(dst, value, bytes);
    return hipSuccess;
}

hipError_t hipDeviceSynchronize(void)
{
    calls++;
    return hipSuccess;
}

hipError_t hipIpcGetMemHandle(hipIpcMemHandle_t *h, void *p)
{
    calls++;
    const int i = own_of(p);
    if (i < 0) return hipErrorInvalidValue;
    struct buf *b = &T->b[me][owns[i].gen][owns[i].region];
    b->exported++;
    while (b->lead_zero < b->bytes && ((const unsigned char *)p)[b->lead_zero] == 0) b->lead_zero++;
    const struct tag t = {MAGIC, me, owns[i].gen, owns[i].region};
    memset(h, 0, sizeof(*h));
    memcpy(h, &t, sizeof(t));
    return hipSuccess;
}

hipError_t hipIpcOpenMemHandle(void **p, hipIpcMemHandle_t h, unsigned int flags)
{
    calls++;
    struct tag t;
    memcpy(&t, &h, sizeof(t));
    if (fail_open_in && --fail_open_in == 0) return hipErrorInvalidValue;
    if (t.magic != MAGIC || flags != hipIpcMemLazyEnablePeerAccess) return hipErrorInvalidValue;   /* never exported */
    struct tag *m = (struct tag *)malloc(sizeof(t));
    *m = t;
    *p = m;
    __atomic_fetch_add(&T->b[t.rank][t.gen][t.region].opened[me], 1, __ATOMIC_SEQ_CST);
    return hipSuccess;
}

hipError_t hipIpcCloseMemHandle(void *p)
{
    calls++;
    struct tag *m = (struct tag *)p;
    if (own_of(p) >= 0 || m->magic != MAGIC) {   /* a rank's own region is freed, never closed */
        fails++;
        return hipErrorInvalidValue;
    }
    dropping(m->gen);
    T->b[m->rank][m->gen][m->region].closed[me]++;
    m->magic = 0;
    free(m);
    return hipSuccess;
}

hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int flags)
{
    calls++;
    *p = malloc(bytes);
    memset(*p, 0xab, bytes);
    return flags == hipHostMallocMapped ? hipSuccess : hipErrorInvalidValue;
}

hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned int flags)
{
    calls++;
    *dev = host;
    return hipSuccess;
}

hipError_t hipHostFree(void *p)
{
    calls++;
    free(p);
    return hipSuccess;
}

/* ---- the cases ---- */

static int replace(struct inccl_group *g, struct inccl_ipc_set *s, const struct inccl_ipc_region *reg, int n,
                   int local_rc, int grow)
{
    cur_gen++;
    cur_region = 0;
    expect_next = grow ? cur_gen : -1;
    next_n = n;
    const int rc = inccl_ipc_set_replace(g, s, reg, n, local_rc, "test");
    expect_next = -1;
    return rc;
}

/* the set is generation cur_gen, whole: own regions as asked for, every peer's
 * mapping from that peer's handle of the same region */
static void check_whole(const struct inccl_ipc_set *s, const struct inccl_ipc_region *reg, int n)
{
    CHECK(s->n == n);
    for (int r = 0; r < INCCL_MESH_REGIONS; ++r)
        for (int j = 0; j < INCCL_MAX_LOCAL_INPUTS; ++j) {
            if (r >= n || j >= W) {
                CHECK(s->peer[r][j] == NULL && (r < n || s->own[r] == NULL));
                continue;
            }
            const struct buf *b = &T->b[me][cur_gen][r];
            if (j == me) {
                CHECK(s->own[r] != NULL && s->peer[r][j] == s->own[r] && own_of(s->own[r]) >= 0);
                CHECK(b->alloc == 1 && b->exported == 1 && b->freed == 0 && b->bytes == reg[r].bytes);
                CHECK(b->polled == reg[r].polled);          /* the flag reached the right allocator */
                CHECK(b->lead_zero == reg[r].zero_bytes);   /* zeroed before the export, and no further */
            } else {
                const struct tag *m = (const struct tag *)s->peer[r][j];
                CHECK(m && m->magic == MAGIC && m->rank == j && m->gen == cur_gen && m->region == r);
                CHECK(T->b[j][cur_gen][r].opened[me] == 1 && T->b[j][cur_gen][r].closed[me] == 0);
            }
        }
}

static void check_empty(const struct inccl_ipc_set *s)
{
    static const struct inccl_ipc_set none;
    CHECK(memcmp(s, &none, sizeof(none)) == 0);
}

/* what this rank itself did to generation `gen` (n regions): freed its own and
 * closed its mappings `times` times each */
static void check_dropped(int gen, int n, int times)
{
    for (int r = 0; r < n; ++r)
        for (int j = 0; j < W; ++j)
            CHECK(j == me ? T->b[me][gen][r].freed == times : T->b[j][gen][r].closed[me] == times);
}

static const struct inccl_ipc_region R1[1] = {{4096, 1, 256}};
static const struct inccl_ipc_region R4[4] = {{4096, 1, 4096}, {8192, 0, 0}, {512, 1, 0}, {1024, 0, 128}};
static const struct inccl_ipc_region R2[2] = {{2048, 0, 0}, {1024, 1, 64}};
static const struct inccl_ipc_region R2b[2] = {{4096, 0, 0}, {2048, 1, 64}};

static double now(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* a failed replace: non-zero on every rank, promptly (nobody sat out a
 * bootstrap timeout), and the set is empty */
static void check_failed(int rc, const struct inccl_ipc_set *s, double t0)
{
    CHECK(rc != 0);
    CHECK(now() - t0 < 5.0);
    CHECK(!strstr(g_err, "allgather:") && !strstr(g_err, "barrier:"));
    check_empty(s);
}

static void run_case(int id, struct inccl_group *g)
{
    struct inccl_ipc_set s;
    memset(&s, 0, sizeof(s));
    int rc, failed = -2;
    double t0;
    switch (id) {
        case 1:   /* create: n = 1 and n = 4, mixed polled */
            CHECK(replace(g, &s, R1, 1, 0, 0) == 0);
            check_whole(&s, R1, 1);
            inccl_ipc_set_release(g, &s);
            check_empty(&s);
            CHECK(replace(g, &s, R4, 4, 0, 0) == 0);
            check_whole(&s, R4, 4);
            break;
        case 2:   /* grow twice: generation g goes only once every rank has mapped g + 1 */
            CHECK(replace(g, &s, R2, 2, 0, 0) == 0);
            for (int k = 0; k < 2; ++k) {
                CHECK(replace(g, &s, k ? R4 : R2b, k ? 4 : 2, 0, 1) == 0);
                check_whole(&s, k ? R4 : R2b, k ? 4 : 2);
                check_dropped(cur_gen - 1, 2, 1);
                check_dropped(cur_gen, k ? 4 : 2, 0);
            }
            break;
        case 3:   /* one rank's open fails: on a create, then on a grow */
            if (me == 1) fail_open_in = 2;
            t0 = now();
            rc = replace(g, &s, R2, 2, 0, 0);
            check_failed(rc, &s, t0);
            CHECK(replace(g, &s, R2, 2, 0, 0) == 0);   /* empty is where an engine starts over */
            check_whole(&s, R2, 2);
            if (me == 2) fail_open_in = 3;
            t0 = now();
            rc = replace(g, &s, R2b, 2, 0, 0);
            check_failed(rc, &s, t0);
            break;
        case 4:   /* one rank's allocation fails; it still takes every collective step */
            CHECK(replace(g, &s, R2, 2, 0, 0) == 0);
            if (me == 1) fail_alloc_in = 2;
            t0 = now();
            rc = replace(g, &s, R2b, 2, 0, 0);
            check_failed(rc, &s, t0);
            break;
        case 5:   /* a failure the caller brings along */
            t0 = now();
            rc = replace(g, &s, R2, 2, me == 2 ? -7 : 0, 0);
            check_failed(rc, &s, t0);
            CHECK(me == 2 ? rc == -7 : strstr(g_err, "rank 2 could not map") != NULL);
            break;
        case 6: {   /* release: nothing to do on an empty set, and the second time */
            int before = calls;
            inccl_ipc_set_release(g, &s);
            CHECK(calls == before);
            CHECK(replace(g, &s, R2, 2, 0, 0) == 0);
            inccl_ipc_set_release(g, &s);
            check_empty(&s);
            check_dropped(cur_gen, 2, 1);
            before = calls;
            inccl_ipc_set_release(g, &s);
            CHECK(calls == before);
            uint32_t *host = NULL, *dev = NULL;   /* the error words: zeroed, replaced, dropped */
            CHECK(inccl_err_words_create(&host, &dev, 32) == 0 && host && dev == host);
            for (int i = 0; host && i < 32; ++i) CHECK(host[i] == 0);
            CHECK(inccl_err_words_create(&host, &dev, 1) == 0 && host && host[0] == 0);
            inccl_err_words_destroy(&host, &dev);
            inccl_err_words_destroy(&host, &dev);
            CHECK(!host && !dev);
            break;
        }
        case 7:   /* inccl_boot_agree: the lowest failing rank on every rank, -1 without one */
            CHECK(inccl_boot_agree(g, 0, &failed) == 0 && failed == -1);
            CHECK(inccl_boot_agree(g, me >= 1, &failed) == 0 && failed == 1);
            CHECK(inccl_boot_agree(g, me == 2, &failed) == 0 && failed == 2);
            CHECK(inccl_boot_agree(g, 0, &failed) == 0 && failed == -1);
            break;
        default: fails++;
    }
    inccl_ipc_set_release(g, &s);
    check_empty(&s);
}

static int rank_main(int id, int port)
{
    prctl(PR_SET_PDEATHSIG, SIGKILL);
    struct inccl_group g;
    memset(&g, 0, sizeof(g));
    g.rank = me;
    g.world_size = W;
    g.device = -1;
    g.master_fd = -1;
    g.port = port;
    snprintf(g.master_ip, sizeof(g.master_ip), "127.0.0.1");
    const int up = (me == 0 ? inccl_boot_master(&g) : inccl_boot_worker(&g)) == 0;
    CHECK(up);
    if (up) {
        run_case(id, &g);
        CHECK(inccl_boot_barrier(&g) == 0);
    }
    inccl_boot_close(&g);
    return fails != 0;
}

int main(int argc, char **argv)
{
    const int id = argc > 1 ? atoi(argv[1]) : 0;
    setenv("INCCL_BOOT_TIMEOUT", "20", 1);
    unsetenv("INCCL_IPC_MEM");
    T = (struct table *)mmap(NULL, sizeof(*T), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (T == MAP_FAILED) return 2;
    struct sockaddr_in a;   /* a free port */
    socklen_t al = sizeof(a);
    memset(&a, 0, sizeof(a));
    a.sin_family = AF_INET;
    a.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
    const int ls = socket(AF_INET, SOCK_STREAM, 0);
    if (ls < 0 || bind(ls, (struct sockaddr *)&a, sizeof(a)) != 0 || getsockname(ls, (struct sockaddr *)&a, &al) != 0)
        return 2;
    close(ls);
    pid_t pid[W];
    for (me = 0; me < W; ++me) {
        pid[me] = fork();
        if (pid[me] == 0) _exit(rank_main(id, ntohs(a.sin_port)));
    }
    int bad = 0;
    for (int r = 0; r < W; ++r) {
        int st = 0;
        if (pid[r] < 0 || waitpid(pid[r], &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) {
            fprintf(stderr, "rank %d failed (status 0x%x)\n", r, st);
            bad++;
        }
    }
    /* the ledger: every allocation freed exactly once, every mapping closed
     * exactly once, by the rank that opened it */
    for (int j = 0; j < W; ++j)
        for (int gen = 0; gen < MAXGEN; ++gen)
            for (int r = 0; r < INCCL_MESH_REGIONS; ++r) {
                const struct buf *b = &T->b[j][gen][r];
                int ok = b->alloc <= 1 && b->freed == b->alloc && b->exported <= b->alloc && b->opened[j] == 0;
                for (int i = 0; i < W; ++i) ok = ok && b->opened[i] <= b->alloc && b->closed[i] == b->opened[i];
                if (!ok) {
                    fprintf(stderr, "rank %d generation %d region %d: alloc %d freed %d opened %d,%d,%d closed %d,%d,%d\n",
                            j, gen, r, b->alloc, b->freed, b->opened[0], b->opened[1], b->opened[2], b->closed[0],
                            b->closed[1], b->closed[2]);
                    bad++;
                }
            }
    if (T->violations) {
        fprintf(stderr, "%d old buffers dropped before every rank had mapped the new set\n", T->violations);
        bad++;
    }
    if (bad) return 1;
    printf("ipc_set case %d ok\n", id);
    return 0;
}
