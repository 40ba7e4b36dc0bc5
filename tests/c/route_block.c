/* route_block.c -- the route a call with INCCL_SCALE_BLOCK takes
 * (csrc/inccl_route.h inccl_route_block) against the column of DESIGN.md's
 * route table, written out here as data; then inccl_route_of composed with it
 * over the cases of route_table.c: per-block exponents never reach an engine's
 * own one-scale exchange (a2a, p2p, ll, mesh).  Host code only:
 *   gcc -std=gnu11 -fsanitize=address,undefined -I include -I container_inc_amd/csrc tests/c/route_block.c */
#include <stdio.h>

#include "inccl_route.h"

static const struct {
    enum inccl_route from, to;
} table[] = {
    {INCCL_ROUTE_FUSED, INCCL_ROUTE_FUSED},
    {INCCL_ROUTE_RSAG, INCCL_ROUTE_RSAG},
    {INCCL_ROUTE_AR, INCCL_ROUTE_AR},
    {INCCL_ROUTE_A2A, INCCL_ROUTE_AR},
    {INCCL_ROUTE_IPC_P2P, INCCL_ROUTE_AR},
    {INCCL_ROUTE_IPC_LL, INCCL_ROUTE_AR},
    {INCCL_ROUTE_IPC_MESH, INCCL_ROUTE_AR},
    {INCCL_ROUTE_RS, INCCL_ROUTE_RS},
    {INCCL_ROUTE_IPC_MESH_RS, INCCL_ROUTE_AR_SHARD},
    {INCCL_ROUTE_IPC_LL_RS, INCCL_ROUTE_AR_SHARD},
    {INCCL_ROUTE_IPC_P2P_RS, INCCL_ROUTE_AR_SHARD},
    {INCCL_ROUTE_AR_SHARD, INCCL_ROUTE_AR_SHARD},
};

static int stage_route(enum inccl_route r)
{
    return r == INCCL_ROUTE_FUSED || r == INCCL_ROUTE_RSAG || r == INCCL_ROUTE_AR || r == INCCL_ROUTE_RS ||
           r == INCCL_ROUTE_AR_SHARD;
}

int main(void)
{
    long cases = 0, bad = 0;
    const int nroutes = (int)INCCL_ROUTE_AR_SHARD + 1;   /* the enum's last value */
    if ((int)(sizeof(table) / sizeof(table[0])) != nroutes) {
        ++bad;
        printf("MISMATCH the table has %zu rows for %d routes\n", sizeof(table) / sizeof(table[0]), nroutes);
    }
    for (int r = 0; r < nroutes; ++r) {
        int rows = 0;
        for (size_t j = 0; j < sizeof(table) / sizeof(table[0]); ++j)
            if ((int)table[j].from == r) {
                ++rows;
                ++cases;
                if (inccl_route_block((enum inccl_route)r) != table[j].to) {
                    ++bad;
                    printf("MISMATCH inccl_route_block(%d) = %d, the table says %d\n", r,
                           (int)inccl_route_block((enum inccl_route)r), (int)table[j].to);
                }
            }
        if (rows != 1) {
            ++bad;
            printf("MISMATCH route %d has %d table rows\n", r, rows);
        }
    }
    /* composed with the route policy: fp32 (the mode's only kind), the sizes of route_table.c */
    static const size_t knobs[][2] = {{4096, 16384}, {16384, 4096}, {0, 0}};
    static const size_t ar_n[] = {1, 1000, 1024, 1025, 4096, 4097, 5000};
    static const size_t rs_shard[] = {64, 68, 67, 512, 516, 515, 1024, 1028, 2048, 2052, 2049, 4096, 4100, 4099};
    for (int op = INCCL_OP_ALLREDUCE; op <= INCCL_OP_REDUCE_SCATTER; ++op)
    for (int t = 0; t < 2; ++t)
    for (int e = 0; e < 6; ++e)
    for (int W = 1; W <= 4; ++W)
    for (int fs = 0; fs < 2; ++fs)
    for (int mrs = 0; mrs < 2; ++mrs)
    for (size_t kn = 0; kn < sizeof(knobs) / sizeof(knobs[0]); ++kn) {
        const int rs = op == INCCL_OP_REDUCE_SCATTER;
        const size_t nn = rs ? sizeof(rs_shard) / sizeof(rs_shard[0]) : sizeof(ar_n) / sizeof(ar_n[0]);
        for (size_t i = 0; i < nn; ++i) {
            const size_t n = rs ? rs_shard[i] * (size_t)W : ar_n[i];
            const enum inccl_route plain =
                inccl_route_of(op, INCCL_KIND_F32, t, e, W, fs, mrs, n, knobs[kn][0], knobs[kn][1]);
            const enum inccl_route got = inccl_route_block(plain);
            ++cases;
            const int fused_ok = (got == INCCL_ROUTE_FUSED) == (W == 1 && !fs);
            const int shard_ok = rs ? (got == INCCL_ROUTE_FUSED || got == INCCL_ROUTE_RS || got == INCCL_ROUTE_AR_SHARD)
                                    : (got == INCCL_ROUTE_FUSED || got == INCCL_ROUTE_RSAG || got == INCCL_ROUTE_AR);
            if (!stage_route(got) || !fused_ok || !shard_ok) {
                ++bad;
                printf("MISMATCH op %d transport %d engine %d W %d force_sharded %d mesh_rs %d n %zu: route %d -> %d\n",
                       op, t, e, W, fs, mrs, n, (int)plain, (int)got);
            }
        }
    }
    printf("route block %s: %ld cases, %ld mismatches\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
