/* route_packed.c -- the route an INCCL_SCALE_BLOCK call takes on the packed
 * 16-bit wire (csrc/inccl_route.h inccl_route_packed, applied after
 * inccl_route_block) against the column of DESIGN.md's route table, written
 * out here as data for a shard of n / W elements that is even and one that is
 * odd; then inccl_route_of, inccl_route_block and it composed over the cases of
 * route_table.c: a packed call never takes RSAG (a word cannot be dequantised
 * before every rank's contribution is in it) and takes RS only where a shard is
 * whole words.  Host code only:
 *   gcc -std=gnu11 -fsanitize=address,undefined -I include -I container_inc_amd/csrc tests/c/route_packed.c */
#include <stdio.h>

#include "inccl_route.h"

static const struct {
    enum inccl_route from, even, odd;
} table[] = {
    {INCCL_ROUTE_FUSED, INCCL_ROUTE_FUSED, INCCL_ROUTE_FUSED},
    {INCCL_ROUTE_RSAG, INCCL_ROUTE_AR, INCCL_ROUTE_AR},
    {INCCL_ROUTE_AR, INCCL_ROUTE_AR, INCCL_ROUTE_AR},
    {INCCL_ROUTE_RS, INCCL_ROUTE_RS, INCCL_ROUTE_AR_SHARD},
    {INCCL_ROUTE_AR_SHARD, INCCL_ROUTE_AR_SHARD, INCCL_ROUTE_AR_SHARD},
    /* never handed over (inccl_route_block maps them away): unchanged */
    {INCCL_ROUTE_A2A, INCCL_ROUTE_A2A, INCCL_ROUTE_A2A},
    {INCCL_ROUTE_IPC_P2P, INCCL_ROUTE_IPC_P2P, INCCL_ROUTE_IPC_P2P},
    {INCCL_ROUTE_IPC_LL, INCCL_ROUTE_IPC_LL, INCCL_ROUTE_IPC_LL},
    {INCCL_ROUTE_IPC_MESH, INCCL_ROUTE_IPC_MESH, INCCL_ROUTE_IPC_MESH},
    {INCCL_ROUTE_IPC_MESH_RS, INCCL_ROUTE_IPC_MESH_RS, INCCL_ROUTE_IPC_MESH_RS},
    {INCCL_ROUTE_IPC_LL_RS, INCCL_ROUTE_IPC_LL_RS, INCCL_ROUTE_IPC_LL_RS},
    {INCCL_ROUTE_IPC_P2P_RS, INCCL_ROUTE_IPC_P2P_RS, INCCL_ROUTE_IPC_P2P_RS},
};

int main(void)
{
    long cases = 0, bad = 0;
    const int nroutes = (int)INCCL_ROUTE_AR_SHARD + 1;   /* the enum's last value */
    if ((int)(sizeof(table) / sizeof(table[0])) != nroutes) {
        ++bad;
        printf("MISMATCH the table has %zu rows for %d routes\n", sizeof(table) / sizeof(table[0]), nroutes);
    }
    static const size_t shards[] = {1, 2, 3, 64, 67, 68, 1000, 1001, 4096, 4099};
    for (int r = 0; r < nroutes; ++r) {
        int rows = 0;
        for (size_t j = 0; j < sizeof(table) / sizeof(table[0]); ++j) {
            if ((int)table[j].from != r) continue;
            ++rows;
            for (int W = 1; W <= 8; ++W)
                for (size_t i = 0; i < sizeof(shards) / sizeof(shards[0]); ++i)
                    for (size_t rag = 0; rag < 2; ++rag) {   /* an allreduce's n need not split into W */
                        const size_t n = shards[i] * (size_t)W + (rag && W > 1 ? 1 : 0);
                        const enum inccl_route want = (n / (size_t)W) % 2 ? table[j].odd : table[j].even;
                        const enum inccl_route got = inccl_route_packed((enum inccl_route)r, n, W);
                        ++cases;
                        if (got != want) {
                            ++bad;
                            printf("MISMATCH inccl_route_packed(%d, %zu, %d) = %d, the table says %d\n", r, n, W, (int)got,
                                   (int)want);
                        }
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
            const enum inccl_route got = inccl_route_packed(inccl_route_block(plain), n, W);
            ++cases;
            const int fused_ok = (got == INCCL_ROUTE_FUSED) == (W == 1 && !fs);
            const int shard_ok = rs ? (got == INCCL_ROUTE_FUSED || got == INCCL_ROUTE_AR_SHARD ||
                                       (got == INCCL_ROUTE_RS && (n / (size_t)W) % 2 == 0))
                                    : (got == INCCL_ROUTE_FUSED || got == INCCL_ROUTE_AR);
            if (!fused_ok || !shard_ok) {
                ++bad;
                printf("MISMATCH op %d transport %d engine %d W %d force_sharded %d mesh_rs %d n %zu: route %d -> %d\n",
                       op, t, e, W, fs, mrs, n, (int)plain, (int)got);
            }
        }
    }
    printf("route packed %s: %ld cases, %ld mismatches\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
