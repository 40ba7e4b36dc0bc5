/* route_table.c -- the communicator's route policy (csrc/inccl_route.h) against
 * the table of DESIGN.md ("Route table"), written out here as data: the first
 * row that matches a case names its route.  Walks every operation x kind x
 * transport x engine x world x force_sharded x mesh_rs, with bucket sizes on both
 * sides of the small-bucket and ll thresholds and shards that are a multiple of
 * 64, of 4 only, and of neither.  Host code only:
 *   gcc -std=gnu11 -I include -I container_inc_amd/csrc tests/c/route_table.c */
#include <stdio.h>

#include "inccl_route.h"

enum { ANY = -1 };
#define BIT(x) (1 << (x))
#define K_F32 BIT(INCCL_KIND_F32)
#define K_16 (BIT(INCCL_KIND_BF16) | BIT(INCCL_KIND_F16))
#define K_ALL (K_F32 | K_16)
#define T_RCCL BIT(INCCL_TRANSPORT_RCCL)
#define T_LOCAL BIT(INCCL_TRANSPORT_LOCAL)
#define T_ALL (T_RCCL | T_LOCAL)
#define E(x) BIT(INCCL_ENGINE_##x)
#define E_ALL (E(RCCL) | E(P2P) | E(A2A) | E(LL) | E(MESH) | E(AR))
#define E_IPC (E(P2P) | E(LL) | E(MESH))
#define AR INCCL_OP_ALLREDUCE
#define RS INCCL_OP_REDUCE_SCATTER

/* sharded: W > 1 || force_sharded.  small: n <= rccl_ar_bytes / 4.  llfit:
 * n <= ll_max_bytes / 4.  wgt1: W > 1.  shard64 / shard4: (n / W) % 64 == 0 / % 4
 * == 0.  ANY: the column does not matter to the row. */
static const struct row {
    int op, kinds, transports, engines, sharded, small, llfit, wgt1, mesh_rs, shard64, shard4;
    enum inccl_route route;
} table[] = {
    {ANY, K_ALL, T_ALL, E_ALL, 0, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_FUSED},
    /* allreduce, fp32 */
    {AR, K_F32, T_RCCL, E(P2P), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_IPC_P2P},
    {AR, K_F32, T_RCCL, E(LL), 1, ANY, 1, 1, ANY, ANY, ANY, INCCL_ROUTE_IPC_LL},
    {AR, K_F32, T_RCCL, E(LL), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_IPC_P2P},
    {AR, K_F32, T_RCCL, E(MESH), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_IPC_MESH},
    {AR, K_F32, T_RCCL, E(AR), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_AR},
    {AR, K_F32, T_RCCL, E(RCCL), 1, 1, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_AR},
    {AR, K_F32, T_RCCL, E(RCCL), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_RSAG},
    {AR, K_F32, T_RCCL, E(A2A), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_A2A},
    {AR, K_F32, T_LOCAL, E(AR), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_AR},
    {AR, K_F32, T_LOCAL, E_ALL, 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_RSAG},
    /* allreduce, bf16 / fp16: in-process "ar" takes RSAG, a2a and ll take AR */
    {AR, K_16, T_LOCAL, E_ALL, 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_RSAG},
    {AR, K_16, T_RCCL, E(RCCL), 1, 1, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_AR},
    {AR, K_16, T_RCCL, E(RCCL), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_RSAG},
    {AR, K_16, T_RCCL, E(MESH), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_IPC_MESH},
    {AR, K_16, T_RCCL, E(P2P), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_IPC_P2P},
    {AR, K_16, T_RCCL, E(AR) | E(A2A) | E(LL), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_AR},
    /* reduce-scatter, every kind: never the small-bucket route */
    {RS, K_ALL, T_ALL, E(RCCL), 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_RS},
    {RS, K_ALL, T_LOCAL, E_ALL, 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_RS},
    {RS, K_ALL, T_RCCL, E(MESH), 1, ANY, ANY, ANY, 1, 1, ANY, INCCL_ROUTE_IPC_MESH_RS},
    {RS, K_F32, T_RCCL, E(LL), 1, ANY, 1, ANY, ANY, ANY, 1, INCCL_ROUTE_IPC_LL_RS},
    {RS, K_ALL, T_RCCL, E_IPC, 1, ANY, ANY, ANY, ANY, ANY, 1, INCCL_ROUTE_IPC_P2P_RS},
    {RS, K_ALL, T_RCCL, E_ALL, 1, ANY, ANY, ANY, ANY, ANY, ANY, INCCL_ROUTE_AR_SHARD},
};

static int col(int want, int have) { return want == ANY || want == have; }

int main(void)
{
    static const int kinds[] = {INCCL_KIND_F32, INCCL_KIND_BF16, INCCL_KIND_F16};
    static const size_t knobs[][2] = {{4096, 16384}, {16384, 4096}, {0, 0}};   /* rccl_ar_bytes, ll_max_bytes */
    /* allreduce: elements around 1024 and 4096 (the thresholds / 4); reduce-scatter:
     * shards, n = W * shard, around the same thresholds for W = 1, 2, 3 */
    static const size_t ar_n[] = {1, 1000, 1024, 1025, 4096, 4097, 5000};
    static const size_t rs_shard[] = {64, 68, 67, 512, 516, 515, 1024, 1028, 2048, 2052, 2049, 4096, 4100, 4099};
    long cases = 0, bad = 0;
    for (int op = AR; op <= RS; ++op)
    for (int ki = 0; ki < 3; ++ki)
    for (int t = 0; t < 2; ++t)
    for (int e = 0; e < 6; ++e)
    for (int W = 1; W <= 3; ++W)
    for (int fs = 0; fs < 2; ++fs)
    for (int mrs = 0; mrs < 2; ++mrs)
    for (size_t kn = 0; kn < sizeof(knobs) / sizeof(knobs[0]); ++kn) {
        const size_t *ns = op == AR ? ar_n : rs_shard;
        const size_t nn = op == AR ? sizeof(ar_n) / sizeof(ar_n[0]) : sizeof(rs_shard) / sizeof(rs_shard[0]);
        for (size_t i = 0; i < nn; ++i) {
            const size_t n = op == AR ? ns[i] : ns[i] * (size_t)W, shard = n / (size_t)W;
            const int sharded = W > 1 || fs, small = n <= knobs[kn][0] / 4, llfit = n <= knobs[kn][1] / 4;
            const struct row *r = NULL;
            for (size_t j = 0; j < sizeof(table) / sizeof(table[0]) && !r; ++j) {
                const struct row *q = &table[j];
                if (col(q->op, op) && (q->kinds & BIT(kinds[ki])) && (q->transports & BIT(t)) && (q->engines & BIT(e)) &&
                    col(q->sharded, sharded) && col(q->small, small) && col(q->llfit, llfit) && col(q->wgt1, W > 1) &&
                    col(q->mesh_rs, mrs) && col(q->shard64, shard % 64 == 0) && col(q->shard4, shard % 4 == 0))
                    r = q;
            }
            const int got = (int)inccl_route_of(op, kinds[ki], t, e, W, fs, mrs, n, knobs[kn][0], knobs[kn][1]);
            ++cases;
            if (!r || got != (int)r->route) {
                ++bad;
                printf("MISMATCH op %d kind %d transport %d engine %d W %d force_sharded %d mesh_rs %d n %zu "
                       "rccl_ar_bytes %zu ll_max_bytes %zu: route %d, table row %d says %d\n",
                       op, kinds[ki], t, e, W, fs, mrs, n, knobs[kn][0], knobs[kn][1], got,
                       r ? (int)(r - table) : -1, r ? (int)r->route : -1);
            }
        }
    }
    static const int ipc[6] = {0 /* rccl */, 1 /* p2p */, 0 /* a2a */, 1 /* ll */, 1 /* mesh */, 0 /* ar */};
    for (int e = 0; e < 6; ++e)
        if (inccl_engine_is_ipc(e) != ipc[e]) {
            ++bad;
            printf("MISMATCH inccl_engine_is_ipc(%d)\n", e);
        }
    printf("route table %s: %ld cases, %ld mismatches\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
