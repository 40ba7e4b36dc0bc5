/* inccl_route.h -- which engine carries a bucket: the one statement of the
 * communicator's route policy (Multi-GPU, "Route table").  Pure C:
 * no HIP, no communicator, so a stand-alone program can walk the whole table
 * (tests/c/route_table.c). */
#ifndef INCCL_ROUTE_H
#define INCCL_ROUTE_H

#include <stddef.h>
#include <stdint.h>

#include "inccl_amd.h"

#define INCCL_TRANSPORT_RCCL 0
#define INCCL_TRANSPORT_LOCAL 1
/* communicator-level exchange engine (group transport RCCL only) */
#define INCCL_ENGINE_RCCL 0
#define INCCL_ENGINE_P2P 1
#define INCCL_ENGINE_A2A 2
#define INCCL_ENGINE_LL 3
#define INCCL_ENGINE_MESH 4
#define INCCL_ENGINE_AR 5

#define INCCL_OP_ALLREDUCE 0
#define INCCL_OP_REDUCE_SCATTER 1

enum inccl_route {
    INCCL_ROUTE_FUSED,        /* one rank: quant + sum + dequant in one kernel */
    INCCL_ROUTE_RSAG,         /* quant -> int32 reduce-scatter -> dequant shard -> all-gather */
    INCCL_ROUTE_AR,           /* quant -> the engine's int32 allreduce -> dequant */
    INCCL_ROUTE_A2A,          /* quant -> grouped send/recv of shards -> sum + dequant -> all-gather */
    INCCL_ROUTE_IPC_P2P,      /* p2p.c */
    INCCL_ROUTE_IPC_LL,       /* ll.c */
    INCCL_ROUTE_IPC_MESH,     /* mesh.c */
    INCCL_ROUTE_RS,           /* quant -> int32 reduce-scatter -> dequant shard */
    INCCL_ROUTE_IPC_MESH_RS,
    INCCL_ROUTE_IPC_LL_RS,
    INCCL_ROUTE_IPC_P2P_RS,
    INCCL_ROUTE_AR_SHARD      /* the AR route, own shard dequantised */
};

/* the engines that exchange over HIP IPC buffers without RCCL */
static inline int inccl_engine_is_ipc(int engine)
{
    return engine == INCCL_ENGINE_P2P || engine == INCCL_ENGINE_LL || engine == INCCL_ENGINE_MESH;
}

/* n: elements of the bucket.  Everything here is shared by the ranks (the knobs
 * are agreed when the communicator is made), so every rank takes the same route.
 * Kept on purpose as the three former bodies had them, not fixed here:
 *  - an "ar" communicator on the in-process transport takes AR for fp32 and
 *    RSAG for bf16 / fp16;
 *  - "a2a" and "ll" have fp32-only routes: their 16-bit buckets take AR;
 *  - the rccl engine's small-bucket AR route serves allreduce, never
 *    reduce-scatter;
 *  - the fp32 allreduce takes ll only for W > 1, reduce-scatter does not ask. */
static inline enum inccl_route inccl_route_of(int op, int kind, int transport, int engine, int W, int force_sharded,
                                              int mesh_rs, size_t n, size_t rccl_ar_bytes, size_t ll_max_bytes)
{
    if (W == 1 && !force_sharded) return INCCL_ROUTE_FUSED;
    const int rccl = transport == INCCL_TRANSPORT_RCCL;
    const int small = engine == INCCL_ENGINE_RCCL && rccl && n <= rccl_ar_bytes / sizeof(int32_t);
    const int llfit = engine == INCCL_ENGINE_LL && n <= ll_max_bytes / sizeof(float);
    if (op == INCCL_OP_REDUCE_SCATTER) {
        const size_t shard = n / (size_t)W;
        if (engine == INCCL_ENGINE_RCCL || !rccl) return INCCL_ROUTE_RS;
        if (mesh_rs && engine == INCCL_ENGINE_MESH && !(shard % 64)) return INCCL_ROUTE_IPC_MESH_RS;
        if (inccl_engine_is_ipc(engine) && !(shard & 3))
            return kind == INCCL_KIND_F32 && llfit ? INCCL_ROUTE_IPC_LL_RS : INCCL_ROUTE_IPC_P2P_RS;
        return INCCL_ROUTE_AR_SHARD;
    }
    if (kind == INCCL_KIND_F32) {
        if (inccl_engine_is_ipc(engine) && rccl) {
            if (llfit && W > 1) return INCCL_ROUTE_IPC_LL;
            return engine == INCCL_ENGINE_MESH ? INCCL_ROUTE_IPC_MESH : INCCL_ROUTE_IPC_P2P;
        }
        if (engine == INCCL_ENGINE_AR || small) return INCCL_ROUTE_AR;
        if (engine == INCCL_ENGINE_A2A && rccl) return INCCL_ROUTE_A2A;
        return INCCL_ROUTE_RSAG;
    }
    if ((engine == INCCL_ENGINE_RCCL && !small) || !rccl) return INCCL_ROUTE_RSAG;
    if (engine == INCCL_ENGINE_MESH) return INCCL_ROUTE_IPC_MESH;
    if (engine == INCCL_ENGINE_P2P) return INCCL_ROUTE_IPC_P2P;
    return INCCL_ROUTE_AR;
}

/* The route a call with INCCL_SCALE_BLOCK takes instead of `route`: per-block
 * exponents travel through the stage helpers only (quantise at the agreed words
 * -> an int32 exchange -> dequantise), so the routes built from those stay, and
 * the engines' own exchanges, which carry one scale per call (a2a's fused sum +
 * dequantise, the p2p / ll / mesh kernels), give way to the same engine's int32
 * allreduce.  FUSED stays: it becomes the one-pass per-block kernel. */
static inline enum inccl_route inccl_route_block(enum inccl_route route)
{
    switch (route) {
        case INCCL_ROUTE_A2A:
        case INCCL_ROUTE_IPC_P2P:
        case INCCL_ROUTE_IPC_LL:
        case INCCL_ROUTE_IPC_MESH: return INCCL_ROUTE_AR;
        case INCCL_ROUTE_IPC_MESH_RS:
        case INCCL_ROUTE_IPC_LL_RS:
        case INCCL_ROUTE_IPC_P2P_RS: return INCCL_ROUTE_AR_SHARD;
        default: return route;
    }
}

/* The route an INCCL_SCALE_BLOCK call takes on the packed 16-bit wire
 * (INCCL_WIRE_P16), applied after inccl_route_block.  Two elements share an
 * int32 wire word and a word cannot be dequantised before every rank's
 * contribution is in it, so:
 *  - RSAG becomes AR: the reduced words are what travels, both halves of the
 *    exchange then move 2 bytes an element (a gather of dequantised fp32 shards
 *    would move 4), and `chunks` is ignored;
 *  - RS stays while a shard of n / W elements is whole words, else AR_SHARD,
 *    whose dequantise may start at a word's high lane;
 *  - FUSED, AR and AR_SHARD are unchanged. */
static inline enum inccl_route inccl_route_packed(enum inccl_route route, size_t n, int W)
{
    switch (route) {
        case INCCL_ROUTE_RSAG: return INCCL_ROUTE_AR;
        case INCCL_ROUTE_RS: return (n / (size_t)W) % 2 ? INCCL_ROUTE_AR_SHARD : INCCL_ROUTE_RS;
        default: return route;
    }
}

#endif
