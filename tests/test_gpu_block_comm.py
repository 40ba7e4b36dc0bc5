"""Per-block auto scaling through the communicator (gpu): scale_exp =
INCCL_SCALE_BLOCK on inccl_allreduce_f32, inccl_allreduce_f32_pipelined and
inccl_reduce_scatter_f32, bit-exact against tests/block_ref.py (a NaN compares
equal to a NaN whatever its payload) -- over the in-process transport (ranks =
threads), RCCL at world 1 and one process per rank on the IPC engines, whose
block-scaled calls travel through the engine's int32 allreduce.  Every
communicator and group is destroyed and every thread and process joined before
a test returns."""
import multiprocessing as mp
import socket
import threading

import numpy as np
import pytest

import block_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

R = 2


def _same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn)
    np.testing.assert_array_equal(got.view(np.uint32)[~wn], want.view(np.uint32)[~wn])


def _buckets(world, n, seed, inf_at=None):
    """[rank][r] buckets whose blocks span 10^[-12, 6), block 1 all zero; inf_at:
    +Inf at that element of the last rank's last bucket"""
    bufs = block_ref.mixed_buckets(np.random.default_rng(seed), n, world * R, zero_block=1)
    if inf_at is not None:
        bufs[-1][inf_at] = np.float32(np.inf)
    return [bufs[r * R:(r + 1) * R] for r in range(world)], bufs


def _cases(world):
    """(name, n, what, chunks, average, nonfinite_nan, inf_at) of one world"""
    cases = [("allreduce", 10533, "ar", 1, False, False, None),
             ("rs-aligned", world * 4096, "rs", 1, False, False, None),
             ("rs-ragged", world * 1001, "rs", 1, False, False, None),
             ("pipelined", 3 * world * 64 * 5 + 77, "ar", 3, False, False, None),
             ("inf-saturates", 2341, "ar", 1, False, False, 256 * 2 + 5),
             ("inf-nan", 2341, "ar", 1, False, True, 256 * 2 + 5),
             ("inf-nan-rs", world * 1001, "rs", 1, False, True, 256 * 2 + 5)]
    if world in (2, 4):
        cases += [("average", 10533, "ar", 1, True, False, None), ("average-rs", world * 1001, "rs", 1, True, False, None),
                  ("average-pipelined", 3 * world * 64 * 5 + 77, "ar", 3, True, False, None)]
    return cases


def _reference(orc, world, case, seed):
    _, n, what, _, average, nan, inf_at = case
    per_rank, every = _buckets(world, n, seed, inf_at)
    shift = world.bit_length() - 1 if average else 0
    want, _ = block_ref.reduce_f32_block(orc, every, world * R, out_shift=shift, nonfinite_nan=nan)
    return per_rank, want


def _run_case(comm, inccl, torch, dev, srcs, case, world, rank):
    _, n, what, chunks, average, nan, _ = case
    comm.set_average(average)
    comm.set_nonfinite(nan)
    ts = [torch.from_numpy(x).to(dev) for x in srcs]
    torch.cuda.synchronize()
    if what == "rs":
        out = comm.reduce_scatter(ts, scale_exp=inccl.SCALE_BLOCK, stream=comm.stream)
    else:
        out = comm.allreduce_f32(ts, scale_exp=inccl.SCALE_BLOCK, chunks=chunks, stream=comm.stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _expect(want, case, world, rank):
    if case[2] != "rs":
        return want
    shard = case[1] // world
    return want[rank * shard:(rank + 1) * shard]


def _run_ranks(world, fn):
    errs, out = [None] * world, [None] * world

    def body(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            errs[r] = e

    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "a rank thread did not finish"
    for e in errs:
        if e is not None:
            raise e
    return out


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_block_scale_local(gpu, orc, world):
    """allreduce, reduce-scatter (shards of 4096 and of 1001 elements: the second
    starts its ranks' shards off the quad grid), three pipelined chunks, the mean
    (worlds 2 and 4) and both non-finite modes, over the in-process transport"""
    import torch
    from container_inc_amd import inccl
    cases = _cases(world)
    refs = [_reference(orc, world, c, 100 * world + i) for i, c in enumerate(cases)]

    def rank(r):
        grp = inccl.inccl_group_create_local(world, r, f"block-{world}")
        comm = inccl.inccl_communicator_create(grp, 0)
        try:
            res = [_run_case(comm, inccl, torch, gpu, refs[i][0][r], c, world, r) for i, c in enumerate(cases)]
            comm.barrier()
        finally:
            comm.destroy()
            grp.destroy()
        return res

    for r, res in enumerate(_run_ranks(world, rank)):
        for c, (_, want), got in zip(cases, refs, res):
            try:
                _same(got, _expect(want, c, world, r))
            except AssertionError as e:
                raise AssertionError(f"world {world} rank {r} case {c[0]}: {e}") from None


@pytest.mark.parametrize("engine", ["rccl", "ar"])
def test_block_scale_rccl_world1(gpu, orc, monkeypatch, engine):
    """RCCL at world 1 with the sharded paths forced: "rccl" takes RSAG (the
    small-bucket route off) and RS, "ar" takes AR and AR_SHARD (one rank: the words need no
    exchange; ncclReduceScatter / ncclAllGather / ncclAllReduce are real calls)"""
    import torch
    from container_inc_amd import inccl
    monkeypatch.setenv("INCCL_FORCE_RCCL", "1")
    monkeypatch.setenv("INCCL_FORCE_SHARDED", "1")
    monkeypatch.setenv("INCCL_MASTER_PORT", "0")
    monkeypatch.setenv("INCCL_RCCL_AR_BYTES", "0")
    grp = inccl.inccl_group_create(1, 0, "127.0.0.1")
    assert grp is not None and grp.transport == "rccl"
    comm = inccl.inccl_communicator_create(grp, 1 << 20)
    try:
        comm.set_engine(engine)
        for i, c in enumerate(_cases(1)):
            per_rank, want = _reference(orc, 1, c, 500 + i)
            _same(_run_case(comm, inccl, torch, gpu, per_rank[0], c, 1, 0), want)
    finally:
        comm.destroy()
        grp.destroy()


def test_block_scale_refusals(gpu):
    """bf16 / fp16 buckets, the host-memory allreduce and prepared ops refuse the
    mode with INCCL_ERR_ARG and a text that names it; dst stays as it was"""
    import torch
    from container_inc_amd import inccl
    from container_inc_amd._lib import IncclError
    grp = inccl.inccl_group_create_local(1, 0, "block-refuse")
    comm = inccl.inccl_communicator_create(grp, 0)
    try:
        n = 1024
        for dt, call in ((torch.bfloat16, comm.allreduce_bf16), (torch.float16, comm.allreduce_f16),
                         (torch.bfloat16, comm.reduce_scatter), (torch.float16, comm.reduce_scatter)):
            x = torch.ones(n, dtype=dt, device=gpu)
            out = torch.full((n,), 7.0, dtype=dt, device=gpu)
            torch.cuda.synchronize()
            with pytest.raises(IncclError, match=r"rc=-1.*INCCL_SCALE_BLOCK"):
                call([x], out=out, scale_exp=inccl.SCALE_BLOCK, stream=comm.stream)
            torch.cuda.synchronize()
            assert (out.float().cpu().numpy() == 7.0).all()
        x = torch.ones(n, dtype=torch.float32, device=gpu)
        out = torch.full((n,), 7.0, dtype=torch.float32, device=gpu)
        torch.cuda.synchronize()
        with pytest.raises(IncclError, match="INCCL_SCALE_BLOCK"):
            comm.prepare_allreduce_f32([x], out=out, scale_exp=inccl.SCALE_BLOCK, stream=comm.stream)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 7.0).all()
        src, dst = np.ones(4096, np.float32), np.full(4096, 7.0, np.float32)
        with pytest.raises(IncclError, match=r"rc=-1.*INCCL_SCALE_BLOCK"):
            comm.allreduce_f32_host(src, dst, scale_exp=inccl.SCALE_BLOCK)
        assert (dst == 7.0).all()
    finally:
        comm.destroy()
        grp.destroy()


# ---- one process per rank on one GPU: the IPC engines' AR / AR_SHARD mapping ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, engine, q):
    try:
        import os
        import sys
        os.environ["INCCL_ENGINE"] = engine
        os.environ["INCCL_DEVICE"] = "0"
        os.environ["INCCL_BOOT_TIMEOUT"] = "120"
        sys.path.insert(0, ROOT)
        import torch
        from container_inc_amd import inccl
        from oracle import oracle as O
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        grp = inccl.inccl_group_create(world, rank, "127.0.0.1", port=port, device=0)
        assert grp is not None, "group create failed"
        comm = inccl.inccl_communicator_create(grp, 0)
        assert comm is not None and comm.engine == engine
        bad = []
        try:
            for i, c in enumerate(_cases(world)):
                per_rank, want = _reference(O, world, c, 900 + 10 * world + i)
                got = _run_case(comm, inccl, torch, dev, per_rank[rank], c, world, rank)
                try:
                    _same(got, _expect(want, c, world, rank))
                except AssertionError as e:
                    bad.append(f"{c[0]}: {str(e)[:300]}")
        finally:
            comm.destroy()
            grp.destroy()
        q.put((rank, bad, None))
    except BaseException as e:  # noqa: BLE001
        q.put((rank, None, repr(e)))


@pytest.mark.parametrize("world,engine", [(2, "p2p"), (3, "mesh")])
def test_block_scale_multiprocess(gpu, world, engine):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_rank_main, args=(r, world, port, engine, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r, bad, err = q.get(timeout=240)
            res[r] = (bad, err)
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
                p.join()
    for r in range(world):
        bad, err = res[r]
        assert err is None, f"rank {r}: {err}"
        assert not bad, f"rank {r}: {bad}"
    assert [p.exitcode for p in ps] == [0] * world, [p.exitcode for p in ps]
