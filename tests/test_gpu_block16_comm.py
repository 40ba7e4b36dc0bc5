"""The packed 16-bit wire through the communicator (gpu): inccl_comm_set_wire
(INCCL_WIRE_P16) on the INCCL_SCALE_BLOCK calls of inccl_allreduce_f32,
inccl_allreduce_f32_pipelined and inccl_reduce_scatter_f32, bit-exact against
tests/block16_ref.py (a NaN compares equal to a NaN whatever its payload) -- over
the in-process transport (ranks = threads), RCCL at world 1 with the sharded
paths forced and one process per rank on the IPC engines.  On the same
communicator, INCCL_SCALE_AUTO and fixed-exponent calls give the oracle's
results with the wire set, and after set_wire(INCCL_WIRE_Q32) a block-scaled
call gives tests/block_ref.py's result again.  Every communicator and group is
destroyed and every thread and process joined before a test returns."""
import multiprocessing as mp
import socket
import threading

import numpy as np
import pytest

import block16_ref
import block_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

R = 2
N_EXTRA = 2341


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
    """(name, n, what, chunks, average, nonfinite_nan, inf_at) of one world; the
    shards of 1001 elements are odd: a packed reduce-scatter takes AR_SHARD there"""
    cases = [("allreduce", 10533, "ar", 1, False, False, None),
             ("rs-aligned", world * 4096, "rs", 1, False, False, None),
             ("rs-odd", world * 1001, "rs", 1, False, False, None),
             ("pipelined", 3 * world * 64 * 5 + 77, "ar", 3, False, False, None),
             ("inf-saturates", 2341, "ar", 1, False, False, 256 * 2 + 5),
             ("inf-nan", 2341, "ar", 1, False, True, 256 * 2 + 5),
             ("inf-nan-rs", world * 1001, "rs", 1, False, True, 256 * 2 + 5)]
    if world in (2, 4):
        cases += [("average", 10533, "ar", 1, True, False, None), ("average-rs", world * 1001, "rs", 1, True, False, None),
                  ("average-rs-aligned", world * 4096, "rs", 1, True, False, None)]
    return cases


def _reference(orc, world, case, seed):
    _, n, what, _, average, nan, inf_at = case
    per_rank, every = _buckets(world, n, seed, inf_at)
    shift = world.bit_length() - 1 if average else 0
    want, _ = block16_ref.reduce_f32_block16(orc, every, world * R, out_shift=shift, nonfinite_nan=nan)
    return per_rank, want


def _extras_reference(orc, world, seed):
    """the calls the wire must leave alone: (per_rank, auto, fixed k = 4, 32-bit block)"""
    per_rank, every = _buckets(world, N_EXTRA, seed)
    auto = orc.reduce_f32(every, orc.choose_scale(orc.absmax(every), world * R))
    block, _ = block_ref.reduce_f32_block(orc, every, world * R)
    return per_rank, auto, orc.reduce_f32(every, 4), block


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


def _run_extras(comm, inccl, torch, dev, srcs):
    """with the wire at P16: an auto-scaled and a fixed-exponent call; then at Q32 a block-scaled one"""
    comm.set_average(False)
    comm.set_nonfinite(False)
    ts = [torch.from_numpy(x).to(dev) for x in srcs]
    torch.cuda.synchronize()
    assert comm.wire == inccl.WIRE_P16
    out = []
    for k in (inccl.SCALE_AUTO, 4):
        out.append(comm.allreduce_f32(ts, scale_exp=k, stream=comm.stream))
    comm.set_wire(inccl.WIRE_Q32)
    assert comm.wire == inccl.WIRE_Q32
    out.append(comm.allreduce_f32(ts, scale_exp=inccl.SCALE_BLOCK, stream=comm.stream))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _run_all(comm, inccl, torch, dev, world, rank, refs, extra):
    """every case of one rank on one communicator: a fresh communicator's wire is
    Q32, an unknown wire is refused and leaves it as it was"""
    from container_inc_amd._lib import IncclError
    assert comm.wire == inccl.WIRE_Q32
    with pytest.raises(IncclError, match="rc=-1.*set_wire"):
        comm.set_wire(2)
    comm.set_wire(inccl.WIRE_P16)
    res = [_run_case(comm, inccl, torch, dev, refs[i][0][rank], c, world, rank) for i, c in enumerate(_cases(world))]
    return res, _run_extras(comm, inccl, torch, dev, extra[0][rank])


def _expect(want, case, world, rank):
    if case[2] != "rs":
        return want
    shard = case[1] // world
    return want[rank * shard:(rank + 1) * shard]


def _judge(world, rank, refs, extra, res, ext):
    bad = []
    for c, (_, want), got in zip(_cases(world), refs, res):
        try:
            _same(got, _expect(want, c, world, rank))
        except AssertionError as e:
            bad.append(f"world {world} rank {rank} case {c[0]}: {str(e)[:300]}")
    for name, want, got in zip(("auto", "fixed", "q32-block"), extra[1:], ext):
        try:
            _same(got, want)
        except AssertionError as e:
            bad.append(f"world {world} rank {rank} wire-independent call {name}: {str(e)[:300]}")
    return bad


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
def test_packed_wire_local(gpu, orc, world):
    """allreduce, reduce-scatter (shards of 4096 and of 1001 elements), a call
    with three chunks (ignored on this wire), the mean (worlds 2 and 4) and both
    non-finite modes, over the in-process transport; world 1 is the fused kernel"""
    import torch
    from container_inc_amd import inccl
    refs = [_reference(orc, world, c, 1600 + 100 * world + i) for i, c in enumerate(_cases(world))]
    extra = _extras_reference(orc, world, 1690 + world)

    def rank(r):
        grp = inccl.inccl_group_create_local(world, r, f"pack16-{world}")
        comm = inccl.inccl_communicator_create(grp, 0)
        try:
            res = _run_all(comm, inccl, torch, gpu, world, r, refs, extra)
            comm.barrier()
        finally:
            comm.destroy()
            grp.destroy()
        return res

    bad = []
    for r, (res, ext) in enumerate(_run_ranks(world, rank)):
        bad += _judge(world, r, refs, extra, res, ext)
    assert not bad, bad


@pytest.mark.parametrize("engine", ["rccl", "ar"])
def test_packed_wire_rccl_world1(gpu, orc, monkeypatch, engine):
    """RCCL at world 1 with the sharded paths forced: "rccl" would take RSAG and
    RS, and on this wire takes AR, RS (even shards) and AR_SHARD (odd ones); "ar"
    takes AR and AR_SHARD (ncclReduceScatter / ncclAllReduce are real calls)"""
    import torch
    from container_inc_amd import inccl
    monkeypatch.setenv("INCCL_FORCE_RCCL", "1")
    monkeypatch.setenv("INCCL_FORCE_SHARDED", "1")
    monkeypatch.setenv("INCCL_MASTER_PORT", "0")
    monkeypatch.setenv("INCCL_RCCL_AR_BYTES", "0")
    refs = [_reference(orc, 1, c, 2500 + i) for i, c in enumerate(_cases(1))]
    extra = _extras_reference(orc, 1, 2590)
    grp = inccl.inccl_group_create(1, 0, "127.0.0.1")
    assert grp is not None and grp.transport == "rccl"
    comm = inccl.inccl_communicator_create(grp, 1 << 20)
    try:
        comm.set_engine(engine)
        res, ext = _run_all(comm, inccl, torch, gpu, 1, 0, refs, extra)
    finally:
        comm.destroy()
        grp.destroy()
    bad = _judge(1, 0, refs, extra, res, ext)
    assert not bad, bad


# ---- one process per rank on one GPU: the IPC engines' int32 allreduce carries the words ----
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
        refs = [_reference(O, world, c, 2900 + 10 * world + i) for i, c in enumerate(_cases(world))]
        extra = _extras_reference(O, world, 2990 + world)
        grp = inccl.inccl_group_create(world, rank, "127.0.0.1", port=port, device=0)
        assert grp is not None, "group create failed"
        comm = inccl.inccl_communicator_create(grp, 0)
        assert comm is not None and comm.engine == engine
        try:
            res, ext = _run_all(comm, inccl, torch, dev, world, rank, refs, extra)
        finally:
            comm.destroy()
            grp.destroy()
        q.put((rank, _judge(world, rank, refs, extra, res, ext), None))
    except BaseException as e:  # noqa: BLE001
        q.put((rank, None, repr(e)))


@pytest.mark.parametrize("world,engine", [(2, "p2p"), (2, "mesh"), (2, "ll")])
def test_packed_wire_multiprocess(gpu, world, engine):
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
