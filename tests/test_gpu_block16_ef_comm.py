"""Error feedback through the communicator (gpu): inccl_allreduce_f32_ef on the
packed 16-bit wire, three chained steps, every rank's result and residuals bit
for bit against tests/block16_ef_ref.py (a NaN compares equal to a NaN whatever
its payload) -- over the in-process transport (ranks = threads), RCCL at world 1
with the sharded paths forced and one process per rank on the IPC engines.
What the call refuses it refuses before it touches dst or a residual.  On the
same communicator a plain INCCL_SCALE_BLOCK call afterwards gives
tests/block16_ref.py's result, and after set_wire(INCCL_WIRE_Q32)
tests/block_ref.py's.  Every communicator and group is destroyed and every
thread and process joined before a test returns."""
import multiprocessing as mp

import numpy as np
import pytest

import block16_ef_ref as ef
import block16_ref
import block_ref
from conftest import ROOT
from test_gpu_block16_comm import _free_port, _run_ranks, _same

pytestmark = pytest.mark.gpu

R = 2
STEPS = 3


def _cases(world):
    """(n, average): 2341, and 1024 W + 6 whose shards are an odd count of
    words; the mean for the power-of-two worlds"""
    ns = (2341, 1024 * world + 6)
    return [(n, avg) for n in ns for avg in ((False, True) if world in (2, 4) else (False,))]


def _reference(orc, world, case, seed):
    """([step][rank][r] buckets, [step] (y, [rank][r] residuals)) of one case"""
    n, average = case
    steps = [block_ref.mixed_buckets(np.random.default_rng(seed + t), n, world * R, zero_block=1) for t in range(STEPS)]
    shift = world.bit_length() - 1 if average else 0
    chain = ef.chain(orc, steps, world * R, out_shift=shift)
    split = lambda xs: [xs[r * R:(r + 1) * R] for r in range(world)]   # noqa: E731
    return [split(s) for s in steps], [(y, split(res)) for y, res, _ in chain]


def _extras_reference(orc, world, seed):
    """plain SCALE_BLOCK calls after the EF ones: (per_rank, packed wire, 32-bit wire)"""
    every = block_ref.mixed_buckets(np.random.default_rng(seed), 2341, world * R, zero_block=1)
    return ([every[r * R:(r + 1) * R] for r in range(world)], block16_ref.reduce_f32_block16(orc, every, world * R)[0],
            block_ref.reduce_f32_block(orc, every, world * R)[0])


def _run_all(comm, inccl, torch, dev, world, rank, refs, extra):
    """every case of one rank on one communicator: [case][step] (result, residuals), then the extras"""
    comm.set_wire(inccl.WIRE_P16)
    comm.set_nonfinite(False)
    out = []
    for case, (steps, _) in zip(_cases(world), refs):
        n, average = case
        comm.set_average(average)
        rs = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(R)]
        got = []
        for bufs in steps:
            ts = [torch.from_numpy(x).to(dev) for x in bufs[rank]]
            torch.cuda.synchronize()
            y = comm.allreduce_f32_ef(ts, rs, stream=comm.stream)
            torch.cuda.synchronize()
            got.append((y.cpu().numpy(), [e.cpu().numpy() for e in rs]))
        out.append(got)
    comm.set_average(False)
    ts = [torch.from_numpy(x).to(dev) for x in extra[0][rank]]
    torch.cuda.synchronize()
    ext = [comm.allreduce_f32(ts, scale_exp=inccl.SCALE_BLOCK, stream=comm.stream)]
    comm.set_wire(inccl.WIRE_Q32)
    ext.append(comm.allreduce_f32(ts, scale_exp=inccl.SCALE_BLOCK, stream=comm.stream))
    torch.cuda.synchronize()
    return out, [o.cpu().numpy() for o in ext]


def _judge(world, rank, refs, extra, res, ext):
    bad = []
    for case, (_, want), got in zip(_cases(world), refs, res):
        for t, ((y, wres), (gy, gres)) in enumerate(zip(want, got)):
            try:
                _same(gy, y)
                for g, w in zip(gres, wres[rank]):
                    _same(g, w)
            except AssertionError as e:
                bad.append(f"world {world} rank {rank} case {case} step {t}: {str(e)[:300]}")
    for name, want, got in zip(("p16-block", "q32-block"), extra[1:], ext):
        try:
            _same(got, want)
        except AssertionError as e:
            bad.append(f"world {world} rank {rank} plain call {name}: {str(e)[:300]}")
    return bad


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_error_feedback_local(gpu, orc, world):
    """the in-process transport; world 1 is the fused kernel, the others absmax_ef
    -> max over the ranks -> pack_ef -> the int32 allreduce -> unpack"""
    import torch
    from container_inc_amd import inccl
    refs = [_reference(orc, world, c, 3100 + 100 * world + 10 * i) for i, c in enumerate(_cases(world))]
    extra = _extras_reference(orc, world, 3190 + world)

    def rank(r):
        grp = inccl.inccl_group_create_local(world, r, f"pack16-ef-{world}")
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
def test_error_feedback_rccl_world1(gpu, orc, monkeypatch, engine):
    """RCCL at world 1 with the sharded paths forced: both engines take the AR
    route on this wire (ncclAllReduce is a real call), so the residuals go
    through resolve_block_scale and the quantise stage, not the fused kernel"""
    import torch
    from container_inc_amd import inccl
    monkeypatch.setenv("INCCL_FORCE_RCCL", "1")
    monkeypatch.setenv("INCCL_FORCE_SHARDED", "1")
    monkeypatch.setenv("INCCL_MASTER_PORT", "0")
    monkeypatch.setenv("INCCL_RCCL_AR_BYTES", "0")
    refs = [_reference(orc, 1, c, 3700 + 10 * i) for i, c in enumerate(_cases(1))]
    extra = _extras_reference(orc, 1, 3790)
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


def test_refusals_leave_dst_and_residuals(gpu):
    """wire Q32, a NULL residual, a residual overlapping a source (the source
    itself, and one that starts inside it) or dst: INCCL_ERR_ARG by name, and
    dst and the residuals are as they were"""
    import torch
    from container_inc_amd import inccl
    from container_inc_amd._lib import IncclError
    n = 2341
    grp = inccl.inccl_group_create_local(1, 0, "pack16-ef-refuse")
    comm = inccl.inccl_communicator_create(grp, 0)
    try:
        big = torch.full((2 * n,), 3.0, dtype=torch.float32, device=gpu)
        ts = [big[:n], torch.full((n,), 2.0, dtype=torch.float32, device=gpu)]
        rs = [torch.full((n,), 0.5, dtype=torch.float32, device=gpu) for _ in ts]
        out = torch.full((n,), 7.0, dtype=torch.float32, device=gpu)

        def untouched():
            torch.cuda.synchronize()
            assert (out == 7.0).all() and all((e == 0.5).all() for e in rs) and (big == 3.0).all()

        assert comm.wire == inccl.WIRE_Q32
        with pytest.raises(IncclError, match=r"rc=-1.*INCCL_WIRE_P16"):
            comm.allreduce_f32_ef(ts, rs, out=out, stream=comm.stream)
        untouched()
        comm.set_wire(inccl.WIRE_P16)
        with pytest.raises(IncclError, match=r"rc=-1.*residuals\[1\] is NULL"):
            comm.allreduce_f32_ef(ts, [rs[0], None], out=out, stream=comm.stream)
        untouched()
        for alias in (ts[1], big[n - 1:2 * n - 1]):
            with pytest.raises(IncclError, match=r"rc=-1.*residuals\[1\] overlaps srcs"):
                comm.allreduce_f32_ef(ts, [rs[0], alias], out=out, stream=comm.stream)
            untouched()
        with pytest.raises(IncclError, match=r"rc=-1.*residuals\[0\] overlaps dst"):
            comm.allreduce_f32_ef(ts, [out, rs[1]], out=out, stream=comm.stream)
        untouched()
        assert (ts[1] == 2.0).all()
        # and the call goes through once nothing is wrong: dst may alias srcs[0]
        comm.allreduce_f32_ef(ts, rs, out=ts[0], stream=comm.stream)
        torch.cuda.synchronize()
        assert not (rs[0] == 0.5).all()
    finally:
        comm.destroy()
        grp.destroy()


# ---- one process per rank on one GPU: the IPC engines' int32 allreduce carries the words ----
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
        refs = [_reference(O, world, c, 3900 + 10 * i) for i, c in enumerate(_cases(world))]
        extra = _extras_reference(O, world, 3990 + world)
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


@pytest.mark.parametrize("world,engine", [(2, "p2p"), (2, "mesh")])
def test_error_feedback_multiprocess(gpu, world, engine):
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
