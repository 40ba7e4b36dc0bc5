"""Every communicator route writes only inside dst (gpu), in-process: the
in-process transport (ranks are threads, worlds 1, 3 and 8) and RCCL at world 1
with the sharded path forced (engines rccl, ar, a2a).  The matrix, the
references and the three checks of every case -- the result bit for bit, both
guards of dst, every source and every residual's guards as uploaded -- are
tests/comm_guard_cases.py's; the buffers are tests/guarded.py's.  World 1 of
the in-process transport is the FUSED route; the others take RSAG / RS / AR /
AR_SHARD of inccl_route.h, the "ar" engine AR for fp32.  Every communicator and
group is destroyed and every thread joined before a test returns."""
import numpy as np
import pytest

import comm_guard_cases as cg
from test_gpu_block16_comm import _run_ranks

pytestmark = pytest.mark.gpu


def _local(gpu, orc, world, hub, cs, engine=None, prepared=()):
    """the cases `cs`, then the prepared ops, on one communicator per rank thread"""
    from container_inc_amd import inccl
    preps = [cg.prepare(orc, world, c) for c in cs]
    pcs = [cg.prepared_case(world, kind) for kind in prepared]
    ppreps = [cg.prepare(orc, world, c) for c in pcs]

    def rank(r):
        grp = inccl.inccl_group_create_local(world, r, hub)
        comm = inccl.inccl_communicator_create(grp, 0)
        try:
            if engine:
                comm.set_engine(engine)
            res = cg.run_cases(comm, inccl, gpu, world, r, cs, preps, comm.stream)
            for c, p in zip(pcs, ppreps):
                res += cg.run_prepared(comm, inccl, gpu, world, r, c, p, comm.stream)
            comm.barrier()
        finally:
            comm.destroy()
            grp.destroy()
        return res

    bad = {r: cg.failures(res) for r, res in enumerate(_run_ranks(world, rank))}
    assert not any(bad.values()), bad


@pytest.mark.parametrize("part", cg.PARTS + ("chunks",))
@pytest.mark.parametrize("world", [1, 3, 8])
def test_local_routes(gpu, orc, world, part):
    """allreduce of the three kinds at a fixed exponent and at auto scale, fp32
    per block, on the packed wire and with error feedback over two steps,
    chunks = 3 of the RSAG route, in place, reduce-scatter at the four shards,
    and what the API refuses"""
    _local(gpu, orc, world, f"guards-{world}-{part}", cg.cases(world, part))


@pytest.mark.parametrize("world", [3, 8])
def test_local_ar_engine(gpu, orc, world):
    """engine "ar" on the in-process transport: AR for fp32 (block, packed and
    error feedback included), RSAG for bf16"""
    cs = [c for part in ("f32", "bf16", "block", "p16", "ef") for c in cg.cases(world, part)]
    _local(gpu, orc, world, f"guards-ar-{world}", cs, engine="ar")


def test_local_average_world8(gpu, orc):
    """inccl_comm_set_average once per mode: the mean of every kind, per block,
    packed, with error feedback, and of three reduce-scatters"""
    _local(gpu, orc, 8, "guards-avg-8", cg.cases(8, "average"))


@pytest.mark.parametrize("world", [3])
def test_local_prepared(gpu, orc, world):
    """prepare_allreduce_f32 and prepare_allreduce_bf16, each run twice"""
    _local(gpu, orc, world, f"guards-prepared-{world}", [], prepared=("f32", "bf16"))


@pytest.fixture()
def force_rccl(monkeypatch):
    monkeypatch.setenv("INCCL_FORCE_RCCL", "1")
    monkeypatch.setenv("INCCL_FORCE_SHARDED", "1")
    monkeypatch.setenv("INCCL_MASTER_PORT", "0")


def _rccl_world1(gpu, orc, engine, cs, prepared=()):
    from container_inc_amd import inccl
    grp = inccl.inccl_group_create(1, 0, "127.0.0.1")
    assert grp is not None and grp.transport == "rccl"
    comm = inccl.inccl_communicator_create(grp, 0)
    try:
        comm.set_engine(engine)
        assert comm.engine == engine
        res = cg.run_cases(comm, inccl, gpu, 1, 0, cs, [cg.prepare(orc, 1, c) for c in cs], comm.stream)
        for kind in prepared:
            c = cg.prepared_case(1, kind)
            res += cg.run_prepared(comm, inccl, gpu, 1, 0, c, cg.prepare(orc, 1, c), comm.stream)
    finally:
        comm.destroy()
        grp.destroy()
    bad = cg.failures(res)
    assert not bad, bad


@pytest.mark.parametrize("engine", ["rccl", "ar", "a2a"])
def test_rccl_world1_routes(gpu, orc, force_rccl, monkeypatch, engine):
    """every part of the matrix on one communicator (an RCCL communicator costs
    half a second to make): ncclReduceScatter / ncclAllGather / ncclAllReduce
    and the grouped send / recv are real RCCL calls on a one-rank communicator;
    the small-bucket AR route is off (INCCL_RCCL_AR_BYTES=0), so "rccl" takes
    RSAG and RS"""
    monkeypatch.setenv("INCCL_RCCL_AR_BYTES", "0")
    _rccl_world1(gpu, orc, engine, [c for part in cg.PARTS + ("chunks",) for c in cg.cases(1, part)])


def test_rccl_world1_small_bucket_route(gpu, orc, force_rccl, monkeypatch):
    """INCCL_RCCL_AR_BYTES = 512: buckets of up to 128 elements (1, 65, 67 and
    128) take one ncclAllReduce, the others (130, 1287) reduce-scatter + all-gather"""
    monkeypatch.setenv("INCCL_RCCL_AR_BYTES", "512")
    _rccl_world1(gpu, orc, "rccl", [c for part in ("f32", "bf16", "block", "p16") for c in cg.cases(1, part)])


def test_rccl_world1_prepared(gpu, orc, force_rccl, monkeypatch):
    """prepare_allreduce_f32 and prepare_allreduce_bf16 over RCCL, each run twice"""
    monkeypatch.setenv("INCCL_RCCL_AR_BYTES", "0")
    _rccl_world1(gpu, orc, "rccl", [], prepared=("f32", "bf16"))


def test_buf_guards_catch_a_store_outside(gpu):
    """the helper itself: a store one element before or past the payload fails bits()"""
    from guarded import Buf
    for kind in ("f32", "bf16"):
        for at in (-1, 5):
            b = Buf(gpu, kind, 5, np.zeros(5, np.float32 if kind == "f32" else np.uint16), shift=1)
            np.testing.assert_array_equal(b.bits(), 0)
            b.raw[b.lo + at] = 0
            with pytest.raises(AssertionError, match="written"):
                b.bits()
