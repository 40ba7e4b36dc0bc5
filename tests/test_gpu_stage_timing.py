"""Per-stage timing (gpu): inccl_comm_set_stage_timing / inccl_comm_stage_times
on the sharded allreduce (quant + local sum -> int32 reduce-scatter -> dequantise
the own shard -> all-gather: api.c allreduce_piece, one function for every
format, run per chunk by the pipelined form) and the reduce-scatter.  The stages
must be recorded with plausible times, for fp32 and 2-byte buckets alike, the
pipelined call must report its chunks' stages, and timing must not change a
result (bit-exact vs the oracle with timing on)."""
import numpy as np
import pytest

from test_gpu_comm import _run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt,chunks", [pytest.param("f32", 1, id="1"), pytest.param("f32", 4, id="4"),
                                        pytest.param("bf16", 1, id="bf16")])
def test_stage_times_allreduce_local(gpu, orc, fmt, chunks):
    """bf16: a small ragged bucket (the copy-out stage exists) through the piece
    the fp32 path runs, so its stages are recorded too."""
    import torch
    from container_inc_amd import inccl
    world = 2
    n, k = ((1 << 22) + 192, 25) if fmt == "f32" else ((1 << 16) + 192, 22)
    rng = np.random.default_rng(chunks if fmt == "f32" else 16)
    hs = [[rng.standard_normal(n).astype(np.float32) for _ in range(2)] for _ in range(world)]
    if fmt == "bf16":
        hs = [[orc.f32_to_bf16(h) for h in per] for per in hs]
        want = orc.reduce_bf16([h for per in hs for h in per], k).view(np.int16)
    else:
        want = orc.reduce_f32([h for per in hs for h in per], k).view(np.uint32)

    def rank(r):
        grp = inccl.inccl_group_create_local(world, r, f"stage-{fmt}-{chunks}")
        comm = inccl.inccl_communicator_create(grp, 0)
        if fmt == "bf16":
            xs = [torch.from_numpy(h.view(np.int16)).to(gpu).view(torch.bfloat16) for h in hs[r]]
            allreduce = comm.allreduce_bf16
            bits = lambda t: t.view(torch.int16).cpu().numpy()   # noqa: E731
        else:
            xs = [torch.from_numpy(h).to(gpu) for h in hs[r]]
            allreduce = lambda *a, **kw: comm.allreduce_f32(*a, chunks=chunks, **kw)   # noqa: E731
            bits = lambda t: t.cpu().numpy().view(np.uint32)   # noqa: E731
        allreduce(xs, scale_exp=k, stream=comm.stream)   # workspaces, untimed
        torch.cuda.synchronize()
        assert comm.stage_times()["stages"] == 0   # timing is off by default
        comm.set_stage_timing(True)
        out = allreduce(xs, scale_exp=k, stream=comm.stream)
        torch.cuda.synchronize()
        st = comm.stage_times()
        rs = comm.reduce_scatter(xs, scale_exp=k, stream=comm.stream)
        torch.cuda.synchronize()
        st_rs = comm.stage_times()
        comm.set_stage_timing(False)
        res = bits(out), bits(rs), st, st_rs
        comm.barrier()
        comm.destroy()
        grp.destroy()
        return res

    shard = n // world
    for r, (got, got_rs, st, st_rs) in enumerate(_run_ranks(world, rank)):
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_rs, want[r * shard:(r + 1) * shard])
        for name in ("quant", "reduce_scatter", "dequant", "all_gather"):
            assert st.get(name, 0.0) > 0.0, (name, st)
        # 4 stages per chunk (+ the copy-out of a ragged bucket), + the pipelined form's anchor
        assert st["stages"] >= 4 * chunks + (1 if chunks > 1 else 0), st
        assert st["wall_us"] > 0.0
        assert sum(v for key, v in st.items() if key in inccl.Communicator.STAGE_NAMES) >= 0.5 * st["wall_us"]
        for name in ("quant", "reduce_scatter", "dequant"):
            assert st_rs.get(name, 0.0) > 0.0, (name, st_rs)


@pytest.mark.parametrize("chunks", [1, 4])
def test_stage_times_rccl_world1(gpu, orc, monkeypatch, chunks):
    """The rccl engine's own stages around real RCCL collectives (world 1, the
    sharded route forced: ncclReduceScatter and ncclAllGather are launched)."""
    import torch
    from container_inc_amd import inccl
    monkeypatch.setenv("INCCL_FORCE_RCCL", "1")
    monkeypatch.setenv("INCCL_FORCE_SHARDED", "1")
    monkeypatch.setenv("INCCL_MASTER_PORT", "0")
    grp = inccl.inccl_group_create(1, 0, "127.0.0.1")
    comm = inccl.inccl_communicator_create(grp, 0)
    comm.set_engine("rccl")
    n, k = 1 << 22, 25
    rng = np.random.default_rng(5 + chunks)
    hs = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    xs = [torch.from_numpy(h).to(gpu) for h in hs]
    comm.allreduce_f32(xs, scale_exp=k, chunks=chunks, stream=comm.stream)
    torch.cuda.synchronize()
    comm.set_stage_timing(True)
    out = comm.allreduce_f32(xs, scale_exp=k, chunks=chunks, stream=comm.stream)
    torch.cuda.synchronize()
    st = comm.stage_times()
    comm.set_stage_timing(False)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), orc.reduce_f32(hs, k).view(np.uint32))
    for name in ("quant", "reduce_scatter", "dequant", "all_gather"):
        assert st.get(name, 0.0) > 0.0, (name, st)
    assert st["stages"] >= 4 * chunks, st
    comm.destroy()
    grp.destroy()
