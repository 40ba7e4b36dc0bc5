"""DDP comm hook on the packed 16-bit wire (gpu): ``ddp.register(model, comm,
scale_exp=inccl.SCALE_BLOCK, wire_bits=16)`` at W = 2 on the p2p engine, every
rank on cuda:0, on the model of tests/test_gpu_block_ddp.py (gradients spanning
eighteen decades inside one flat bucket; tests/_block16_ddp_rank.py).  Every
hooked bucket must equal block16_ref's result divided by W bit for bit and sit
within the lanes' bound of the float64 mean on every lane; the hook leaves the
communicator on INCCL_WIRE_P16."""
import multiprocessing as mp

import pytest

from test_ddp_hook import _free_ports

pytestmark = pytest.mark.gpu


def test_ddp_hook_packed_wire_gpu(gpu, orc):
    import _block16_ddp_rank
    from container_inc_amd import inccl
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port, boot_port = _free_ports(2)
    ps = [ctx.Process(target=_block16_ddp_rank.run, args=(r, world, port, boot_port, q)) for r in range(world)]
    for p in ps:
        p.start()
    try:
        res = dict(q.get(timeout=240) for _ in range(world))
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
                p.join()
    for r in range(world):
        rep = res[r]
        assert "error" not in rep, rep.get("tb")
        print(f"rank {r}: {rep}")
        assert rep["buckets"] == [1, 1] and rep["calls"] == 2, rep
        assert rep["wire"] == inccl.WIRE_P16, rep
        assert rep["bit_exact"], rep
        assert rep["lane_err"] <= 1.0, rep
    assert [p.exitcode for p in ps] == [0] * world, [p.exitcode for p in ps]
