"""DDP comm hook with per-block scaling on the GPU (gpu):
``ddp.register(model, comm, scale_exp=inccl.SCALE_BLOCK)`` at W = 2 on the p2p
engine, every rank on cuda:0, on a model whose parameters' gradients span
eighteen decades inside one flat bucket (tests/_block_ddp_rank.py).  Every
hooked bucket must equal block_ref's result divided by W bit for bit and sit
within block_ref.error_bound of the float64 mean on every lane, where
SCALE_AUTO's one exponent misses that bound on more than half of the lanes (the
reference alone, on the CPU: tests/test_block_hooks.py)."""
import multiprocessing as mp

import pytest

from test_ddp_hook import _free_ports

pytestmark = pytest.mark.gpu


def test_ddp_hook_block_scale_gpu(gpu, orc):
    import _block_ddp_rank
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port, boot_port = _free_ports(2)
    ps = [ctx.Process(target=_block_ddp_rank.run, args=(r, world, port, boot_port, q)) for r in range(world)]
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
        assert rep["bit_exact"], rep
        assert rep["block_err"] <= 1.0, rep
        assert rep["auto_miss"] > 0.5, rep
    assert [p.exitcode for p in ps] == [0] * world, [p.exitcode for p in ps]
