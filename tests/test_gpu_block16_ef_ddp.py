"""DDP comm hook with error feedback: ``ddp.register(model, comm,
scale_exp=inccl.SCALE_BLOCK, wire_bits=16, error_feedback=True)``.

gpu: W = 2 on the p2p engine, every rank on cuda:0, on the model of
tests/test_gpu_block_ddp.py with no optimizer step, so the gradients repeat
(tests/_ef_ddp_rank.py).  Over T = 8 backward passes every hooked bucket and
its residual equal the reference's step bit for bit, and the sum of the T
``.grad``s is within the telescoping bound / W of T exact mean gradients on
every lane; the same passes with ``error_feedback=False`` exceed that bound on
at least half of the lanes (tests/test_block16_ef_ref.py shows both on the
reference alone).

cpu: the option's plumbing -- what it refuses, and how the hook state keys its
residuals."""
import multiprocessing as mp

import pytest

from test_ddp_hook import _free_ports


@pytest.mark.gpu
def test_ddp_hook_error_feedback_gpu(gpu, orc):
    import _ef_ddp_rank
    from container_inc_amd import inccl
    world, T = 2, 8
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port, boot_port = _free_ports(2)
    ps = [ctx.Process(target=_ef_ddp_rank.run, args=(r, world, port, boot_port, q, "p2p", T)) for r in range(world)]
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
        assert rep["buckets"] == [1] * (T + 1) and rep["calls"] == T + 1, rep
        assert rep["plain_buckets"] == [1] * (T + 1) and rep["plain_calls"] == T + 1, rep
        assert rep["residuals"] == 1 and rep["wire"] == inccl.WIRE_P16, rep
        assert rep["bit_exact"] and rep["grads_are_buckets"], rep
        assert rep["within"] and rep["worst"] <= 1.0, rep
        assert rep["plain_miss"] >= 0.5, rep
    assert [p.exitcode for p in ps] == [0] * world, [p.exitcode for p in ps]


class _Bucket:
    """what the hook asks of a GradBucket"""

    def __init__(self, buf, index=0, params=(), last=True):
        self._buf, self._index, self._params, self._last = buf, index, list(params), last

    def buffer(self):
        return self._buf

    def index(self):
        return self._index

    def parameters(self):
        return self._params

    def is_last(self):
        return self._last


def test_error_feedback_is_refused_by_name():
    """wire_bits=32, SCALE_AUTO and a fixed exponent: refused naming both
    settings; a bf16 bucket: refused; fsdp.register(error_feedback=True): refused"""
    import torch
    from container_inc_amd import ddp, fsdp, inccl
    from container_inc_amd._lib import IncclError

    class Model:
        def register_comm_hook(self, state, hook):
            raise AssertionError("the hook must not be registered")

    for kw in (dict(scale_exp=inccl.SCALE_BLOCK, wire_bits=32), dict(scale_exp=inccl.SCALE_AUTO, wire_bits=16),
               dict(scale_exp=25, wire_bits=16), dict()):
        with pytest.raises(IncclError, match=r"error_feedback.*scale_exp=SCALE_BLOCK.*wire_bits=16"):
            ddp.register(Model(), None, error_feedback=True, **kw)
    state = ddp.HookState(comm=None, scale_exp=inccl.SCALE_BLOCK, wire_bits=16, error_feedback=True)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(IncclError, match="fp32"):
            ddp.allreduce_hook(state, _Bucket(torch.ones(8, dtype=dt)))
    assert state.calls == 0 and not state._residuals
    with pytest.raises(IncclError, match=r"FSDP.*error_feedback"):
        fsdp.register(Model(), None, error_feedback=True)
    with pytest.raises(IncclError, match=r"FSDP.*error_feedback"):
        fsdp.register(Model(), None, sharded=False, error_feedback=True, scale_exp=inccl.SCALE_BLOCK, wire_bits=16)
    assert ddp.HookState(comm=None).error_feedback is False          # off by default


def test_residuals_follow_the_buckets():
    """one zero residual per (bucket index, numel); a bucket whose size or
    parameter layout changed starts from zero and the stale residual is dropped,
    as are those past the last bucket; reset_residuals() forgets them all"""
    import torch
    from container_inc_amd import ddp, inccl
    state = ddp.HookState(comm=None, scale_exp=inccl.SCALE_BLOCK, wire_bits=16, error_feedback=True)
    a, b, c = (torch.zeros(s) for s in (16, 32, 8))
    b0, b1 = torch.zeros(48), torch.zeros(8)
    r0 = state.residual(_Bucket(b0, 0, [a, b], last=False), b0)
    r1 = state.residual(_Bucket(b1, 1, [c]), b1)
    assert r0.dtype == torch.float32 and r0.numel() == 48 and not r0.any() and r1.numel() == 8
    r0.add_(1.0)
    assert state.residual(_Bucket(b0, 0, [a, b], last=False), b0) is r0            # the same bucket: carried
    fresh = state.residual(_Bucket(b0, 0, [b, a], last=False), b0)                 # rebuilt in another order
    assert fresh is not r0 and not fresh.any() and len(state._residuals) == 2
    big = torch.zeros(56)
    only = state.residual(_Bucket(big, 0, [b, a, c]), big)                         # rebuilt into one bucket
    assert only.numel() == 56 and set(state._residuals) == {(0, 56)}
    state.reset_residuals()
    assert not state._residuals
    assert not state.residual(_Bucket(big, 0, [b, a, c]), big).any()
