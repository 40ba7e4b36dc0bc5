"""Per-block scaling in the DDP / FSDP hooks, the parts that need no GPU: a
16-bit bucket is refused by name, and the gradients of the GPU DDP test
(tests/_block_ddp_rank.py) show the gap on the reference alone -- whatever order
DDP packs the three parameters in, SCALE_AUTO's one exponent misses the
per-block bound on more than half of the lanes and per-block exponents meet it
on every lane -- so the GPU test's condition is known before it runs."""
import itertools

import numpy as np
import pytest

import _block_ddp_rank


def test_hooks_refuse_a_16_bit_bucket_in_block_mode():
    import torch
    from container_inc_amd import ddp, inccl
    from container_inc_amd._lib import IncclError
    state = ddp.HookState(comm=None, scale_exp=inccl.SCALE_BLOCK)
    state.check_format(torch.float32)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(IncclError, match="SCALE_BLOCK.*fp32"):
            state.check_format(dt)
    ddp.HookState(comm=None).check_format(torch.bfloat16)   # SCALE_AUTO: every format


def test_fsdp_hook_refuses_a_16_bit_gradient_in_block_mode():
    import torch
    from container_inc_amd import ddp, fsdp, inccl
    from container_inc_amd._lib import IncclError
    state = ddp.HookState(comm=None, scale_exp=inccl.SCALE_BLOCK)
    g = torch.ones(8, dtype=torch.bfloat16)
    with pytest.raises(IncclError, match="SCALE_BLOCK"):
        fsdp.reduce_scatter_hook(state, g, torch.empty(4, dtype=torch.bfloat16))
    with pytest.raises(IncclError, match="SCALE_BLOCK"):
        fsdp.allreduce_hook(state, g)


@pytest.mark.parametrize("world", [2])
def test_ddp_gradients_show_the_gap_in_any_bucket_order(orc, world):
    grads = _block_ddp_rank.gradients(world)
    assert sum(g.size for g in grads[0]) == _block_ddp_rank.N == 2341
    for order in itertools.permutations(range(len(_block_ddp_rank.SIZES))):
        every = [np.concatenate([per[i] for i in order]) for per in grads]
        ok, block_err, auto_miss = _block_ddp_rank.judge(orc, every, None, world)
        print(f"order {order}: block scale at {block_err:.3f} of the bound, auto scale misses it on {auto_miss:.3f}")
        assert ok and block_err <= 1.0 and auto_miss > 0.5, (order, block_err, auto_miss)
