"""One rank of the error-feedback DDP test (tests/test_gpu_block16_ef_ddp.py):
the model, the gradients and the teardown order of tests/_block_ddp_rank.py --
three parameters of 2341 elements in all, no optimizer step, so every backward
pass produces the same gradients -- hooked with ``ddp.register(model, comm,
scale_exp=SCALE_BLOCK, wire_bits=16, error_feedback=True)`` on the real library
(p2p engine, every rank on cuda:0).

DDP rebuilds its buckets after the first iteration, in the order the gradients
became ready, and the hook then starts that bucket from a zero residual.  So
the rank runs one pass first, checks it, calls ``reset_residuals()`` and then
runs the T passes that are judged, all on the rebuilt bucket.  It reports:

* ``bit_exact``: every hooked bucket and its residual equal
  block16_ef_ref.step of all ranks' buckets and residuals at out_shift = log2 W;
* ``grads_are_buckets``: every pass's ``.grad``s are the reduced bucket's slices;
* ``within`` / ``worst``: |sum_t grad_t - T * exact mean| is within the
  telescoping bound / W (block16_ef_ref.telescoping_bound) on every lane, and
  the worst lane's share of it;
* ``plain_miss``: the share of lanes on which the same T passes with
  ``error_feedback=False`` exceed that bound.
"""
import itertools
import os
import sys

import numpy as np

from _block_ddp_rank import ROOT, SIZES, gradients


def _train(comm, rank, world, dev, T, orc, feedback):
    """One DDP model, one warm-up pass and T judged ones; everything torch made
    here dies with this frame, before the caller destroys the communicator
    (_block_ddp_rank._train).  Returns (report, [T] grads in bucket order,
    the ranks' buckets, the ranks' last residuals)."""
    import torch
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP

    import block16_ef_ref as ef
    from container_inc_amd import ddp, inccl

    class Dictated(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(s)) for s in SIZES])

        def forward(self, gs):
            return sum((p * g).sum() for p, g in zip(self.ps, gs))

    seen = []

    class Spy:
        """the communicator, recording every bucket and residual before and after its allreduce"""

        def __getattr__(self, name):
            return getattr(comm, name)

        def allreduce_f32_ef(self, srcs, residuals, out=None, **kw):
            before, res_before = srcs[0].detach().clone(), residuals[0].detach().clone()
            ret = comm.allreduce_f32_ef(srcs, residuals, out=out, **kw)
            seen.append((before, res_before, out, residuals[0]))
            return ret

        def allreduce_f32(self, srcs, out=None, **kw):
            before = srcs[0].detach().clone()
            ret = comm.allreduce_f32(srcs, out=out, **kw)
            seen.append((before, None, out, None))
            return ret

    def gather(t):
        allb = [None] * world
        dist.all_gather_object(allb, t.detach().cpu().numpy().tobytes())
        return [np.frombuffer(b, np.float32) for b in allb]

    shift = world.bit_length() - 1
    mine = gradients(world)[rank]
    report = {"buckets": [], "bit_exact": True, "grads_are_buckets": True}
    gs = [torch.from_numpy(g.copy()).to(dev) for g in mine]
    net = DDP(Dictated().to(dev), device_ids=[0])
    state = ddp.register(net, Spy(), scale_exp=inccl.SCALE_BLOCK, wire_bits=16, error_feedback=feedback)
    sums, every, last = None, None, None
    for it in range(T + 1):
        if it == 1:
            state.reset_residuals()        # the judged passes start from zero, on the rebuilt bucket
        seen.clear()
        net.zero_grad()
        net(gs).backward()
        torch.cuda.synchronize()
        report["buckets"].append(len(seen))
        before, res_before, after, res_after = seen[0]
        got = after.detach().cpu().numpy()
        every = gather(before)
        if feedback:
            y, new, _ = ef.step(orc, every, gather(res_before), world, out_shift=shift)
            last = gather(res_after)
            ok = np.array_equal(got.view(np.uint32), y.view(np.uint32)) and all(
                np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(last, new))
            report["bit_exact"] = report["bit_exact"] and bool(ok)
        # the order DDP packed the parameters in: the permutation whose pieces are this rank's bucket
        mine_flat = every[rank]
        order = next(o for o in itertools.permutations(range(len(SIZES)))
                     if np.array_equal(np.concatenate([mine[i] for i in o]), mine_flat))
        grads = np.concatenate([net.module.ps[i].grad.detach().cpu().numpy() for i in order])
        report["grads_are_buckets"] = report["grads_are_buckets"] and bool(np.array_equal(grads, got))
        if it >= 1:
            sums = grads.astype(np.float64) if sums is None else sums + grads.astype(np.float64)
    report["calls"] = state.calls
    report["residuals"] = len(state._residuals)
    seen.clear()
    return report, sums, every, last


def run(rank, world, port, boot_port, q, engine="p2p", T=8):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ["INCCL_BOOT_TIMEOUT"] = "120"
        os.environ["INCCL_ENGINE"] = engine
        import datetime
        import gc

        import torch
        import torch.distributed as dist

        import block16_ef_ref as ef
        from container_inc_amd import inccl
        from oracle import oracle as O

        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                timeout=datetime.timedelta(seconds=120))
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        grp = inccl.inccl_group_create(world, rank, "127.0.0.1", port=boot_port, device=0)
        assert grp is not None, "group create failed"
        comm = inccl.inccl_communicator_create(grp, 0)
        assert comm is not None and comm.engine == engine, comm and comm.engine
        try:
            report, sums, every, last = _train(comm, rank, world, dev, T, O, True)
            gc.collect()
            plain, plain_sums, plain_every, _ = _train(comm, rank, world, dev, T, O, False)
            assert all(np.array_equal(a, b) for a, b in zip(every, plain_every)), "the two runs packed different buckets"
            exact, bound = ef.telescoping_bound([every] * T, last, world)
            exact, bound = exact / world, bound / world
            err = np.abs(sums - exact)
            report["within"] = bool((err <= bound).all())
            report["worst"] = float(np.max(err[bound > 0] / bound[bound > 0]))
            report["plain_miss"] = float(np.mean(np.abs(plain_sums - exact) > bound))
            report["plain_buckets"], report["plain_calls"] = plain["buckets"], plain["calls"]
            report["wire"] = comm.wire
        finally:
            # torch lets go of the communicator's stream first (_train): the model and
            # the buckets are collected, their blocks' events recorded and waited for
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            comm.destroy()
            grp.destroy()
            dist.destroy_process_group()
        q.put((rank, report))
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put((rank, {"error": repr(e), "tb": traceback.format_exc()}))
