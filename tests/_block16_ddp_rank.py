"""One rank of the packed-wire DDP test (tests/test_gpu_block16_ddp.py): the
model, the gradients and the teardown order of tests/_block_ddp_rank.py, hooked
with ``ddp.register(model, comm, scale_exp=SCALE_BLOCK, wire_bits=16)`` on the
real library (p2p engine, every rank on cuda:0).  Each rank reports, over every
hooked bucket:

* ``bit_exact``: the bucket equals block16_ref.reduce_f32_block16 of all ranks'
  buckets, divided by W (exact: W is a power of two);
* ``lane_err``: max |bucket - float64 mean| over the lanes' bound
  (W * 2^-(k_b + 1) + |sum| * 2^-23) / W;
* ``wire``: the communicator's wire after the hook ran (INCCL_WIRE_P16).
"""
import os
import sys

import numpy as np

from _block_ddp_rank import ROOT, SIZES, gradients


def judge(orc, every, got, world):
    """(bit_exact, lane_err) of one bucket: `every` the ranks' inputs, `got` the averaged result"""
    import block16_ref
    import block_ref
    shift = world.bit_length() - 1
    want, ks = block16_ref.reduce_f32_block16(orc, every, world, out_shift=shift)
    exact, bound = block_ref.error_bound(every, ks, world)
    bit_exact = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    return bit_exact, float(np.max(np.abs(got.astype(np.float64) - exact / world) / (bound / world)))


def _train(comm, rank, world, dev, iters, orc):
    """The DDP iterations on `comm`; everything torch made here dies with this
    frame, before the caller destroys the communicator (_block_ddp_rank._train)."""
    import torch
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP

    from container_inc_amd import ddp, inccl

    class Dictated(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(s)) for s in SIZES])

        def forward(self, gs):
            return sum((p * g).sum() for p, g in zip(self.ps, gs))

    seen = []

    class Spy:
        """the communicator, recording every bucket before and after its allreduce"""

        def __getattr__(self, name):
            return getattr(comm, name)

        def allreduce_f32(self, srcs, out=None, **kw):
            before = srcs[0].detach().clone()
            res = comm.allreduce_f32(srcs, out=out, **kw)
            seen.append((before, out))
            return res

    report = {"buckets": [], "bit_exact": True, "lane_err": 0.0}
    gs = [torch.from_numpy(g.copy()).to(dev) for g in gradients(world)[rank]]
    net = DDP(Dictated().to(dev), device_ids=[0])
    state = ddp.register(net, Spy(), scale_exp=inccl.SCALE_BLOCK, wire_bits=16)
    for it in range(iters):
        seen.clear()
        net.zero_grad()
        net(gs).backward()
        torch.cuda.synchronize()
        report["buckets"].append(len(seen))
        for before, after in seen:
            allb = [None] * world
            dist.all_gather_object(allb, before.cpu().numpy().tobytes())
            every = [np.frombuffer(b, np.float32) for b in allb]
            ok, err = judge(orc, every, after.detach().cpu().numpy(), world)
            report["bit_exact"] = report["bit_exact"] and ok
            report["lane_err"] = max(report["lane_err"], err)
    report["calls"] = state.calls
    report["wire"] = comm.wire
    seen.clear()
    return report


def run(rank, world, port, boot_port, q, engine="p2p", iters=2):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ["INCCL_BOOT_TIMEOUT"] = "120"
        os.environ["INCCL_ENGINE"] = engine
        import datetime
        import gc

        import torch
        import torch.distributed as dist

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
            report = _train(comm, rank, world, dev, iters, O)
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
