"""One rank of the per-block scaling DDP test (tests/test_gpu_block_ddp.py), and
the gradients it uses (tests/test_block_hooks.py checks them on the CPU).

The model is three parameter vectors whose gradients are dictated: rank r's
loss is sum_p <p, g_r[p]>, so its gradient is g_r exactly, and g_r is rank r's
bucket of ``block_ref.mixed_buckets(default_rng(0), 2341, W, zero_block=4)`` --
the data of tests/test_block_ref.py: 256-element runs whose magnitudes span
10^[-12, 6), cut into the parameters.  DDP packs the three into one flat
bucket, in an order of its choosing, and
``container_inc_amd.ddp.allreduce_hook`` reduces it with
``scale_exp=SCALE_BLOCK`` on the real library (p2p engine, every rank on
cuda:0).  Each rank reports, over every hooked bucket:

* ``bit_exact``: the bucket equals block_ref.reduce_f32_block of all ranks'
  buckets, divided by W (exact: W is a power of two);
* ``block_err``: max |bucket - float64 mean| over block_ref.error_bound / W;
* ``auto_miss``: the smallest share of lanes on which the same buckets under
  SCALE_AUTO's one exponent (the oracle's reduce_f32 / W) exceed that bound.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (768, 1061, 512)   # the parameters: 2341 = 256 * 9 + 37 elements in all
N = sum(SIZES)


def gradients(world):
    """[rank][param] fp32 arrays"""
    import block_ref
    bufs = block_ref.mixed_buckets(np.random.default_rng(0), N, world, zero_block=4)
    cuts = np.cumsum((0,) + SIZES)
    return [[b[cuts[i]:cuts[i + 1]] for i in range(len(SIZES))] for b in bufs]


def judge(orc, every, got, world):
    """(bit_exact, block_err, auto_miss) of one bucket: `every` the ranks' inputs,
    `got` the averaged result (None: the reference's own)"""
    import block_ref
    shift = world.bit_length() - 1
    want, ks = block_ref.reduce_f32_block(orc, every, world, out_shift=shift)
    exact, bound = block_ref.error_bound(every, ks, world)
    exact, bound = exact / world, bound / world
    y = want if got is None else got
    bit_exact = bool(np.array_equal(y.view(np.uint32), want.view(np.uint32)))
    block_err = float(np.max(np.abs(y.astype(np.float64) - exact) / bound))
    auto = orc.reduce_f32(every, orc.choose_scale(orc.absmax(every), world)) / np.float32(world)
    auto_miss = float(np.mean(np.abs(auto.astype(np.float64) - exact) > bound))
    return bit_exact, block_err, auto_miss


def _train(comm, rank, world, dev, iters, orc):
    """The DDP iterations on `comm`.  Everything torch made here -- the DDP
    model, its buckets, the recorded buckets -- dies with this frame, before the
    caller destroys the communicator: the hook runs each bucket on the
    communicator's own stream and marks it as used there
    (ddp.allreduce_hook: ExternalStream, record_stream), and the caching
    allocator records an event on that stream when such a block is freed."""
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

    report = {"buckets": [], "bit_exact": True, "block_err": 0.0, "auto_miss": 1.0}
    gs = [torch.from_numpy(g.copy()).to(dev) for g in gradients(world)[rank]]
    net = DDP(Dictated().to(dev), device_ids=[0])
    state = ddp.register(net, Spy(), scale_exp=inccl.SCALE_BLOCK)
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
            ok, err, miss = judge(orc, every, after.detach().cpu().numpy(), world)
            report["bit_exact"] = report["bit_exact"] and ok
            report["block_err"] = max(report["block_err"], err)
            report["auto_miss"] = min(report["auto_miss"], miss)
    report["calls"] = state.calls
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
