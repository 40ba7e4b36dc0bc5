"""PyTorch DDP communication hook over the INCCL engine -- the caller of this path.

The reference's only caller is ``host.c:39-47``: it creates a group and a
communicator, then calls ``inccl_allreduce_write`` on one int32 buffer.  In a
training job the caller of a gradient-aggregation engine is the data-parallel
wrapper, which hands over one flat fp32 gradient bucket at a time.  This module
plugs the engine in there: ``DistributedDataParallel.register_comm_hook`` with
:func:`allreduce_hook` sends every bucket through ``inccl_allreduce_f32``
(quantise -> int32 sum across ranks -> dequantise; the int32 sum is the
reference switch's aggregate, ``non_termination_switch.c:361-363``) and returns
the bucket averaged over the ranks, as DDP's built-in allreduce hook does.

Numerics: the scale defaults to ``SCALE_AUTO`` -- the bucket's absmax over every
rank picks the largest exponent whose int32 sum cannot overflow
(``orc_choose_scale``), so a bucket of any magnitude keeps ~30 significant bits
of its largest element.  Non-finite gradients: the hook switches its
communicator to ``set_nonfinite(True)``, so a NaN or +-Inf in any rank's bucket
makes the whole averaged bucket NaN on every rank -- a mixed-precision loss
scaler (``torch.amp.GradScaler``) then sees the overflow and skips the step, as
it would after a float allreduce.  (The quantiser alone would map NaN to 0 and
saturate +-Inf: a finite, wrong gradient.)  The averaged result is bit-identical to the oracle's
``reduce_f32`` of the same buckets divided by the world size.

``scale_exp=inccl.SCALE_BLOCK`` (fp32 buckets only) gives every 256-element
block of the bucket its own auto exponent instead: a flat bucket concatenates
parameters whose gradients differ by orders of magnitude, and under
``SCALE_AUTO`` the largest one sets the exponent for all of them (a LayerNorm
gain next to an embedding row keeps few or no significant bits).  The mean and
the non-finite mode apply alike, the latter per block: only the blocks that
held a NaN or +-Inf come out NaN.  A bf16 / fp16 bucket in this mode raises.
``wire_bits=16`` with it exchanges packed 16-bit lanes (``Communicator.set_wire``,
``inccl_comm_set_wire``): half the exchanged bytes at 16 bits less precision per
block, for 2-16 contributors; 32 (the default) is one int32 per element.

``error_feedback=True`` (with ``scale_exp=SCALE_BLOCK`` and ``wire_bits=16``
only, fp32 buckets) keeps what the 16-bit lanes could not carry: the hook state
holds one fp32 residual per bucket, zero at first, which
``Communicator.allreduce_f32_ef`` adds to the bucket before it is quantised and
overwrites with the new remainder (``inccl_allreduce_f32_ef``).  Nothing is lost,
it arrives a step later: the sum of T averaged gradients stays within the last
residuals of T exact means instead of drifting by the same rounding error T
times.  A residual belongs to ``bucket.index()`` and its size and parameter
layout: DDP rebuilds its buckets after the first iteration, and a bucket that no
longer matches starts from a fresh zero residual.  The residuals live on the
communicator's stream, as the buckets' reductions do; ``reset_residuals()``
drops them (after a skipped step or a change of the learning-rate schedule,
where a carried remainder is unwanted).

fp32, bf16 and fp16 CUDA buckets are accepted (bf16 / fp16 through
``inccl_allreduce_bf16`` / ``_f16``: the same int32 sums, the result rounded to
the bucket's format).  For a power-of-two world the mean comes out of the
dequantise stage itself (``inccl_comm_set_average``: scale 2^-(k + log2 W)),
for every format alike; otherwise the hook divides by W in torch.  Anything
else raises (no silent fallback to another collective).

Teardown: the hook runs every bucket on the communicator's own stream and marks
it as used there (``record_stream``), and torch's caching allocator records an
event on that stream when such a bucket is freed.  So drop the DDP model (and
anything else that holds its buckets), ``torch.cuda.synchronize()`` and
``torch.cuda.empty_cache()`` before ``comm.destroy()``: a rank that destroyed
its communicator first, with the model still alive, crashed at exit
(tests/_block_ddp_rank.py keeps this order).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

from . import inccl
from ._lib import IncclError


@dataclass
class HookState:
    """What :func:`allreduce_hook` needs: the communicator, the scale and
    whether to average.  ``calls`` counts the buckets reduced (for tests and
    logging)."""

    comm: object
    scale_exp: int = inccl.SCALE_AUTO
    average: bool = True
    calls: int = 0
    folded: bool | None = None   # the mean comes out of the dequantise stage (inccl_comm_set_average)
    propagate_nonfinite: bool = True   # NaN / +-Inf anywhere -> the bucket is NaN (inccl_comm_set_nonfinite)
    _nonfinite_set: bool = False
    _wire_set: bool = False
    error_feedback: bool = False   # keep what the 16-bit lanes drop and add it to the next step (allreduce_f32_ef)
    _residuals: dict = field(default_factory=dict, repr=False)   # (bucket index, numel) -> (layout, fp32 residual)
    wire_bits: int = 32          # 16: SCALE_BLOCK buckets travel as packed 16-bit lanes (inccl_comm_set_wire)

    def __post_init__(self):
        if self.error_feedback and (self.scale_exp != inccl.SCALE_BLOCK or self.wire_bits != 16):
            raise IncclError("inccl hook: error_feedback=True corrects the packed 16-bit lanes: it needs "
                             "scale_exp=SCALE_BLOCK and wire_bits=16, got "
                             f"scale_exp={_scale_name(self.scale_exp)} and wire_bits={self.wire_bits!r}")

    def residual(self, bucket, buf):
        """The residual of this bucket, on the current stream's device memory:
        zeros for a bucket seen for the first time or whose size or parameter
        layout changed (DDP's rebuilt buckets); residuals of buckets past the
        last one are dropped."""
        import torch
        index = bucket.index() if hasattr(bucket, "index") else 0
        params = bucket.parameters() if hasattr(bucket, "parameters") else ()
        layout = tuple((p.data_ptr(), p.numel()) for p in params)
        key = (index, buf.numel())
        held = self._residuals.get(key)
        if held is None or held[0] != layout:
            for k in [k for k in self._residuals if k[0] == index]:
                del self._residuals[k]
            held = (layout, torch.zeros(buf.numel(), dtype=torch.float32, device=buf.device))
            self._residuals[key] = held
        if hasattr(bucket, "is_last") and bucket.is_last():
            for k in [k for k in self._residuals if k[0] > index]:
                del self._residuals[k]
        return held[1]

    def reset_residuals(self) -> None:
        """Forget every residual: the next step of each bucket starts from zero."""
        self._residuals.clear()

    def fold_average(self) -> bool:
        """Once: let the engine return the mean (power-of-two worlds: 2^-log2 W is
        folded into the dequantise scale, bit-identical to dividing, one pass
        fewer); otherwise the hook divides.  This switches the communicator
        itself to averaging: give the hook a communicator of its own."""
        if self.folded is None:
            self.folded = False
            if self.average and self.world_size > 1 and hasattr(self.comm, "set_average"):
                try:
                    self.comm.set_average(True)
                    self.folded = True
                except IncclError:
                    pass
        return self.folded

    def apply_nonfinite(self) -> None:
        """Once: the communicator's non-finite mode (auto scale and per-block scale only)."""
        if not self._nonfinite_set:
            self._nonfinite_set = True
            if hasattr(self.comm, "set_nonfinite"):
                self.comm.set_nonfinite(self.propagate_nonfinite)

    def apply_wire(self) -> None:
        """Once: the communicator's wire for per-block scaled buckets."""
        if self.wire_bits not in (16, 32):
            raise IncclError(f"inccl hook: wire_bits={self.wire_bits!r} is not a wire; 32 (one int32 per element) "
                             f"or 16 (packed 16-bit lanes)")
        if not self._wire_set:
            self._wire_set = True
            if hasattr(self.comm, "set_wire"):
                self.comm.set_wire(inccl.WIRE_P16 if self.wire_bits == 16 else inccl.WIRE_Q32)

    def check_format(self, dtype) -> None:
        """Per-block scaling serves fp32 buckets only: say so here, by name."""
        import torch
        if self.scale_exp == inccl.SCALE_BLOCK and dtype != torch.float32:
            raise IncclError(f"inccl hook: scale_exp=SCALE_BLOCK (per-block auto scaling) takes fp32 gradients only, "
                             f"got {dtype}; use SCALE_AUTO for bf16 / fp16 buckets")
        if self.error_feedback and dtype != torch.float32:
            raise IncclError(f"inccl hook: error_feedback=True takes fp32 gradients only, got {dtype}")

    @property
    def world_size(self) -> int:
        return self.comm.group.world_size


def _scale_name(k) -> str:
    return {inccl.SCALE_AUTO: "SCALE_AUTO", inccl.SCALE_BLOCK: "SCALE_BLOCK"}.get(k, repr(k))


def allreduce_hook(state: HookState, bucket):
    """DDP comm hook: ``bucket.buffer()`` <- mean over ranks, through INCCL.

    The collective runs on the communicator's own stream, after the work queued
    so far on the current stream (the gradients of this bucket), so the backward
    pass keeps computing the next buckets' gradients on its stream while this
    one is exchanged -- the overlap DDP gets from its own collectives.  The
    returned future is CUDA-aware: DDP's wait on it orders its copy-back into
    ``.grad`` after the reduction."""
    import torch

    buf = bucket.buffer()
    name = {torch.float32: "allreduce_f32", torch.bfloat16: "allreduce_bf16", torch.float16: "allreduce_f16"}.get(buf.dtype)
    if name is None:
        raise IncclError(f"inccl DDP hook: fp32, bf16 or fp16 gradient buckets only, got {buf.dtype}")
    state.check_format(buf.dtype)
    reduce = getattr(state.comm, name)
    state.apply_nonfinite()
    state.apply_wire()
    w = state.world_size
    divide = state.average and w > 1 and not state.fold_average()
    if not buf.is_cuda:   # reaches the communicator, which refuses it ("must live on the GPU")
        reduce([buf], out=buf, scale_exp=state.scale_exp, stream=None)
        if divide:
            buf.div_(w)
        fut = torch.futures.Future()
    else:
        side = torch.cuda.ExternalStream(state.comm.stream, device=buf.device)
        side.wait_stream(torch.cuda.current_stream(buf.device))
        with torch.cuda.stream(side):
            if state.error_feedback:   # the residual is allocated on, and only touched on, `side`
                state.comm.allreduce_f32_ef([buf], [state.residual(bucket, buf)], out=buf, stream=side.cuda_stream)
            else:
                reduce([buf], out=buf, scale_exp=state.scale_exp, stream=side.cuda_stream)
            if divide:
                buf.div_(w)
            # the bucket is used on `side` now: the caching allocator must not
            # hand its memory out before this stream's work is done
            buf.record_stream(side)
            fut = torch.futures.Future(devices=[buf.device])
            fut.set_result(buf)   # records an event on `side`; wait() makes the waiter's stream wait on it
    if not buf.is_cuda:
        fut.set_result(buf)
    state.calls += 1
    return fut


def communicator_from_env(port_offset: int = 17, device: int | None = None, engine: str | None = None):
    """Create the INCCL group + communicator for this rank from the torchrun
    environment (RANK, WORLD_SIZE, LOCAL_RANK, MASTER_ADDR, MASTER_PORT).  The
    group's bootstrap listens on MASTER_PORT + ``port_offset`` so it does not
    collide with torch.distributed's own store.  ``engine`` as in
    ``Communicator.set_engine`` (default: the library's choice)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    master = os.environ.get("MASTER_ADDR", "127.0.0.1")
    port = int(os.environ.get("MASTER_PORT", "29500")) + port_offset
    grp = inccl.inccl_group_create(world, rank, master, port=port, device=device)
    if grp is None:
        from ._lib import load
        raise IncclError("inccl_group_create failed: " + load().inccl_last_error().decode(errors="replace"))
    comm = inccl.inccl_communicator_create(grp, 0)
    if comm is None:
        grp.destroy()
        from ._lib import load
        raise IncclError("inccl_communicator_create failed: " + load().inccl_last_error().decode(errors="replace"))
    if engine:
        comm.set_engine(engine)
    return comm


def register(ddp_model, comm, scale_exp: int = inccl.SCALE_AUTO, average: bool = True, wire_bits: int = 32,
             error_feedback: bool = False) -> HookState:
    """Route every gradient bucket of ``ddp_model`` through ``comm``; returns the hook
    state.  ``scale_exp``: a fixed exponent, ``SCALE_AUTO`` (one per bucket) or
    ``SCALE_BLOCK`` (one per 256-element block, fp32 buckets; ``wire_bits=16``:
    exchanged as packed 16-bit lanes; ``error_feedback=True`` with both: what the
    lanes drop is kept per bucket and added to the next step)."""
    state = HookState(comm=comm, scale_exp=scale_exp, average=average, wire_bits=wire_bits,
                      error_feedback=error_feedback)
    ddp_model.register_comm_hook(state, allreduce_hook)
    return state
