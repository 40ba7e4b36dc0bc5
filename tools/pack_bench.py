#!/usr/bin/env python3
"""Packed 16-bit lanes (INCCL_KIND_P16 / INCCL_WIRE_P16) against the 32-bit
lanes of INCCL_SCALE_BLOCK, on one GPU, R = 2 x 256 MiB fp32 buckets:

  stages  quant16    F32 -> P16   k_pack_block     (4 R + 2) n + n / 64 bytes
          quant32    F32 -> Q32   k_stream_block   (4 R + 4) n + n / 64
          dequant16  P16 -> F32   k_unpack_block   (2 R + 4) n + n / 64   (R packed sources)
          dequant32  Q32 -> F32   k_stream_block   (4 R + 4) n + n / 64
  fused   fused16    inccl_reduce_f32_block16      (R + 1) * 4 n  (the same bytes; a clamp per element more)
          fused32    inccl_reduce_f32_block        (R + 1) * 4 n
  step    a W = 2 in-process allreduce (ranks = threads on this GPU) of R x
          --mib per rank under INCCL_SCALE_BLOCK at wire Q32 and at wire P16: a
          ONE-GPU REHEARSAL.  Both ranks share the GPU and the "exchange" is a
          local kernel, so it shows the local stage cost only; the halved xGMI
          traffic of a real exchange is not measured here.

Each leg is warmed up, then the legs of a group are timed in alternating rounds
(HIP events around `steps` back-to-back calls, ending in a synchronise), so that
a drift of the machine falls on all alike; a leg's figure is the median of its
rounds and its spread is (max - min) / median over the rounds.  Prints one JSON
line: per leg the time per call, TB/s of the algorithmic bytes above and that
rate as a fraction of the 8 TB/s HBM peak; the step legs carry no byte count.
No GPU: it fails.

  python tools/pack_bench.py [--mib 256] [--R 2] [--steps 20] [--warmup 5] [--rounds 7] [--json-out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s, MI355X


def _time_group(torch, legs, a, stream=None):
    """{name: [seconds per call, one per round]} of `legs` (name -> callable), alternating"""
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.steps):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3 / a.steps)
    return times


def _figure(ts, nbytes=None):
    t = statistics.median(ts)
    out = {"us": round(t * 1e6, 2), "us_min": round(min(ts) * 1e6, 2), "us_max": round(max(ts) * 1e6, 2),
           "spread": round((max(ts) - min(ts)) / t, 4)}
    if nbytes is not None:
        out.update(algorithmic_bytes=nbytes, tbs=round(nbytes / t / 1e12, 3), hbm_fraction=round(nbytes / t / HBM_PEAK, 3))
    return out


def _step_legs(torch, inccl, dev, a, n):
    """the W = 2 in-process step: rank 1 mirrors rank 0's calls; rank 0 times them"""
    world, out, errs = 2, {}, []
    count = a.warmup + a.rounds * a.steps

    def rank(r):
        try:
            grp = inccl.inccl_group_create_local(world, r, "pack-bench")
            comm = inccl.inccl_communicator_create(grp, 0)
            try:
                gen = torch.Generator(device=dev).manual_seed(2000 + r)
                srcs = [torch.randn(n, generator=gen, device=dev, dtype=torch.float32) for _ in range(a.R)]
                dst = torch.empty(n, dtype=torch.float32, device=dev)
                st = torch.cuda.ExternalStream(comm.stream, device=dev)

                def call(wire):
                    comm.set_wire(wire)
                    comm.allreduce_f32(srcs, out=dst, scale_exp=inccl.SCALE_BLOCK, stream=comm.stream)

                legs = {"step_q32": lambda: call(inccl.WIRE_Q32), "step_p16": lambda: call(inccl.WIRE_P16)}
                if r == 0:
                    out.update(_time_group(torch, legs, a, st))
                else:   # the same calls in the same order
                    for fn in legs.values():
                        for _ in range(a.warmup):
                            fn()
                    for _ in range(a.rounds):
                        for fn in legs.values():
                            for _ in range(a.steps):
                                fn()
                torch.cuda.synchronize()
                comm.barrier()
            finally:
                comm.destroy()
                grp.destroy()
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=600)
    if errs or any(t.is_alive() for t in ts):
        raise SystemExit(f"pack_bench: the W = 2 step failed ({errs or 'a rank did not finish'}; {count} calls per leg)")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mib", type=int, default=256, help="MiB per bucket")
    ap.add_argument("--R", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the W = 2 in-process step")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if a.steps < 1 or a.rounds < 1 or a.R < 1 or a.R > 8 or a.mib < 1:
        ap.error("--mib, --steps and --rounds are at least 1, --R is 1..8")

    import torch

    import container_inc_amd
    from container_inc_amd import inccl
    container_inc_amd.load()
    if not torch.cuda.is_available():
        raise SystemExit("pack_bench: no GPU (a time measured elsewhere says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    n, R = a.mib * (1 << 20) // 4, a.R
    gen = torch.Generator(device=dev).manual_seed(1000)
    srcs = [torch.randn(n, generator=gen, device=dev, dtype=torch.float32) for _ in range(R)]
    out = torch.empty(n, dtype=torch.float32, device=dev)
    words = inccl.block_absmax(srcs)
    q32 = [inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_Q32, [s], words, scale_R=R) for s in srcs]
    p16 = [inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_P16, [s], words, scale_R=R) for s in srcs]
    qout, pout = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n // 2, dtype=torch.int32, device=dev)
    K = inccl
    stage = {
        "quant16": (lambda: K.stream_op_block(K.KIND_F32, K.KIND_P16, srcs, words, out=pout, scale_R=R),
                    (4 * R + 2) * n + n // 64),
        "quant32": (lambda: K.stream_op_block(K.KIND_F32, K.KIND_Q32, srcs, words, out=qout, scale_R=R),
                    (4 * R + 4) * n + n // 64),
        "dequant16": (lambda: K.stream_op_block(K.KIND_P16, K.KIND_F32, p16, words, out=out, n=n, scale_R=R),
                      (2 * R + 4) * n + n // 64),
        "dequant32": (lambda: K.stream_op_block(K.KIND_Q32, K.KIND_F32, q32, words, out=out, scale_R=R),
                      (4 * R + 4) * n + n // 64),
    }
    fused = {
        "fused16": (lambda: K.reduce_f32_block16(srcs, out=out), (R + 1) * 4 * n),
        "fused32": (lambda: K.reduce_f32_block(srcs, out=out), (R + 1) * 4 * n),
    }
    res = {"tool": "pack_bench", "R": R, "mib_per_bucket": a.mib, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "hbm_peak_tbs": HBM_PEAK / 1e12, "device": torch.cuda.get_device_name(0)}
    for group in (stage, fused):
        times = _time_group(torch, {k: v[0] for k, v in group.items()}, a)
        for name, (_, nbytes) in group.items():
            res[name] = _figure(times[name], nbytes)
    res["quant16_over_quant32"] = round(res["quant16"]["us"] / res["quant32"]["us"], 4)
    res["dequant16_over_dequant32"] = round(res["dequant16"]["us"] / res["dequant32"]["us"], 4)
    res["fused16_over_fused32"] = round(res["fused16"]["us"] / res["fused32"]["us"], 4)
    if not a.no_step:
        del q32, p16, qout, pout
        for name, ts in _step_legs(torch, inccl, dev, a, n).items():
            res[name] = _figure(ts)
        res["step_p16_over_step_q32"] = round(res["step_p16"]["us"] / res["step_q32"]["us"], 4)
        res["step_note"] = ("one-GPU rehearsal, W = 2 in-process: both ranks share this GPU and the exchange is a local "
                            "kernel; the local stage cost only -- the halved xGMI traffic is not measured")
    line = json.dumps(res)
    print(line)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
