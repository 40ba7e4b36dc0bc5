#!/usr/bin/env python3
"""Per-block auto scaling against the two scales it sits between, on one GPU:
the fused bucket reduce of R = 2 x 256 MiB fp32 buckets at

  fixed   a fixed exponent, k = 25          inccl_reduce_f32        (R + 1) * 4 n bytes
  auto    INCCL_SCALE_AUTO                  inccl_reduce_f32_auto   (2 R + 1) * 4 n bytes
                                            (absmax pass + fused pass: the buckets are read twice)
  block   INCCL_SCALE_BLOCK                 inccl_reduce_f32_block  (R + 1) * 4 n bytes (one pass)

Each leg is warmed up, then the legs are timed in alternating rounds (HIP
events around `steps` back-to-back calls, ending in a synchronise), so that a
drift of the machine falls on all three alike; the figure of a leg is the
median of its rounds and its spread is (max - min) / median over the rounds.
Prints one JSON line: per leg the time per call, TB/s of the algorithmic bytes
above and that rate as a fraction of the 8 TB/s HBM peak.  No GPU: it fails.

  python tools/block_bench.py [--mib 256] [--R 2] [--steps 20] [--warmup 5] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mib", type=int, default=256, help="MiB per bucket")
    ap.add_argument("--R", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if a.steps < 1 or a.rounds < 1 or a.R < 1 or a.mib < 1:
        ap.error("--mib, --R, --steps and --rounds are at least 1")

    import torch

    import container_inc_amd
    from container_inc_amd import inccl
    container_inc_amd.load()
    if not torch.cuda.is_available():
        raise SystemExit("block_bench: no GPU (a time measured elsewhere says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    n = a.mib * (1 << 20) // 4
    gen = torch.Generator(device=dev).manual_seed(1000)
    srcs = [torch.randn(n, generator=gen, device=dev, dtype=torch.float32) for _ in range(a.R)]
    out = torch.empty(n, dtype=torch.float32, device=dev)
    word = torch.zeros(4, dtype=torch.int32, device=dev)
    legs = {
        "fixed": (lambda: inccl.reduce_f32(srcs, 25, out=out), (a.R + 1) * 4 * n),
        "auto": (lambda: inccl.reduce_f32_auto(srcs, out=out, word=word), (2 * a.R + 1) * 4 * n),
        "block": (lambda: inccl.reduce_f32_block(srcs, out=out), (a.R + 1) * 4 * n),
    }
    for fn, _ in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, (fn, _) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3 / a.steps)
    res = {"tool": "block_bench", "R": a.R, "mib_per_bucket": a.mib, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "hbm_peak_tbs": HBM_PEAK / 1e12, "device": torch.cuda.get_device_name(0)}
    for name, (_, nbytes) in legs.items():
        t = statistics.median(times[name])
        res[name] = {"us": round(t * 1e6, 2), "us_min": round(min(times[name]) * 1e6, 2),
                     "us_max": round(max(times[name]) * 1e6, 2),
                     "spread": round((max(times[name]) - min(times[name])) / t, 4), "algorithmic_bytes": nbytes,
                     "tbs": round(nbytes / t / 1e12, 3), "hbm_fraction": round(nbytes / t / HBM_PEAK, 3)}
    res["block_over_auto"] = round(res["block"]["us"] / res["auto"]["us"], 4)
    res["block_over_fixed"] = round(res["block"]["us"] / res["fixed"]["us"], 4)
    line = json.dumps(res)
    print(line)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
