#!/usr/bin/env python3
"""Error feedback for packed 16-bit lanes (inccl_*_ef) against the same kernels
without it, on one GPU, R = 2 x 256 MiB fp32 buckets (and as many residuals):

  quant   quant16_ef   inccl_pack_f32_block16_ef    k_pack_block<.., ResPtrs>          (12 R + 2) n + n / 64 bytes
          quant16      F32 -> P16                   k_pack_block                       (4 R + 2) n + n / 64
  absmax  absmax_ef    inccl_block_absmax_f32_ef    k_block_absmax<.., ResPtrs>        8 R n + n / 64
          absmax       inccl_block_absmax_f32       k_block_absmax                     4 R n + n / 64
  fused   fused16_ef   inccl_reduce_f32_block16_ef  k_stream_block_fused<.., ResPtrs>  (12 R + 4) n
          fused16      inccl_reduce_f32_block16     k_stream_block_fused               (4 R + 4) n

The discipline is tools/pack_bench.py's, whose timing it uses: each leg warmed
up, the two legs of a group timed in alternating rounds, a leg's figure the
median of its rounds and its spread (max - min) / median.  Prints one JSON line:
per leg the time per call, TB/s of the algorithmic bytes above and that rate as
a fraction of the 8 TB/s HBM peak; per group the EF leg's time over its plain
sibling's and the ratio the byte counts predict.  Recorded, never a gate.  No
GPU: it fails.

  python tools/ef_bench.py [--mib 256] [--R 2] [--steps 20] [--warmup 5] [--rounds 7] [--json-out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pack_bench import HBM_PEAK, _figure, _time_group  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mib", type=int, default=256, help="MiB per bucket")
    ap.add_argument("--R", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if a.steps < 1 or a.rounds < 1 or a.R < 1 or a.R > 8 or a.mib < 1:
        ap.error("--mib, --steps and --rounds are at least 1, --R is 1..8")

    import torch

    import container_inc_amd
    from container_inc_amd import inccl as K
    container_inc_amd.load()
    if not torch.cuda.is_available():
        raise SystemExit("ef_bench: no GPU (a time measured elsewhere says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    n, R = a.mib * (1 << 20) // 4, a.R
    gen = torch.Generator(device=dev).manual_seed(1000)
    srcs = [torch.randn(n, generator=gen, device=dev, dtype=torch.float32) for _ in range(R)]
    res_t = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(R)]
    out = torch.empty(n, dtype=torch.float32, device=dev)
    pout = torch.empty(n // 2, dtype=torch.int32, device=dev)
    words = K.block_absmax(srcs)
    wout = torch.empty_like(words)
    groups = {
        "quant": {
            "quant16_ef": (lambda: K.pack_block16_ef(srcs, res_t, words, out=pout, scale_R=R),
                           (12 * R + 2) * n + n // 64),
            "quant16": (lambda: K.stream_op_block(K.KIND_F32, K.KIND_P16, srcs, words, out=pout, scale_R=R),
                        (4 * R + 2) * n + n // 64),
        },
        "absmax": {
            "absmax_ef": (lambda: K.block_absmax_ef(srcs, res_t, words=wout), 8 * R * n + n // 64),
            "absmax": (lambda: K.block_absmax(srcs, words=wout), 4 * R * n + n // 64),
        },
        "fused": {
            "fused16_ef": (lambda: K.reduce_f32_block16_ef(srcs, res_t, out=out), (12 * R + 4) * n),
            "fused16": (lambda: K.reduce_f32_block16(srcs, out=out), (4 * R + 4) * n),
        },
    }
    res = {"tool": "ef_bench", "R": R, "mib_per_bucket": a.mib, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "hbm_peak_tbs": HBM_PEAK / 1e12, "device": torch.cuda.get_device_name(0)}
    for legs in groups.values():
        times = _time_group(torch, {k: v[0] for k, v in legs.items()}, a)
        (ef_name, (_, ef_bytes)), (name, (_, nbytes)) = legs.items()
        res[ef_name], res[name] = _figure(times[ef_name], ef_bytes), _figure(times[name], nbytes)
        res[f"{ef_name}_over_{name}"] = round(res[ef_name]["us"] / res[name]["us"], 4)
        res[f"{ef_name}_over_{name}_by_bytes"] = round(ef_bytes / nbytes, 4)
    line = json.dumps(res)
    print(line)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
