"""TEST INFRASTRUCTURE ONLY -- the case matrix, the references and the per-rank
runner of the communicator-level guard tests (tests/test_gpu_comm_guards.py:
ranks are threads or one RCCL rank; tests/test_gpu_engine_guards.py: one process
per rank on the IPC engines).

Every case is one call of a communicator whose dst, sources and residuals are
tests/guarded.py buffers, and is checked three ways: the result bit for bit
against the reference the project uses for its mode, both guards of dst, and
every source (and every residual's guards) as uploaded.  An in-place call's
dst is srcs[0]'s guarded view.  A case the API refuses asserts the refusal
and an untouched dst.

Where the sizes come from, with S = 64 W (inccl_shard_elems pads a shard to 64
elements, so W * shard > n for almost every n):

  1          one element: every rank but the first owns padding alone
  65         one full shard and one element: ranks 2.. own nothing
  2 S        total == n: the gather lands in dst in place
  2 S - 61   a ragged last shard, odd, n % 4 == 3, a 16-bit tail element
  2 S + 2    n % 4 == 2, the widest padding (S - 2 elements)
  1287       block modes: five 256-element blocks and 7 elements, odd

dst sits 16-B aligned and one element further (fp32: 4 B; bf16 / fp16: 2 B, the
workspace copy-out of allreduce_body), and for the 2-byte kinds two elements
further (4-B aligned: the element path of the p2p gather).  Reduce-scatter
shards: 4 (the smallest IPC_P2P_RS / IPC_LL_RS), 64 (IPC_MESH_RS), 68 (p2p, not
mesh), 1001 (AR_SHARD; on the packed wire an odd rank * shard starts at a word's
high lane)."""
import zlib
from collections import namedtuple

import numpy as np

import block16_ef_ref as ef_ref
import block16_ref
import block_ref
from guarded import SENT, Buf

R = 2                 # local buckets of every rank
K_FIXED = 20          # the fixed exponent: |x| < 2048 does not saturate, the inputs are N(0, 2)
RS_SHARDS = (4, 64, 68, 1001)
EF_STEPS = 2          # the second step consumes the first one's residuals
KINDS = ("f32", "bf16", "f16")

Case = namedtuple("Case", "op kind scale n shift chunks inplace average refuse", defaults=(1, False, False, None))
# op     "ar" allreduce, "rs" reduce-scatter, "ef" allreduce_f32_ef
# scale  an exponent, "auto", "block" (INCCL_SCALE_BLOCK) or "p16" (... on INCCL_WIRE_P16)
# refuse None, or a piece of the error the API must answer with


def name(c):
    return (f"{c.op}-{c.kind}-{c.scale}-n{c.n}-shift{c.shift}" + (f"-chunks{c.chunks}" if c.chunks != 1 else "")
            + ("-inplace" if c.inplace else "") + ("-avg" if c.average else "") + ("-refused" if c.refuse else ""))


def sizes(W, block=False):
    S = 64 * W
    return (1, 65, 2 * S, 2 * S - 61, 2 * S + 2) + ((1287,) if block else ())


def shifts(kind):
    return (0, 1) if kind == "f32" else (0, 1, 2)


PARTS = ("f32", "bf16", "f16", "block", "p16", "ef", "inplace", "rs", "refused")


def cases(W, part):
    """the cases of one part of the matrix at world W"""
    if part in KINDS:
        return [Case("ar", part, s, n, sh) for s in (K_FIXED, "auto") for n in sizes(W) for sh in shifts(part)]
    if part in ("block", "p16"):
        return [Case("ar", "f32", part, n, sh) for n in sizes(W, True) for sh in (0, 1)]
    if part == "ef":
        return [Case("ef", "f32", "p16", n, sh) for n in sizes(W, True) for sh in (0, 1)]
    if part == "chunks":   # three pieces of the RSAG route (per-block exponents: every piece starts at its own block)
        return ([Case("ar", "f32", K_FIXED, n, sh, chunks=3) for n in sizes(W) for sh in (0, 1)]
                + [Case("ar", "f32", "block", n, 1, chunks=3) for n in sizes(W, True)])
    if part == "inplace":
        return ([Case("ar", k, "auto", n, sh, inplace=True) for k in KINDS for n in sizes(W) for sh in shifts(k)]
                + [Case(op, "f32", s, n, 1, inplace=True) for op, s in (("ar", "block"), ("ar", "p16"), ("ef", "p16"))
                   for n in sizes(W, True)])
    if part == "rs":
        return ([Case("rs", k, s, W * shard, sh) for k in KINDS for s in (K_FIXED, "auto") for shard in RS_SHARDS
                 for sh in (0, 1)]
                + [Case("rs", "f32", s, W * shard, sh) for s in ("block", "p16") for shard in RS_SHARDS for sh in (0, 1)])
    if part == "refused":
        return [Case("ar", "bf16", "block", 65, 0, refuse="not available for bf16 / fp16 buckets"),
                Case("rs", "f32", K_FIXED, W * 64, 0, inplace=True, refuse="dst overlaps srcs[0]")]
    if part == "average":   # once per mode; a power-of-two world
        n = 2 * 64 * W - 61
        return ([Case("ar", k, "auto", n, 1, average=True) for k in KINDS]
                + [Case("ar", "f32", "block", n, 1, average=True), Case("ar", "f32", "p16", n, 1, average=True),
                   Case("ef", "f32", "p16", n, 1, average=True), Case("rs", "f32", "auto", W * 68, 1, average=True),
                   Case("rs", "bf16", K_FIXED, W * 64, 1, average=True),
                   Case("rs", "f32", "p16", W * 1001, 1, average=True)])
    raise ValueError(part)


def _bucket(rng, n, kind):
    x = rng.standard_normal(n).astype(np.float32) * 2.0
    if kind == "f32":
        return x
    if kind == "bf16":
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    return x.astype(np.float16).view(np.uint16)


def _mixed(rng, n, RW):
    return block_ref.mixed_buckets(rng, n, RW, zero_block=1 if block_ref.nblocks(n) > 1 else None)


def _mean16(bits, W):
    """sum / W of a bf16 result in its own format, as tests/test_gpu_comm.py takes the bf16 mean"""
    import torch
    t = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)
    return (t / W).view(torch.int16).numpy().view(np.uint16)


def prepare(O, W, c):
    """{"inputs": [step][rank][r] buckets, "want": [step] (result bits of the
    whole bucket, [rank][r] residuals or None)} of one case; a refused case has
    inputs alone"""
    rng = np.random.default_rng(zlib.crc32(repr((W,) + tuple(c)).encode()))
    RW = R * W
    shift = W.bit_length() - 1 if c.average else 0
    split = lambda xs: [xs[r * R:(r + 1) * R] for r in range(W)]   # noqa: E731
    if c.op == "ef":
        steps = [_mixed(rng, c.n, RW) for _ in range(EF_STEPS)]
        chain = ef_ref.chain(O, steps, RW, out_shift=shift)
        return {"inputs": [split(s) for s in steps], "want": [(y.view(np.uint32), split(res)) for y, res, _ in chain]}
    if c.scale in ("block", "p16") and c.kind == "f32":
        every = _mixed(rng, c.n, RW)
        fn = block_ref.reduce_f32_block if c.scale == "block" else block16_ref.reduce_f32_block16
        want = None if c.refuse else fn(O, every, RW, out_shift=shift)[0].view(np.uint32)
        return {"inputs": [split(every)], "want": [(want, None)]}
    every = [_bucket(rng, c.n, c.kind) for _ in range(RW)]
    if c.refuse:
        return {"inputs": [split(every)], "want": [(None, None)]}
    amax = {"f32": O.absmax, "bf16": O.absmax_bf16, "f16": O.absmax_f16}[c.kind]
    k = O.choose_scale(amax(every), RW) if c.scale == "auto" else c.scale
    want = {"f32": O.reduce_f32, "bf16": O.reduce_bf16, "f16": O.reduce_f16}[c.kind](every, k)
    if c.kind == "f32":
        want = (want / np.float32(W) if c.average else want).view(np.uint32)
    elif c.average and c.kind == "bf16":
        want = _mean16(want, W)
    elif c.average:   # fp16: sum / W may be subnormal, where dividing the rounded sum would round twice
        want = O.sum_dequant_f16([O.quant_sum_f16(every, k)], k + shift)
    return {"inputs": [split(every)], "want": [(want, None)]}


def _scale_arg(inccl, c):
    return {"auto": inccl.SCALE_AUTO, "block": inccl.SCALE_BLOCK, "p16": inccl.SCALE_BLOCK}.get(c.scale, c.scale)


def run_case(comm, inccl, dev, W, rank, c, prep, stream):
    """one rank's call(s) of one case: the list of what was wrong (empty: all three checks held)"""
    import torch
    from container_inc_amd._lib import IncclError
    bad = []

    def check(what, fn):
        try:
            fn()
        except AssertionError as e:
            bad.append(f"{what}: {' '.join(str(e).split())[:240]}")

    comm.set_average(c.average)
    comm.set_wire(inccl.WIRE_P16 if c.scale == "p16" else inccl.WIRE_Q32)
    n_out = c.n // W if c.op == "rs" else c.n
    dst = None if c.inplace else Buf(dev, c.kind, n_out, None, c.shift)
    res = [Buf(dev, "f32", c.n, np.zeros(c.n, np.float32), c.shift) for _ in range(R)] if c.op == "ef" else []
    for t, step in enumerate(prep["inputs"]):
        srcs = [Buf(dev, c.kind, c.n, x, c.shift) for x in step[rank]]
        out = srcs[0].t[:n_out] if c.inplace else dst.t
        ts = [s.t for s in srcs]
        torch.cuda.synchronize()   # the uploads ran on torch's stream, the call runs on the communicator's
        refused = None
        try:
            if c.op == "ef":
                comm.allreduce_f32_ef(ts, [e.t for e in res], out=out, stream=stream)
            elif c.op == "rs":
                comm.reduce_scatter(ts, out=out, scale_exp=_scale_arg(inccl, c), stream=stream)
            elif c.kind == "f32":
                comm.allreduce_f32(ts, out=out, scale_exp=_scale_arg(inccl, c), chunks=c.chunks, stream=stream)
            else:
                fn = comm.allreduce_bf16 if c.kind == "bf16" else comm.allreduce_f16
                fn(ts, out=out, scale_exp=_scale_arg(inccl, c), stream=stream)
        except IncclError as e:
            refused = str(e)
        if c.refuse:
            if refused is None or c.refuse not in refused:
                bad.append(f"not refused with {c.refuse!r}: {refused!r}")
            if dst is not None:
                check("dst of a refused call", lambda: np.testing.assert_array_equal(dst.bits(), SENT[dst.w]))
            for r, s in enumerate(srcs):
                check(f"srcs[{r}] of a refused call", s.assert_unchanged)
            continue
        if refused is not None:
            bad.append(f"refused: {refused[:240]}")
            continue
        y, wres = prep["want"][t]
        want = y[rank * n_out:(rank + 1) * n_out] if c.op == "rs" else y
        holder = srcs[0] if c.inplace else dst
        check(f"step {t} result", lambda: np.testing.assert_array_equal(holder.bits(), want))
        for r, s in enumerate(srcs):
            if not (c.inplace and r == 0):
                check(f"step {t} srcs[{r}]", s.assert_unchanged)
        for r, e in enumerate(res):
            check(f"step {t} residuals[{r}]",
                  lambda: np.testing.assert_array_equal(e.bits(), wres[rank][r].view(np.uint32)))
    return bad


def run_cases(comm, inccl, dev, W, rank, cs, preps, stream):
    """[(case name, what was wrong)] of one rank; the communicator's average and wire are put back"""
    comm.set_nonfinite(False)
    try:
        return [(name(c), run_case(comm, inccl, dev, W, rank, c, p, stream)) for c, p in zip(cs, preps)]
    finally:
        comm.set_average(False)
        comm.set_wire(inccl.WIRE_Q32)


def prepared_case(W, kind):
    return Case("ar", kind, K_FIXED, 2 * 64 * W - 61, 1)


def run_prepared(comm, inccl, dev, W, rank, c, prep, stream):
    """a prepared allreduce (prepare_allreduce_f32 / _bf16) bound to guarded
    buffers and run twice, dst refilled with the sentinel in between"""
    import torch
    bad = []
    srcs = [Buf(dev, c.kind, c.n, x, c.shift) for x in prep["inputs"][0][rank]]
    dst = Buf(dev, c.kind, c.n, None, c.shift)
    torch.cuda.synchronize()
    make = comm.prepare_allreduce_f32 if c.kind == "f32" else comm.prepare_allreduce_bf16
    op = make([s.t for s in srcs], out=dst.t, scale_exp=c.scale, stream=stream)
    try:
        for run in range(2):
            op()
            try:
                np.testing.assert_array_equal(dst.bits(), prep["want"][0][0])
                for s in srcs:
                    s.assert_unchanged()
            except AssertionError as e:
                bad.append(f"run {run}: {' '.join(str(e).split())[:240]}")
            dst.raw.fill_(SENT[dst.w])
            torch.cuda.synchronize()
    finally:
        op.destroy()
    return [(name(c) + "-prepared", bad)]


def failures(results):
    """the (name, what) pairs of run_cases / run_prepared that did not hold"""
    return [(n, b) for n, b in results if b]
