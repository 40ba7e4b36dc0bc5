"""TEST INFRASTRUCTURE ONLY -- the case tables, the edge-valued buckets and the
per-rank runner of tests/test_gpu_engine_variants.py: the ll and mesh kernels
under the knobs that select their other code paths, and edge values through
every IPC engine.

A V is one case: a comm_guard_cases.Case (run by comm_guard_cases.run_case on
tests/guarded.py buffers: the result bit for bit against the oracle, both guards
of dst, every source as uploaded), the local bucket count R, the kind of its
inputs, and the launch line the library's INCCL_TRACE must show for it.

Inputs
  edge None    N(0, 2), as tests/comm_guard_cases.py
  "fixed"      fp32 N(0, 300) with VALUES32 planted (below), exponent 20
  "auto"       the same without NaN and the infinities, the automatic exponent
  "k16"        bf16 / fp16 N(0, 2) with VALUES16 and RAW16 planted, exponent 20
  rot          three input sets in rotation over 12 calls on one stream with no
               host synchronisation in between (run_rotating)

Planted values sit at element 0, across every shard boundary b * S (S =
inccl_shard_elems(n, W); 13 values from b * S - 6 on, so S - 2 .. S + 2 are
covered) and over the tail, rotated by the contributor's index as _plant of
tests/test_gpu_stream_matrix.py rotates them.  Lanes 20.. and S + 20.. are set
apart (_lanes32 / _lanes16): every contributor saturating the same way, so the
sum of W * R INT32_MAX wraps (6 contributors: -6), and lanes with one large or
one tiny contributor and zeros elsewhere.  At exponent 20 in and out a result's
magnitude stays below 2^31 * 2^-20 = 2048, so no output can overflow a half;
what the 2-byte narrowing can reach is the subnormal range of fp16 (a single
contributor of 2^-20, the wrapped -6 * 2^-20), which edge_prepare asserts of the
oracle's own output."""
import os
import re
import sys
import zlib
from collections import namedtuple

import numpy as np

import comm_guard_cases as cg
from comm_guard_cases import Case
from guarded import Buf

K = cg.K_FIXED            # 20: |x| >= 2048 saturates
ROT_CALLS, ROT_SETS = 12, 3

V = namedtuple("V", "case R edge rot trace", defaults=(2, None, False, None))
# trace  mesh: (n, shard, chunk, nchunks, lag), the grid is the spawn's; ll: (n, grid); None: not an ll / mesh launch

VALUES32 = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 3e38, -3e38, 2048.0, -2048.0, 2047.9998, 5000.0, -1e9]
VALUES16 = [65504.0, np.inf, -np.inf, np.nan, 2.0 ** -20, -3 * 2.0 ** -17, 2048.0, 70000.0, -2048.0, -65504.0]
RAW16 = [0x0001, 0x8001, 0x03FF]   # subnormals of either 2-byte format, as bit patterns


def name(v):
    return cg.name(v.case) + f"-R{v.R}" + (f"-edge-{v.edge}" if v.edge else "") + ("-rot12" if v.rot else "")


def shard_elems(n, W):
    """inccl_shard_elems"""
    return (-(-n // W) + 63) & ~63


def _bits16(kind, x):
    from test_gpu_stream_matrix import BF16, F16, _bits16 as enc
    return enc(BF16 if kind == "bf16" else F16, x)


def _offsets(n, S, W, m):
    return [0] + [b * S - 6 for b in range(1, W) if b * S - 6 < n] + [n - m]


def _plant(x, v, S, W):
    for off in _offsets(x.size, S, W, v.size):
        cut = v[:x.size - off]
        x[off:off + cut.size] = cut


def _lanes32(x, i, S):
    """fp32 contributor i of the set-apart lanes"""
    for base in [b for b in (20, S + 20) if b + 4 <= x.size - 13]:
        x[base] = 5000.0                          # every contributor saturates: the sum wraps
        x[base + 1] = -1e9                        # ... at INT32_MIN: six of them sum to 0
        x[base + 2] = 2047.9998 if i == 1 else 0.0
        x[base + 3] = 1e-45 if i == 0 else -0.0


def _lanes16(kind, h, i, S, RW):
    """2-byte contributor i of the set-apart lanes: all 65504 (saturating, the
    sum wraps to a half-subnormal result), then one contributor and zeros"""
    single = [2.0 ** -20, 3 * 2.0 ** -20, 2.0 ** -15, -(2.0 ** -16), 65504.0, -65504.0, 70000.0, 1023 * 2.0 ** -24]
    for base in [b for b in (20, S + 20) if b + 1 + len(single) <= h.size - 13]:
        h[base] = _bits16(kind, [65504.0])[0]
        for j, s in enumerate(single):
            h[base + 1 + j] = _bits16(kind, [s if i == j % RW else 0.0])[0]


def edge_buckets(kind, edge, n, RW, S, W, seed):
    assert n >= 385 and S >= 192, "the planted ranges and the set-apart lanes need room"
    rng = np.random.default_rng(seed)
    out = []
    for i in range(RW):
        if kind == "f32":
            x = (rng.standard_normal(n) * 300.0).astype(np.float32)
            vals = np.asarray(VALUES32 if edge == "fixed" else [v for v in VALUES32 if np.isfinite(v)], np.float32)
            _plant(x, np.roll(vals, i), S, W)
            _lanes32(x, i, S)
        else:
            x = _bits16(kind, rng.standard_normal(n) * 2.0)
            vals = np.concatenate([_bits16(kind, VALUES16), np.asarray(RAW16, np.uint16)])
            _plant(x, np.roll(vals, i), S, W)
            _lanes16(kind, x, i, S, RW)
        out.append(x)
    return out


def _reduce(O, kind, every, scale, RW):
    amax = {"f32": O.absmax, "bf16": O.absmax_bf16, "f16": O.absmax_f16}[kind]
    k = O.choose_scale(amax(every), RW) if scale == "auto" else scale
    y = {"f32": O.reduce_f32, "bf16": O.reduce_bf16, "f16": O.reduce_f16}[kind](every, k)
    return y.view(np.uint32) if kind == "f32" else y


def _check_edge_reference(O, v, every, want, S, RW):
    """what the buckets were built to reach, shown on the oracle's own numbers"""
    c = v.case
    if c.kind == "f32" and v.edge == "fixed":
        qs = O.quant_sum(every, K)
        assert RW != 6 or (qs[20] == -6 and qs[21] == 0), qs[20:22]
        np.testing.assert_array_equal(O.dequantise(qs, K).view(np.uint32), want)
    if c.kind == "f16":
        sub = (want & 0x7C00 == 0) & (want & 0x03FF != 0)
        assert sub[20] and sub[21], "the wrapped lane and the 2^-20 lane are fp16 subnormals"


def prepare(O, W, v):
    """{"inputs": [set][rank][r], "want": [set] (bits of the whole result, None)} as comm_guard_cases.prepare"""
    c, RW = v.case, v.R * W
    S = shard_elems(c.n, W)
    seed = zlib.crc32(repr((W, v.R, v.edge, v.rot) + tuple(c)).encode())
    rng = np.random.default_rng(seed)
    inputs, want = [], []
    for t in range(ROT_SETS if v.rot else 1):
        every = (edge_buckets(c.kind, v.edge, c.n, RW, S, W, seed + t) if v.edge
                 else [cg._bucket(rng, c.n, c.kind) for _ in range(RW)])
        y = _reduce(O, c.kind, every, c.scale, RW)
        if v.edge:
            _check_edge_reference(O, v, every, y, S, RW)
        inputs.append([every[r * v.R:(r + 1) * v.R] for r in range(W)])
        want.append((y, None))
    return {"inputs": inputs, "want": want}


def run_rotating(comm, dev, rank, v, prep):
    """ROT_CALLS allreduces back to back on one stream with no host
    synchronisation, the input sets in rotation, every output copied on the
    stream right after its call; checked at the end, with dst's guards and
    every source"""
    import torch
    c, bad = v.case, []
    assert c.op == "ar" and not c.inplace
    srcs = [[Buf(dev, c.kind, c.n, x, c.shift) for x in step[rank]] for step in prep["inputs"]]
    dst = Buf(dev, c.kind, c.n, None, c.shift)
    raw = dst.raw[dst.lo:dst.lo + c.n]
    hist = torch.empty((ROT_CALLS, c.n), dtype=raw.dtype, device=dev)
    st = torch.cuda.Stream(device=dev)
    fn = {"f32": comm.allreduce_f32, "bf16": comm.allreduce_bf16, "f16": comm.allreduce_f16}[c.kind]
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for i in range(ROT_CALLS):
            fn([s.t for s in srcs[i % ROT_SETS]], out=dst.t, scale_exp=c.scale, stream=st.cuda_stream)
            hist[i].copy_(raw)
    torch.cuda.synchronize()
    got = hist.cpu().numpy().view(np.uint32 if dst.w == 4 else np.uint16)
    wrong = [i for i in range(ROT_CALLS) if not np.array_equal(got[i], prep["want"][i % ROT_SETS][0])]
    if wrong:
        bad.append(f"wrong outputs at calls {wrong}")
    for what, b in [("dst", dst)] + [(f"set {t} srcs[{r}]", s) for t, ss in enumerate(srcs) for r, s in enumerate(ss)]:
        try:
            b.bits() if b is dst else b.assert_unchanged()
        except AssertionError as e:
            bad.append(f"{what}: {' '.join(str(e).split())[:240]}")
    return bad


def rank_main(rank, world, port, engine, env, vs, trace_path, q):
    """one rank of one spawn: every case of vs on one communicator, the
    library's trace (this process's fd 2) in trace_path with a line naming each
    case before its calls"""
    try:
        fd = os.open(trace_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.dup2(fd, 2)
        os.environ.update({"INCCL_ENGINE": engine, "INCCL_DEVICE": "0", "INCCL_BOOT_TIMEOUT": "120",
                           "INCCL_TRACE": "1", "INCCL_LL_TIMEOUT_MS": "10000"})   # a stall ends as a reported error
        os.environ.update(env)
        from conftest import ROOT
        sys.path.insert(0, ROOT)
        import torch
        from container_inc_amd import inccl
        from oracle import oracle as O
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        preps = [prepare(O, world, v) for v in vs]
        grp = inccl.inccl_group_create(world, rank, "127.0.0.1", port=port, device=0)
        assert grp is not None, "group create failed"
        comm = inccl.inccl_communicator_create(grp, 0)
        assert comm is not None and comm.engine == engine
        res = []
        try:
            comm.set_nonfinite(False)
            for v, p in zip(vs, preps):
                os.write(2, f"[case {name(v)}]\n".encode())
                if v.rot:
                    bad = run_rotating(comm, dev, rank, v, p)
                else:
                    bad = cg.run_case(comm, inccl, dev, world, rank, v.case, p, comm.stream)
                res.append((name(v), bad))
            comm.barrier()
        finally:
            comm.destroy()
            grp.destroy()
        q.put((rank, res, None))
    except BaseException as e:  # noqa: BLE001
        q.put((rank, None, repr(e)))


_MESH = re.compile(r"mesh launch n (\d+) shard (\d+) chunk (\d+) nchunks (\d+) lag (\d+) grid (\d+)")
_LL = re.compile(r"ll launch n (\d+) grid (\d+) protocol (\w+)")


def launches(trace_path):
    """{case name: [launch tuple]} of one rank's trace: mesh (n, shard, chunk,
    nchunks, lag, grid), ll (n, grid, protocol)"""
    out, cur = {}, None
    with open(trace_path, errors="replace") as f:
        for line in f:
            if line.startswith("[case "):
                cur = line[6:].rstrip("]\n")
                out[cur] = []
            m = _MESH.search(line) or _LL.search(line)
            if m and cur is not None:
                out[cur].append(tuple(int(g) if g.isdigit() else g for g in m.groups()))
    return out


# ---- the tables ----
# The trace tuples below are what the tests assert; the docstring of tests/test_gpu_engine_variants.py
# tabulates the same numbers for the reader and is edited together with them.
def ar(kind, n, scale=K, shift=0, inplace=False):
    return Case("ar", kind, scale, n, shift, inplace=inplace)


def rs(kind, n):
    return Case("rs", kind, K, n, 0)


def edges(n, trace, kinds=("f32", "bf16", "f16")):
    """the edge buckets at one size: fp32 at the fixed and the automatic exponent, bf16 and fp16"""
    out = []
    if "f32" in kinds:
        out += [V(ar("f32", n), edge="fixed", trace=trace), V(ar("f32", n, "auto"), edge="auto", trace=trace)]
    return out + [V(ar(k, n), edge="k16", trace=trace) for k in kinds if k != "f32"]


def ll_cases(variant):
    """part 2 of the module's docstring: (world, env, [V]); trace = (n, grid)"""
    if variant == "fence":
        return 3, {"INCCL_LL_PROTOCOL": "fence"}, [
            V(ar("f32", 1), R=2, trace=(1, 1)), V(ar("f32", 1000), R=1, trace=(1000, 1)),
            V(ar("f32", 4099, shift=1), R=3, trace=(4099, 5)),
            V(ar("f32", 3 * 65536 + 5, "auto"), R=2, trace=(196613, 64)),
            V(ar("f32", 262144), R=8, trace=(262144, 64)),
            V(rs("f32", 3 * 4), trace=(12, 1)), V(rs("f32", 3 * 1001 * 4), trace=(12012, 12)),
            V(ar("f32", 4099, inplace=True), trace=(4099, 5)),
            *edges(4099, (4099, 5), ("f32",)),
            V(ar("f32", 4099), rot=True, trace=(4099, 5))]
    if variant == "cap1":
        return 2, {"INCCL_LL_GRID_CAP": "1"}, [
            V(ar("f32", 5271), trace=(5271, 1)), V(ar("f32", 5271, shift=1), trace=(5271, 1)),
            V(rs("f32", 5272), trace=(5272, 1)), *edges(5271, (5271, 1), ("f32",))]
    if variant == "cap2":
        return 3, {"INCCL_LL_GRID_CAP": "2"}, [
            V(ar("f32", 10391), trace=(10391, 2)), V(rs("f32", 10392), trace=(10392, 2)),
            V(ar("f32", 10391, inplace=True), trace=(10391, 2)), V(ar("f32", 10391), rot=True, trace=(10391, 2))]
    if variant == "cap256":
        return 2, {"INCCL_LL_GRID_CAP": "256"}, [
            V(ar("f32", 262144), trace=(262144, 256)), V(ar("f32", 262143, shift=3), trace=(262143, 256))]
    raise ValueError(variant)


LL_VARIANTS = ("fence", "cap1", "cap2", "cap256")

# part 3: row -> (INCCL_MESH_CHUNK, INCCL_MESH_LAG, INCCL_MESH_GRID or None); world 3
MESH_ROWS = {"c64-l1-g4": (64, 1, 4), "c64-l1000": (64, 1000, None), "c192-l2": (192, 2, None),
             "c1088-l1": (1088, 1, None), "c4160-l1": (4160, 1, None), "c64-clamped": (64, 1, None)}
MESHW_ROWS = ("c64-l1-g4", "c192-l2", "c1088-l1")


def mesh_cases(row):
    """[V]; trace = (n, shard, chunk, nchunks, lag)"""
    if row == "c64-l1-g4":
        t = {1: (1, 64, 64, 1, 1), 385: (385, 192, 64, 3, 1), 899: (899, 320, 64, 5, 1), 960: (960, 320, 64, 5, 1)}
        vs = []
        for k in cg.KINDS:
            vs += [V(ar(k, n), trace=t[n]) for n in (1, 385, 899)] + [V(rs(k, 960), trace=t[960])]
        vs += [V(ar("f32", 899, shift=1), trace=t[899]), V(ar("bf16", 899, shift=1), trace=t[899]),
               V(ar("f32", 899, inplace=True), trace=t[899]), V(ar("f32", 899), rot=True, trace=t[899])]
        return vs + edges(385, t[385])
    if row == "c64-l1000":
        return [V(ar("f32", 899), trace=(899, 320, 64, 5, 5))] + edges(899, (899, 320, 64, 5, 5))
    if row == "c192-l2":
        return [V(ar("f32", 899), trace=(899, 320, 192, 2, 2)), V(ar("f32", 2051), trace=(2051, 704, 192, 4, 2)),
                V(rs("f32", 3 * 704), trace=(2112, 704, 192, 4, 2))] + edges(899, (899, 320, 192, 2, 2))
    if row == "c1088-l1":
        t = (6659, 2240, 1088, 3, 1)
        return [V(ar("f32", 6659), trace=t), V(ar("bf16", 6659), trace=t)] + edges(6659, t)
    if row == "c4160-l1":
        t = (25147, 8384, 4160, 3, 1)
        return [V(ar("f32", 25147), trace=t), V(ar("f32", 25147, shift=1), trace=t)] + edges(25147, t)
    if row == "c64-clamped":
        t = (196795, 65600, 128, 513, 1)
        return [V(ar("f32", 196795), trace=t)] + edges(196795, t)
    raise ValueError(row)


def mesh_env(row):
    chunk, lag, grid = MESH_ROWS[row]
    env = {"INCCL_LL_MAX_BYTES": "0", "INCCL_MESH_CHUNK": str(chunk), "INCCL_MESH_LAG": str(lag)}
    if grid:
        env["INCCL_MESH_GRID"] = str(grid)
    return env


def default_edge_cases(engine):
    """part 4 at default knobs, world 3: (env, [V])"""
    if engine == "p2p":
        return {"INCCL_LL_MAX_BYTES": "0"}, edges(899, None) + edges(3 * 4096 + 5, None)
    if engine == "ll":   # fp32 through the ll kernel; the 2-byte kinds take the engine's AR route
        return {}, edges(4099, (4099, 5), ("f32",)) + edges(4099, None, ("bf16", "f16"))
    return {"INCCL_LL_MAX_BYTES": "0"}, (edges(899, (899, 320, 320, 1, 1))
                                         + edges(3 * 4096 + 5, (12293, 4160, 4096, 2, 2)))
