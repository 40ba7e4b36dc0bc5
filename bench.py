"""bench.py -- BASELINE.json metric: GB/s of device-resident fp32 gradient buckets
quantised + reduced (+ dequantised), 256 MiB per bucket, 1/2/4/8 GPUs.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

A plain run does what the headline needs and no more: it sets up, settles and
warms up, times the K steps, writes the last timed step's result if
--dump-outputs is given (DIR/out.npy, float32: the reduced bucket, or a fixed
seeded lane sample of a large one -- dump_lanes), and prints the line (N > 1:
the engine candidates are still verified and timed first, since the fastest
verified one is the headline).  Everything else this file measures or checks
-- the oracle parity checks, rooflines, per-stage times, CPU baselines, sizes,
other precisions, the N > 1 sweep: the "Extra JSON fields" below -- runs only
with --full, after the headline, and leaves the headline as it is.

`python bench.py --gpus N` (N > 1, no WORLD_SIZE) starts its N ranks itself
through torch.distributed.run before touching the GPU; WORLD_SIZE != --gpus is
an error.  Whatever happens, rank 0's one JSON line gets printed: a watchdog
timed from process start (INCCL_BENCH_BUDGET, 480 s) prints it with the stuck
stage and exits 3, and a helper process prints it if rank 0 dies after the
headline (LineKeeper); both carry an "error" key and leave a non-zero status.

Workload (one "step"): every rank holds R = 2 resident 256 MiB fp32 buckets
(the reference's FAN_IN = 2 children per switch, non_termination_switch.c:23)
and produces their allreduce over all ranks into a third buffer:
  N = 1   one fused HIP kernel: dequant(sum_r quant(x_r))          (config 2)
  N > 1   the exchange engine that is fastest during warmup among rccl
          (quant + local sum -> RCCL reduce-scatter int32 -> dequant shard ->
          RCCL all-gather), ar, a2a, p2p, mesh and meshw, all bit-identical
          (config 4; DESIGN.md "Multi-GPU"); then the config 5 size sweep.
          Two phases: the RCCL engines are tuned and a full headline is
          measured with the fastest BEFORE the library's IPC engines (never
          run across separate GPUs) are tried; an IPC engine that tunes faster
          is measured the same way, and the faster measured headline is the
          line (`headline_candidates` lists both).  An IPC engine that faults or
          hangs leaves the RCCL headline to the line keeper / watchdog.
value = bucket bytes reduced per second over the whole job = N * R * 256 MiB / t.

Extra JSON fields (--full):
  roofline          N = 1: the fused kernel's HBM roofline (algorithmic bytes
                    (R+1)*4*n per launch, timed with HIP events on its own stream).
                    N > 1: the step's xGMI link roofline; the quant+sum kernel's
                    HBM figure is roofline_hbm_kernel
  cpu_baseline      the C oracle on a bounded sample, rank 0 at N = 1 only
  parity_vs_oracle  the timed engine's result at 2^20 strided lanes plus every
                    shard / chunk boundary, every rank's inputs gathered to rank 0
                    and checked bit for bit by the C oracle (also per engine
                    candidate, sweep row and bf16 row, on smaller samples)
  runtime           the HIP / HSA / RCCL libraries this rank mapped
  sizes             N = 1: 4 KiB .. 1 GiB buckets (north_star's 4/64/256/1024 MiB among them):
                    call latency eager / prepared / graph-replayed, kernel time, GB/s + HBM fraction
  roofline_cold     N = 1: the fused kernel rotating through input sets far larger
                    than the 256 MiB Infinity Cache
  r_variants        N = 1: config 2's R = 1 and R = 8 at 256 MiB, repeated and rotated
  numerics_vs_exact N = 1: error vs the exact (fp64) sum, R = 2 and 8, k = 25 and auto
  host_e2e          N = 1: BASELINE config 3, 1 GiB pinned host fp32 in 64 MiB buckets
  api_allreduce_write N = 1: the reference's entry point on a 256 MiB host int32
                    message, registered and unregistered
  f16               N = 1: the same for IEEE float16 buckets (k_stream16<F16,F16,R>);
                    N > 1: inccl_allreduce_f16 on the same engines as bf16, verified
  bf16              N = 1: R bf16 buckets of 256 MiB (k_stream16), repeated and rotated;
                    N > 1: inccl_allreduce_bf16 on the rccl, p2p, mesh and meshw engines, verified
  reduce_scatter    N > 1: inccl_reduce_scatter_f32 of R x 256 MiB per rank on rccl and p2p, each
                    rank's shard checked against the oracle
  sweep             N > 1: 4 KiB .. 256 MiB and 1 GiB per engine, verified with
                    alternating input sets
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
TUNE_CALLS = 10         # timed calls per engine candidate (after TUNE_CALLS / 2 untimed ones)
T_START = time.monotonic()
# what the process is doing now; the watchdog and the line keeper name it
STAGE = {"stage": "start"}
KEEPER = [None]   # rank 0's LineKeeper
RESULT = [None]   # the result dict once the headline is measured
PHASES = {}       # wall seconds of each phase of the run, in order (the line's "phase_s")
SWEEP_ROWS = []   # N > 1: the size sweep's rows as they finish (the line's "sweep")


class Phase:
    """Records the wall seconds of one phase of the run into PHASES."""

    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        self.t0 = time.monotonic()
        return self

    def __exit__(self, *exc):
        PHASES[self.name] = round(time.monotonic() - self.t0, 1)
        if KEEPER[0] is not None:
            KEEPER[0].update()
        return False


def set_stage(stage: str) -> None:
    STAGE["stage"] = stage
    if KEEPER[0] is not None:
        KEEPER[0].update()


class LineKeeper:
    """Rank 0's guarantee that the run prints its JSON line even if rank 0
    dies (a GPU fault, a signal) after the headline is measured.

    A helper process, started before this process touches the GPU and in a
    session of its own (so a launcher's kill of the rank's process group does
    not reach it), blocks on a pipe from rank 0.  Rank 0 keeps a state file
    current: the result so far, the stage it is in, and whether the line has
    been printed.  When the pipe closes -- rank 0 exited for any reason -- the
    helper prints nothing if the line was printed, else the result so far
    with an "error" naming the stage rank 0 died in (or a null-valued line
    if the headline never existed).  The exit status stays the launcher's:
    non-zero for a rank that died."""

    def __init__(self):
        import subprocess
        import tempfile
        fd, self.path = tempfile.mkstemp(prefix="inccl_bench_line_", suffix=".json")
        os.close(fd)
        self.printed = False
        self.update()
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--line-keeper", self.path],
                                     stdin=subprocess.PIPE, start_new_session=True)

    def update(self, printed: bool = False) -> None:
        self.printed = self.printed or printed
        state = {"res": RESULT[0], "stage": STAGE["stage"], "printed": self.printed,
                 "elapsed_s": round(time.monotonic() - T_START, 1)}
        tmp = self.path + ".tmp"
        try:
            with open(tmp, "w") as f:
                json.dump(state, f)
            os.replace(tmp, self.path)
        except (OSError, TypeError, ValueError) as e:   # never costs the run
            print(f"bench: line keeper state not written: {e!r}", file=sys.stderr, flush=True)


def line_keeper_main(path: str) -> None:
    """The helper side of LineKeeper: wait for rank 0 to exit, then print its
    line if it did not."""
    try:
        sys.stdin.buffer.read()   # EOF when rank 0's end of the pipe closes
    except OSError:
        pass
    try:
        with open(path) as f:
            state = json.load(f)
    except (OSError, ValueError):
        state = {"res": None, "stage": "unknown (no state file)", "printed": False}
    if not state.get("printed"):
        msg = f"rank 0 exited without printing its line, during: {state.get('stage')}"
        res = state.get("res")
        if res is None:
            res = {"metric": METRIC, "value": None, "unit": "GB/s"}
            msg += " (before the headline was measured)"
        else:
            msg += "; headline measured and kept, later keys partial"
        res["error"] = msg
        res.setdefault("elapsed_s", state.get("elapsed_s"))
        print(json.dumps(res), flush=True)
    for q in (path, path + ".tmp"):
        try:
            os.remove(q)
        except OSError:
            pass


def self_launch(a) -> int:
    """--gpus N > 1 with no WORLD_SIZE in the environment: start the N rank
    processes ourselves (torch.distributed.run as a child, one rank per GPU,
    rendezvous on 127.0.0.1) and return their exit code.  Runs before this
    process touches the GPU; rank 0's JSON line reaches stdout directly."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"bench: launching {a.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.call(cmd)


class Watchdog:
    """Bounds the whole run from process start.  A collective that never
    returns cannot be interrupted, so when the budget is spent this thread
    emits what has been measured (rank 0), names the stage it was stuck in,
    and ends the process with exit code 3: a hang never reads as success.
    The budget default (480 s) sits well below the driver's 600 s limit."""

    def __init__(self, budget_s: float, rank: int):
        self.rank = rank
        self.on_fire = None   # set once the headline exists: emits it with the error
        self.t = threading.Timer(max(1.0, budget_s - (time.monotonic() - T_START)), self.fire)
        self.t.daemon = True
        self.budget_s = budget_s
        self.t.start()

    def fire(self):
        msg = f"watchdog: run exceeded {self.budget_s:.0f} s from process start, stuck in: {STAGE['stage']}"
        print(f"rank {self.rank}: {msg}", file=sys.stderr, flush=True)
        if self.on_fire is not None:
            self.on_fire(msg)
        elif self.rank == 0:
            print(json.dumps({"metric": METRIC, "value": None, "unit": "GB/s", "error": msg}), flush=True)
            if KEEPER[0] is not None:
                KEEPER[0].update(printed=True)
        os._exit(3)

    def cancel(self):
        self.t.cancel()


METRIC = "GB/s device-resident fp32 bucket quantise+reduce, 256 MiB, 1/2/4/8 GPUs"


def oracle_lanes(n: int, world: int, chunks: int, target: int) -> "list[int]":
    """A deterministic lane sample of an n-element bucket: `target` evenly
    strided lanes plus both sides of every shard and chunk boundary any engine
    uses (the rank shards of chunk_plan, the plain n*g/W split, the mesh chunks'
    256 KiB grid) and both ends."""
    from container_inc_amd.plan import chunk_plan
    stride = max(1, n // max(1, target))
    lanes = set(range(0, n, stride))
    cuts = {0, n}
    for off, cnt, shard in chunk_plan(n, world, chunks):
        for g in range(world + 1):
            cuts.add(min(n, off + g * shard))
        cuts.add(off + cnt)
    for g in range(world + 1):
        cuts.add(n * g // world)
    for c in range(0, n, 1 << 16):   # 256 KiB of fp32: the mesh engines' chunk grid
        cuts.add(c)
    for c in cuts:
        for d in (-1, 0):
            if 0 <= c + d < n:
                lanes.add(c + d)
    return sorted(lanes)


def oracle_check(srcs, out, lanes, k: int, rank: int, world: int, fmt: str = "f32") -> dict:
    """The C oracle as the checker of an N-rank result (outside any timed
    region): every rank's R inputs and its output at `lanes` are gathered to
    rank 0 over gloo; rank 0 runs orc_reduce_f32 (orc_reduce_bf16 / _f16 for
    fmt "bf16" / "f16") on all W*R
    inputs -- the reference's sum over every child, non_termination_switch.c:361-372,
    behind the quantiser -- and compares every rank's output bit for bit."""
    import numpy as np
    import torch
    import torch.distributed as dist
    idx = torch.as_tensor(lanes, dtype=torch.int64, device=out.device)
    rows = [s.index_select(0, idx) for s in srcs] + [out.index_select(0, idx)]
    mine = torch.stack(rows).cpu()
    # gloo gathers no 16-bit integers: 16-bit patterns travel widened to int32
    b16 = fmt != "f32"
    mine = mine.view(torch.int16).to(torch.int32) if b16 else mine.view(torch.int32)
    if world > 1:
        bucket = [torch.empty_like(mine) for _ in range(world)] if rank == 0 else None
        dist.gather(mine, gather_list=bucket, dst=0)
    else:
        bucket = [mine]
    res = {"lanes": len(lanes), "ranks": world, "mismatches": None,
           "checker": "oracle/inccl_oracle.c orc_reduce_" + fmt}
    if rank == 0:
        from oracle import oracle as O
        R = len(srcs)
        arr = [b.numpy() for b in bucket]
        if b16:
            red = O.reduce_bf16 if fmt == "bf16" else O.reduce_f16
            want = red([a[j].astype(np.uint16) for a in arr for j in range(R)], k).view(np.uint16)
            got = [a[R].astype(np.uint16) for a in arr]
        else:
            want = O.reduce_f32([a[j].view(np.float32) for a in arr for j in range(R)], k).view(np.uint32)
            got = [a[R].view(np.uint32) for a in arr]
        res["mismatches"] = int(sum(np.count_nonzero(g != want) for g in got))
    return res


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--bucket-mib", type=int, default=256)
    p.add_argument("--local-buckets", type=int, default=2)
    p.add_argument("--scale-exp", type=int, default=25)
    p.add_argument("--chunks", type=int, default=0, help="pipelined chunks for the rccl engine (0 = tune)")
    p.add_argument("--engine", default="auto", choices=["auto", "rccl", "ar", "a2a", "p2p", "mesh", "meshw"],
                   help="N>1 exchange engine; auto = time every candidate during warmup, keep the fastest")
    p.add_argument("--no-sweep", action="store_true", help="N>1: skip the bucket-size sweep (BASELINE config 5)")
    p.add_argument("--settle-seconds", type=float, default=1.0,
                   help="untimed steps before the W warmup steps, until this much wall time has passed: the first "
                        "launches over freshly allocated buckets run up to 2x slower, and the first process on a "
                        "fresh box runs ~3%% slower for its first ~0.25 s of load (launch_drift_probe.py)")
    p.add_argument("--cpu-seconds", type=float, default=10.0)
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-extras", action="store_true",
                   help="N=1: skip the size list, cold-input run, numerics and host-memory (config 3) keys")
    p.add_argument("--grid-cap", type=int, default=0)
    p.add_argument("--json-out", default="")
    p.add_argument("--full", action="store_true",
                   help="beyond the headline: the oracle parity checks, rooflines and per-stage times, and the extra "
                        "keys (CPU baselines, sizes, other precisions, the N>1 sweep, ...); off, the run only sets "
                        "up, warms up, times --steps steps and prints the line")
    p.add_argument("--dump-outputs", default="", metavar="DIR",
                   help="after the timed steps, write what the last timed step computed to DIR/out.npy (float32; "
                        "of a bucket above DUMP_MAX_ELEMS elements a fixed, seeded lane sample)")
    a = p.parse_args(argv)
    if a.steps < 1:
        p.error("--steps must be at least 1")
    return a


# --dump-outputs: at most 2^23 fp32 values (32 MiB) of the reduced bucket
DUMP_MAX_ELEMS = 1 << 23
DUMP_SEED = 20240


def dump_lanes(n: int) -> "np.ndarray | None":
    """The lanes of an n-element result that --dump-outputs writes: all of
    them (None) up to DUMP_MAX_ELEMS, else one lane out of each of
    DUMP_MAX_ELEMS contiguous, near-equal parts of the bucket, at an offset
    drawn from a fixed seed -- the same lanes in every run and every build,
    in increasing order."""
    import numpy as np
    if n <= DUMP_MAX_ELEMS:
        return None
    edges = np.arange(DUMP_MAX_ELEMS + 1, dtype=np.int64) * n // DUMP_MAX_ELEMS
    rng = np.random.default_rng(DUMP_SEED)
    return edges[:-1] + (rng.random(DUMP_MAX_ELEMS) * (edges[1:] - edges[:-1])).astype(np.int64)


def write_outputs(directory: str, arrays: dict) -> None:
    """DIR/<name>.npy for every array the timed path returned (float32)."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    for name, arr in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float32))


def cpu_baseline(n_elems: int, R: int, k: int, seconds: float) -> dict:
    """The C restatement (oracle/inccl_oracle.c, scalar, 1 core) on a bounded
    sample of the same workload: R buckets of 16 Mi elements (64 MiB each)."""
    import numpy as np

    from oracle import oracle as O
    O.build()
    m = min(n_elems, 1 << 24)
    rng = np.random.default_rng(1000)
    xs = [rng.standard_normal(m).astype(np.float32) for _ in range(R)]
    out = None
    t0 = time.perf_counter()
    iters = 0
    while True:
        out = O.reduce_f32(xs, k)
        iters += 1
        if time.perf_counter() - t0 >= seconds:
            break
    dt = time.perf_counter() - t0
    del out
    return {"value": round(iters * R * m * 4 / dt / 1e9, 4), "unit": "GB/s", "cores": 1, "kind": "port",
            "sample": f"{iters} x fused quantise+sum+dequantise of R={R} x {m * 4 >> 20} MiB fp32 buckets "
                      f"(oracle/inccl_oracle.c orc_reduce_f32, 1 thread, {dt:.1f} s)"}


def cpu_baseline_allcores(n_elems: int, R: int, k: int, seconds: float) -> dict:
    """The same restatement on every host core: threads over disjoint 1 Mi-element
    chunks of the sample (ctypes releases the GIL inside the C loop)."""
    import threading

    import numpy as np

    from oracle import oracle as O
    # the GPU box exposes the whole machine's CPUs; our share is $OMP_NUM_THREADS (16)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = max(1, min(cores, int(os.environ.get("OMP_NUM_THREADS", "16") or 16), 64))
    m = min(n_elems, 1 << 24)
    rng = np.random.default_rng(1000)
    xs = [rng.standard_normal(m).astype(np.float32) for _ in range(R)]
    out = np.empty(m, np.float32)
    chunk = 1 << 20
    jobs = [(o, min(m, o + chunk)) for o in range(0, m, chunk)]
    L = O.lib()

    def worker(tid, stop_at, counter):
        while time.perf_counter() < stop_at:
            for j in range(tid, len(jobs), cores):
                lo, hi = jobs[j]
                srcs = (O.ctypes.c_void_p * R)(*[x[lo:hi].ctypes.data for x in xs])
                L.orc_reduce_f32(srcs, R, out[lo:hi].ctypes.data, hi - lo, k)
                counter[tid] += hi - lo

    counter = [0] * cores
    t0 = time.perf_counter()
    th = [threading.Thread(target=worker, args=(t, t0 + seconds, counter)) for t in range(cores)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    return {"value": round(sum(counter) * R * 4 / dt / 1e9, 4), "unit": "GB/s", "cores": cores, "kind": "port",
            "sample": f"orc_reduce_f32 over 1 Mi-element chunks of R={R} x {m * 4 >> 20} MiB buckets on {cores} "
                      f"threads for {dt:.1f} s"}


def cpu_reference_pipeline(seconds: float) -> dict:
    """BASELINE config 1 as SURVEY.md §8(d) states it: the reference's own
    per-element CPU path restated end to end -- encode (api.c:300-302) -> root
    switch add per 1 KiB packet (nts.c:361-363) -> egress frame build + ICRC per
    child (util.c:331-442) -> decode (api.c:428-430) -- on one 4 MiB bucket per
    rank, in one thread (oracle orc_allreduce_write_loopback with framing), at
    2 ranks (the reference's FAN_IN, nts.c:23) and at 8 ranks (FAN_IN
    generalised to one switch with 8 children).  Each rank count runs on int32
    buckets (the reference's data) and on fp32 buckets through the quantiser
    (orc_quantise_f32 before the encode, orc_dequantise_q32 after the decode,
    k = 25).  Every run's result is checked against the plain sum."""
    import numpy as np

    from oracle import oracle as O
    m = 1 << 20   # 4 MiB bucket per rank (BASELINE config 1)
    k = 25
    rows = []
    per = seconds / 4
    for W in (2, 8):
        rng = np.random.default_rng(1)
        xi = [rng.integers(-2 ** 31, 2 ** 31 - 1, m, dtype=np.int64).astype(np.int32) for _ in range(W)]
        xf = [rng.standard_normal(m).astype(np.float32) for _ in range(W)]
        want_i = O.sum_q32(xi)
        want_f = O.reduce_f32(xf, k)
        for kind in ("int32", "fp32"):
            t0 = time.perf_counter()
            iters, ok = 0, True
            while True:
                if kind == "int32":
                    rc, dsts, _ = O.allreduce_write_loopback(xi, with_icrc=True)
                    ok = ok and all(np.array_equal(d, want_i) for d in dsts)
                else:
                    rc, dsts, _ = O.allreduce_write_loopback([O.quantise(x, k) for x in xf], with_icrc=True)
                    outs = [O.dequantise(d, k) for d in dsts]
                    ok = ok and all(np.array_equal(o.view(np.uint32), want_f.view(np.uint32)) for o in outs)
                assert rc == m // 1024
                iters += 1
                if time.perf_counter() - t0 >= per:
                    break
            dt = time.perf_counter() - t0
            rows.append({"ranks": W, "data": kind, "iters": iters, "ms_per_allreduce": round(dt / iters * 1e3, 2),
                         "GBps_one_rank_bucket": round(iters * m * 4 / dt / 1e9, 4),
                         "GBps_all_ranks": round(iters * W * m * 4 / dt / 1e9, 4), "correct": bool(ok)})
    head = rows[0]
    return {"value": head["GBps_one_rank_bucket"], "unit": "GB/s of one rank's int32 bucket", "cores": 1,
            "kind": "port", "configs": rows,
            "sample": f"loopback inccl_allreduce_write of 4 MiB per rank with switch aggregation and ICRC framing, "
                      f"2 and 8 ranks, int32 and quantised fp32; `value` = 2 ranks int32, {head['iters']} calls"}


# 4 KiB (one reference message, api.h:39) .. 256 MiB in x4 steps (BASELINE config 5),
# plus north_star's 1024 MiB point
SWEEP_BYTES = [(4 << 10) << (2 * i) for i in range(9)] + [1 << 30]
# xGMI: 7 links per MI355X, 153.6 GB/s per link counting both directions (AMD's
# per-link figure; 76.8 GB/s each way).  A rank of a W-GPU full mesh has W-1 links.
XGMI_LINK_GBS_BIDIR = 153.6


def xgmi_roofline(world: int, bucket_bytes: int, seconds: float) -> dict:
    """Link roofline of one N>1 step: RS + AG move (W-1)/W of the bucket out of
    every rank and (W-1)/W into it, twice (int32 partials, fp32 results):
    4 (W-1)/W B bytes across the rank's W-1 links, both directions counted,
    against (W-1) x 153.6 GB/s."""
    link_bytes = 4 * (world - 1) * bucket_bytes // world
    achieved = link_bytes / seconds / 1e9
    peak = (world - 1) * XGMI_LINK_GBS_BIDIR
    return {"bound": "xgmi", "achieved": round(achieved, 1), "peak": round(peak, 1), "unit": "GB/s",
            "frac": round(achieved / peak, 4), "traffic": None, "link_bytes_per_rank_per_step": link_bytes,
            "peak_source": f"{world - 1} xGMI links x 153.6 GB/s (both directions; 76.8 GB/s each way)"}


def run_verified(comm, eng: str, ch: int, inputs, out, k: int, stream, refs):
    """Three calls alternating two input sets (A, B, A), each compared with the
    reference engine's results.  Identical inputs on every call would hide a
    buffer that is read stale; alternating them cannot.  Returns the three
    outputs and whether they match `refs` (or, with no refs yet, whether the
    two A calls agree with each other)."""
    import torch
    got = []
    for xs in (inputs[0], inputs[1], inputs[0]):
        comm.allreduce_f32(xs, out=out, scale_exp=k, chunks=ch, stream=stream.cuda_stream)
        torch.cuda.synchronize()
        got.append(out.clone())
        # the clone runs on torch's stream, the next call on `stream`: without
        # this wait the next call can overwrite lanes of `out` before the clone
        # has read them (seen as "the previous call's values on some lanes")
        torch.cuda.synchronize()
    if refs is None:
        same = bool(torch.equal(got[0], got[2]))
    else:
        same = all(bool(torch.equal(g, refs[i % 2])) for i, g in enumerate(got))
    return got, same


def agree(values, world: int):
    """Max over ranks of a list of floats (gloo)."""
    import torch
    import torch.distributed as dist
    v = torch.tensor(values, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(v, op=dist.ReduceOp.MAX)
    return v.tolist()


def stage_probe(comm, xs, out, k: int, chunks: int, st, world: int, calls: int = 3) -> dict:
    """Where one allreduce's time goes (N > 1): `calls` untimed calls with
    per-stage HIP events (inccl_comm_set_stage_timing), after the timed ones;
    per stage the mean microseconds over the calls, max over ranks, plus the
    call's wall span and the overlap between stages (sum - wall: the pipelined
    rccl path quantises chunk i+1 beside chunk i's collectives).  Stages:
    quant (+ local sum), reduce_scatter (int32), dequant, all_gather, copy,
    allreduce (the "ar" engine's ncclAllReduce), ipc (an IPC engine's whole
    exchange: its kernels do every stage)."""
    import torch
    names = list(comm.STAGE_NAMES) + ["wall_us", "overlap_us"]
    acc = {key: 0.0 for key in names}
    # ranks arrive skewed (rank 0 has just run the oracle check): one untimed call
    # after a barrier absorbs that, so no stage counts a wait for a late peer
    agree([0.0], world)
    comm.allreduce_f32(xs, out=out, scale_exp=k, chunks=chunks, stream=st.cuda_stream)
    torch.cuda.synchronize()
    try:
        comm.set_stage_timing(True)
        for _ in range(calls):
            comm.allreduce_f32(xs, out=out, scale_exp=k, chunks=chunks, stream=st.cuda_stream)
            torch.cuda.synchronize()
            t = comm.stage_times()
            for key in names:
                acc[key] += t.get(key, 0.0) / calls
    finally:
        comm.set_stage_timing(False)
    v = agree([acc[key] for key in names], world)
    return {key: round(x, 2) for key, x in zip(names, v) if x != 0.0 or key == "overlap_us"}


def graph_replay_us(comm, xs, out, k: int, st, world: int, want, per: int = 20, reps: int = 10):
    """Latency floor of a small bucket: `per` calls captured in one hipGraph
    (torch.cuda.CUDAGraph around the C-ABI call), replayed `reps` times; µs per
    call, max over ranks, or None if any rank could not capture.  The replayed
    output must still equal the reference engine's."""
    import torch
    g = torch.cuda.CUDAGraph()
    ok = 1
    try:
        with torch.cuda.graph(g, stream=st):
            for _ in range(per):
                comm.allreduce_f32(xs, out=out, scale_exp=k, stream=st.cuda_stream)
    except Exception:  # noqa: BLE001 -- an engine with host synchronisation cannot be captured
        ok = 0
    if agree([0.0 if ok else 1.0], world)[0] != 0.0:   # every rank replays, or none does
        return None, None
    g.replay()
    torch.cuda.synchronize()
    agree([0.0], world)
    t0 = time.perf_counter()
    for _ in range(reps):
        g.replay()
    torch.cuda.synchronize()
    dt = agree([(time.perf_counter() - t0) / (reps * per)], world)[0]
    same = agree([0.0 if want is None or torch.equal(out, want) else 1.0], world)[0] == 0.0
    del g
    return dt, same


SMALL_ENGINES = ("rccl", "ar", "p2p", "ll", "mesh", "meshw")   # buckets up to 1 MiB
LARGE_ENGINES = ("rccl", "ar", "a2a", "p2p", "mesh", "meshw")


def size_sweep(comm, dev, R: int, k: int, rank: int, world: int, soft_budget_s: float, rows: list,
               want=lambda eng: True, ref_of=None) -> list:
    """BASELINE config 5 at N > 1 (and north_star's 1024 MiB point): per bucket
    size and engine, host wall time per call over back-to-back calls (max over
    ranks), GB/s, the xGMI link fraction, whether the results of two
    alternating input sets are bit-identical to the first engine's, and a
    sampled oracle check of each engine's result (`parity_vs_oracle`).
    Rows are appended to `rows` as they finish (the watchdog reports a partial
    sweep).  A size is started only while every rank is within
    `soft_budget_s` of process start; the rest are skipped and listed.

    `want(engine)` selects this pass's engines: the sweep runs in two passes
    (RCCL first, so that its rows exist before anything else runs, then the
    rest).  `ref_of` maps a size to the engine whose results were the
    reference in an earlier pass; that engine is re-run untimed first, so the
    later pass compares against the same reference."""
    import torch
    import torch.distributed as dist
    ref_of = {} if ref_of is None else ref_of
    for b in SWEEP_BYTES:
        engines = SMALL_ENGINES if b <= (1 << 20) else LARGE_ENGINES
        only = os.environ.get("INCCL_BENCH_SWEEP_ENGINES")   # debugging aid: a subset, in this order
        if only:
            engines = tuple(e for e in only.split(",") if e in engines)
        engines = tuple(e for e in engines if want(e))
        if not engines:
            continue
        if agree([time.monotonic() - T_START], world)[0] > soft_budget_s:
            rows.append({"bucket_bytes": b, "engines": list(engines),
                         "skipped": f"run past {soft_budget_s:.0f} s from process start"})
            continue
        n = b // 4
        lanes = oracle_lanes(n, world, 1, 4096)
        inputs = []
        for seed in (7000, 8000):
            gen = torch.Generator(device=dev)
            gen.manual_seed(seed + rank)
            inputs.append([torch.randn(n, generator=gen, device=dev) for _ in range(R)])
        out = torch.empty(n, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()   # inputs made on torch's stream; the calls run on st
        refs = None
        iters = 50 if b <= (1 << 20) else (10 if b <= (256 << 20) else 4)
        # the reference engine is the first that passes on every rank: RCCL, or
        # else the host-synchronised p2p exchange, before the in-kernel ll protocol
        if b in ref_of:   # an earlier pass's reference, recomputed untimed
            set_stage(f"sweep {b} B reference {ref_of[b]}")
            ok = 1
            try:
                comm.set_engine(ref_of[b])
                got, _ = run_verified(comm, ref_of[b], 1, inputs, out, k, st, None)
            except Exception as e:  # noqa: BLE001
                print(f"rank {rank}: sweep {b} B reference {ref_of[b]} failed: {e}", file=sys.stderr, flush=True)
                ok, got = 0, None
            if agree([0.0 if ok else 1.0], world)[0] == 0.0:
                refs = (got[0], got[1])
            del got
        for eng in engines:
            if agree([time.monotonic() - T_START], world)[0] > soft_budget_s:   # the budget holds per engine too
                rows.append({"bucket_bytes": b, "engine": eng,
                             "skipped": f"run past {soft_budget_s:.0f} s from process start"})
                continue
            set_stage(f"sweep {b} B engine {eng}")
            ok, dt, dtp, same, got = 1, float("inf"), float("inf"), False, None
            try:
                comm.set_engine(eng)
                got, same = run_verified(comm, eng, 1, inputs, out, k, st, refs)
                # untimed calls first: an engine's buffers may just have been
                # (re)allocated for this size, and the first passes over fresh
                # memory run slow (launch_drift_probe.py)
                for _ in range(max(3, iters // 2)):
                    comm.allreduce_f32(inputs[0], out=out, scale_exp=k, stream=st.cuda_stream)
                torch.cuda.synchronize()
                dist.barrier()
                t0 = time.perf_counter()
                for _ in range(iters):
                    comm.allreduce_f32(inputs[0], out=out, scale_exp=k, stream=st.cuda_stream)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / iters
                # up to 4 MiB, the same call prepared once
                # (inccl_op_create_allreduce_f32): without the per-call argument
                # marshalling of the binding (above that it is noise)
                dtp = float("nan")
                if b <= (4 << 20):
                    op = comm.prepare_allreduce_f32(inputs[0], out=out, scale_exp=k, stream=st.cuda_stream)
                    for _ in range(max(3, iters // 2)):
                        op()
                    torch.cuda.synchronize()
                    dist.barrier()
                    t0 = time.perf_counter()
                    for _ in range(iters):
                        op()
                    torch.cuda.synchronize()
                    dtp = (time.perf_counter() - t0) / iters
                    op.destroy()
            except Exception as e:  # noqa: BLE001
                print(f"rank {rank}: sweep {b} B engine {eng} failed: {e}", file=sys.stderr, flush=True)
                ok = 0
            v = agree([dt if ok else float("inf"), 0.0 if ok else 1.0, 0.0 if same else 1.0,
                       dtp if ok else float("inf")], world)
            good, ident = v[1] == 0.0, v[2] == 0.0
            if good and ident and refs is None:
                refs = (got[0], got[1])
                ref_of[b] = eng
            if rank == 0:
                print(f"sweep {b} B {eng}: ok={good} identical={ident} us={v[0] * 1e6:.1f}", file=sys.stderr,
                      flush=True)
            row = {"bucket_bytes": b, "engine": eng, "ok": good, "bit_identical": good and ident,
                   "us": round(v[0] * 1e6, 2) if good else None,
                   "prepared_us": round(v[3] * 1e6, 2) if good and b <= (4 << 20) else None,
                   "algbw_GBps": round(b / v[0] / 1e9, 2) if good else None,
                   "value_GBps": round(world * R * b / v[0] / 1e9, 2) if good else None}
            if good:
                row["parity_vs_oracle"] = oracle_check(inputs[0], got[0], lanes, k, rank, world)
                row["xgmi_frac"] = xgmi_roofline(world, b, v[0])["frac"]
                if b <= (1 << 20) and eng != "p2p":   # the small-message floor without host launch cost
                    gdt, gsame = graph_replay_us(comm, inputs[0], out, k, st, world, refs[0] if refs else None)
                    row["graph_us"] = round(gdt * 1e6, 2) if gdt is not None else None
                    row["graph_bit_identical"] = gsame
            rows.append(row)
            del got
        del inputs, out, refs
        torch.cuda.empty_cache()
    return rows


def bf16_engines(comm, dev, R: int, rank: int, world: int, mib: int = 256, fmt: str = "bf16") -> list:
    """N > 1: R resident `mib` MiB bf16 (fmt "f16": IEEE fp16) buckets per rank
    through inccl_allreduce_bf16 / _f16 on the engines with a 2-byte result
    exchange (rccl: ncclAllGather of 2-byte words; p2p: 2-byte result shards
    gathered; mesh / meshw: 2-byte result chunks), each verified
    bit-identical to the first engine that passes on every rank over two
    alternating input sets; wall time per call, max over ranks, and the xGMI link
    fraction of its (W-1)/W * n * (4 + 2) bytes."""
    import torch
    import torch.distributed as dist

    n = mib * (1 << 20) // 2
    dtype = torch.float16 if fmt == "f16" else torch.bfloat16
    allreduce = comm.allreduce_f16 if fmt == "f16" else comm.allreduce_bf16
    inputs = []
    for seed in (9000, 9500):
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed + rank)
        inputs.append([torch.randn(n, generator=gen, device=dev).to(dtype) for _ in range(R)])
    out = torch.empty(n, device=dev, dtype=dtype)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    rows, refs = [], None
    lanes = oracle_lanes(n, world, 1, 1 << 16)
    for eng in ("rccl", "p2p", "mesh", "meshw"):
        set_stage(f"{fmt} {mib} MiB engine {eng}")
        ok, dt, same = 1, float("inf"), False
        try:
            comm.set_engine(eng)
            got = []
            for xs in (inputs[0], inputs[1], inputs[0]):
                allreduce(xs, out=out, scale_exp=25, stream=st.cuda_stream)
                torch.cuda.synchronize()
                got.append(out.clone())
                torch.cuda.synchronize()
            same = (torch.equal(got[0], got[2]) if refs is None
                    else all(torch.equal(g, refs[i % 2]) for i, g in enumerate(got)))
            for _ in range(5):
                allreduce(inputs[0], out=out, scale_exp=25, stream=st.cuda_stream)
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(10):
                allreduce(inputs[0], out=out, scale_exp=25, stream=st.cuda_stream)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 10
        except Exception as e:  # noqa: BLE001
            print(f"rank {rank}: {fmt} engine {eng} failed: {e}", file=sys.stderr, flush=True)
            ok, got = 0, None
        v = agree([dt if ok else float("inf"), 0.0 if ok else 1.0, 0.0 if same else 1.0], world)
        good, ident = v[1] == 0.0, v[2] == 0.0
        if good and ident and refs is None:
            refs = (got[0], got[1])
        row = {"engine": eng, "bucket_mib": mib, "R": R, "ok": good, "bit_identical": good and ident,
               "ms": round(v[0] * 1e3, 4) if good else None}
        if good:
            row["parity_vs_oracle"] = oracle_check(inputs[0], got[0], lanes, 25, rank, world, fmt=fmt)
            link = (world - 1) * n * 6 // world
            row["GBps_buckets"] = round(world * R * 2 * n / v[0] / 1e9, 1)
            # both directions counted, as xgmi_roofline does: (W-1)/W * n * (4 + 2) bytes out and as many in
            row["xgmi_frac"] = round(2 * link / v[0] / 1e9 / ((world - 1) * XGMI_LINK_GBS_BIDIR), 4)
        rows.append(row)
        del got
    del inputs, out, refs
    torch.cuda.empty_cache()
    return rows


def rs_oracle_check(srcs, out_shard, lanes, k: int, rank: int, world: int) -> dict:
    """oracle_check for a reduce-scatter: every rank's inputs at `lanes` and its
    shard's values at the lanes inside its shard go to rank 0, which runs
    orc_reduce_f32 on all W*R inputs and compares each rank's lanes bit for bit."""
    import numpy as np
    import torch
    import torch.distributed as dist
    n = srcs[0].numel()
    shard = n // world
    idx = torch.as_tensor(lanes, dtype=torch.int64, device=out_shard.device)
    own = [(i, l - rank * shard) for i, l in enumerate(lanes) if rank * shard <= l < (rank + 1) * shard]
    full = torch.zeros(len(lanes), dtype=torch.float32, device=out_shard.device)
    if own:
        pos = torch.as_tensor([i for i, _ in own], dtype=torch.int64, device=out_shard.device)
        loc = torch.as_tensor([j for _, j in own], dtype=torch.int64, device=out_shard.device)
        full.index_copy_(0, pos, out_shard.index_select(0, loc))
    mine = torch.stack([s.index_select(0, idx) for s in srcs] + [full]).cpu().view(torch.int32)
    if world > 1:
        bucket = [torch.empty_like(mine) for _ in range(world)] if rank == 0 else None
        dist.gather(mine, gather_list=bucket, dst=0)
    else:
        bucket = [mine]
    res = {"lanes": len(lanes), "ranks": world, "mismatches": None,
           "checker": "oracle/inccl_oracle.c orc_reduce_f32, each rank's shard"}
    if rank == 0:
        from oracle import oracle as O
        R = len(srcs)
        arr = [b.numpy() for b in bucket]
        want = O.reduce_f32([a[j].view(np.float32) for a in arr for j in range(R)], k).view(np.uint32)
        lane = np.asarray(lanes)
        bad, by_rank = 0, {}
        for r, a in enumerate(arr):
            sel = (lane >= r * shard) & (lane < (r + 1) * shard)
            nb = int(np.count_nonzero(a[R].view(np.uint32)[sel] != want[sel]))
            bad += nb
            if nb:
                by_rank[r] = nb
        res["mismatches"] = bad
        if by_rank:   # which ranks' shards, out of how many lanes each
            res["mismatches_by_rank"] = by_rank
            res["lanes_per_rank"] = int(np.count_nonzero((lane >= 0) & (lane < shard)))
    return res


def reduce_scatter_engines(comm, dev, R: int, rank: int, world: int, mib: float = 256,
                           engines=("rccl", "p2p"), inputs=None, first_out=None) -> list:
    """N > 1: inccl_reduce_scatter_f32 of R resident `mib` MiB fp32 buckets per
    rank (each rank keeps its 1/W shard of the reduced bucket: the sharded-
    gradient callers' half of the allreduce) on rccl (ncclReduceScatter) and p2p
    (pull-reduce into the shard), each verified bit-identical to the first engine
    that passes, over two alternating input sets, and against the oracle on
    every rank's shard; wall time per call (max over ranks) and the xGMI link
    fraction of its (W-1)/W * n * 4 bytes."""
    import torch
    import torch.distributed as dist
    n = int(mib * (1 << 20)) // 4 if inputs is None else inputs[0][0].numel()
    if n % world:
        return [{"skipped": f"{n} elements do not split into {world} shards"}]
    # (inputs / first_out: diagnostics, tools/rs_leg_probe.py -- given input sets,
    # and each engine's first output kept)
    given, inputs = inputs, [] if inputs is None else list(inputs)
    for seed in (9100, 9600) if given is None else ():
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed + rank)
        inputs.append([torch.randn(n, generator=gen, device=dev) for _ in range(R)])
    out = torch.empty(n // world, device=dev, dtype=torch.float32)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    rows, refs = [], None
    lanes = oracle_lanes(n, world, 1, 1 << 16)
    for eng in engines:
        set_stage(f"reduce_scatter {mib} MiB engine {eng}")
        ok, dt, same = 1, float("inf"), False
        try:
            comm.set_engine(eng)
            got = []
            for xs in (inputs[0], inputs[1], inputs[0]):
                comm.reduce_scatter(xs, out=out, scale_exp=25, stream=st.cuda_stream)
                torch.cuda.synchronize()
                got.append(out.clone())
                # the clone runs on torch's stream and the next call on `st`:
                # without this wait the next call overwrote `out` under the clone
                # (round 6: the first call's copy held the second call's result
                # on one or two of eight ranks sharing a GPU, every engine alike)
                torch.cuda.synchronize()
            same = (torch.equal(got[0], got[2]) if refs is None
                    else all(torch.equal(g, refs[i % 2]) for i, g in enumerate(got)))
            if first_out is not None:
                first_out[eng] = got[0].clone()
            for _ in range(5):
                comm.reduce_scatter(inputs[0], out=out, scale_exp=25, stream=st.cuda_stream)
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(10):
                comm.reduce_scatter(inputs[0], out=out, scale_exp=25, stream=st.cuda_stream)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 10
        except Exception as e:  # noqa: BLE001
            print(f"rank {rank}: reduce_scatter engine {eng} failed: {e}", file=sys.stderr, flush=True)
            ok, got = 0, None
        v = agree([dt if ok else float("inf"), 0.0 if ok else 1.0, 0.0 if same else 1.0], world)
        good, ident = v[1] == 0.0, v[2] == 0.0
        if good and ident and refs is None:
            refs = (got[0], got[1])
        row = {"engine": eng, "bucket_mib": mib, "R": R, "ok": good, "bit_identical": good and ident,
               "ms": round(v[0] * 1e3, 4) if good else None}
        if good:
            row["parity_vs_oracle"] = rs_oracle_check(inputs[0], got[0], lanes, 25, rank, world)
            if not (good and ident):   # the third verification call (inputs[0] again) checked as well
                row["parity_vs_oracle_call3"] = rs_oracle_check(inputs[0], got[2], lanes, 25, rank, world)
            link = (world - 1) * n * 4 // world
            row["GBps_buckets"] = round(world * R * 4 * n / v[0] / 1e9, 1)
            # both directions counted: (W-1)/W * n * 4 bytes out and as many in
            row["xgmi_frac"] = round(2 * link / v[0] / 1e9 / ((world - 1) * XGMI_LINK_GBS_BIDIR), 4)
        rows.append(row)
        del got
    del inputs, out, refs
    torch.cuda.empty_cache()
    return rows


def kernel_time_ms(fn, stream, iters: int) -> float:
    """Mean device time of fn() (one launch on `stream`) from HIP events on that stream."""
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters



def switch_batch(dev, fan_in: int = 2, P: int = 1 << 16, iters: int = 20, acks: bool = False) -> dict:
    """The GPU switch dataplane (nts.c:303-501 parse / aggregate / replay / ACK
    reflection, util.c:331-442 egress frames + ICRC) on one batch of fan_in x P
    RoCEv2 data frames, every port of every PSN once: `inccl_switch_batch` =
    claim, classify, sum, egress.  acks=True: every data frame is followed by
    its sender's ACK for that PSN (the reference's RDMA-WRITE flow: each
    downstream packet draws an ACK that the switch reflects, nts.c:403-406), so
    the batch holds 2 fan_in P frames and egress also builds fan_in P 62-B ACKs.
    Batches alternate between the two halves of a 2P-slot ring, so each batch's
    recycle (slot psn + slots/2, nts.c:367) clears the other half and no reset
    runs between batches.  Device time per batch from HIP events on its stream.
    Checked without the oracle: every PSN completes exactly once per batch,
    every completed frame's fan_in rows carry a frame length and every ACK its
    port's 62-B row."""
    import numpy as np
    import torch

    from container_inc_amd import inccl
    stride = 1152
    n = fan_in * P
    rng = np.random.default_rng(7)
    psn = np.repeat(np.arange(P, dtype=np.uint32), fan_in)
    ports = np.tile(np.arange(fan_in, dtype=np.int32), P)
    op = np.where(psn % 4 == 0, 0x06, np.where(psn % 4 == 3, 0x08, 0x07)).astype(np.uint8)   # WRITE_FIRST, MIDDLE, LAST
    wf = op == 0x06
    frames = np.zeros((n, stride), np.uint8)
    udp_len = (8 + 12 + 1024 + 4 + np.where(wf, 16, 0)).astype(np.uint32)   # nts.c:349
    frames[:, 38], frames[:, 39] = udp_len >> 8, udp_len & 0xFF
    frames[:, 42] = op
    pay = rng.integers(0, 256, (n, 1024), dtype=np.uint8)
    for sel, off in ((wf, 70), (~wf, 54)):
        frames[sel, off:off + 1024] = pay[sel]
    is_ack = np.zeros(n, bool)
    if acks:   # data frame i at row 2 i, its sender's ACK at row 2 i + 1
        both = np.zeros((2 * n, stride), np.uint8)
        both[0::2] = frames
        both[1::2, 38], both[1::2, 39], both[1::2, 42] = 0, 28, 0x11   # 62-B ACK: UDP length 28, opcode 0x11
        frames, psn, ports = both, np.repeat(psn, 2), np.repeat(ports, 2)
        is_ack = np.tile(np.array([False, True]), n)
    total = len(frames)

    def with_psns(base):
        f = frames.copy()
        q = np.where(is_ack, psn + base, (psn + base) | 0x80000000)   # ACKs carry no ack-request bit (util.c:387-388)
        f[:, 50], f[:, 51], f[:, 52], f[:, 53] = q >> 24, (q >> 16) & 0xFF, (q >> 8) & 0xFF, q & 0xFF
        return torch.from_numpy(f).to(dev)

    batches = [with_psns(0), with_psns(P)]
    pt = torch.from_numpy(ports).to(dev)
    sw = inccl.GpuSwitch(fan_in, 2 * P)
    tmpl = np.zeros(fan_in, inccl.FRAME_TEMPLATE_DTYPE)
    tmpl["qp"], tmpl["src_port"], tmpl["dst_port"] = 0x11, 4791, 4791
    tmpl_dev = torch.from_numpy(tmpl.view(np.uint8).copy()).to(dev)
    st = torch.cuda.Stream(device=dev)
    out = torch.empty((total * fan_in, stride), dtype=torch.uint8, device=dev)
    out_len = torch.empty(total * fan_in, dtype=torch.int32, device=dev)
    action = torch.empty(total, dtype=torch.int32, device=dev)
    psn_out = torch.empty(total, dtype=torch.int32, device=dev)
    turn = [0]

    def one():
        x = batches[turn[0] % 2]
        turn[0] += 1
        sw.batch(x, pt, tmpl_dev, stream=st.cuda_stream, out=out, out_len=out_len, action=action, psn=psn_out)

    one()
    torch.cuda.synchronize()
    a = action.cpu().numpy()
    lens = out_len.cpu().numpy().reshape(total, fan_in)
    done = a == inccl.SW_COMPLETED
    ok = int(done.sum()) == P and bool((lens[done] > 0).all())
    if acks:
        ack_rows = lens[is_ack, :]
        ok = ok and bool((a[is_ack] == inccl.SW_ACK).all())
        ok = ok and bool((ack_rows[np.arange(n), ports[is_ack]] == 62).all()) and int((ack_rows > 0).sum()) == n
        ok = ok and bool((lens[~done & ~is_ack] == 0).all())
    else:
        ok = ok and bool((lens[~done] == 0).all())
    ms = kernel_time_ms(one, st, iters)
    sw.destroy()
    return {"what": "inccl_switch_batch: claim / classify / sum / egress (frames + ICRC) of one batch"
                    + (", every data frame followed by its sender's ACK (reflected, nts.c:403-406)" if acks else ""),
            "fan_in": fan_in, "psns": P, "frames": total, "data_frames": n, "ack_frames": n if acks else 0,
            "us_per_batch": round(ms * 1e3, 2), "payload_GBs": round(n * 1024 / (ms * 1e-3) / 1e9, 1),
            "frames_per_s": round(total / (ms * 1e-3)), "every_psn_completes_once": ok,
            "timing": "HIP events on the batch's stream, eager calls"}


def switch_nonroot_round(dev, fan_in: int = 2, P: int = 1 << 16, iters: int = 20) -> dict:
    """The non-root switch (nts.c:376-400, :408-423, :457-499) on one round of
    P PSNs: an up batch of fan_in x P child frames (every PSN's aggregate
    FORWARDed to the parent once its last child arrives) and a down batch of
    the parent's P results (each taken and sent to every child, DOWN).  With
    INCCL_SW_RECYCLE (the reference never recycles a non-root slot, so its ring
    serves one pass and no steady state exists); rounds alternate between the
    two halves of a 2P-slot ring, each round's results clearing the other half.
    Device time per round (both batches) from HIP events on their stream.
    Checked without the oracle: every PSN forwards once and takes its result
    once, and the rows written are exactly those."""
    import numpy as np
    import torch

    from container_inc_amd import inccl
    stride = 1152
    rng = np.random.default_rng(8)
    F = fan_in

    def frames_for(psn, op):
        n = len(psn)
        f = np.zeros((n, stride), np.uint8)
        wf = op == 0x06
        udp_len = (8 + 12 + 1024 + 4 + np.where(wf, 16, 0)).astype(np.uint32)
        f[:, 38], f[:, 39], f[:, 42] = udp_len >> 8, udp_len & 0xFF, op
        pay = rng.integers(0, 256, (n, 1024), dtype=np.uint8)
        for sel, off in ((wf, 70), (~wf, 54)):
            f[sel, off:off + 1024] = pay[sel]
        q = psn | 0x80000000
        f[:, 50], f[:, 51], f[:, 52], f[:, 53] = q >> 24, (q >> 16) & 0xFF, (q >> 8) & 0xFF, q & 0xFF
        return torch.from_numpy(f).to(dev)

    up_psn = np.repeat(np.arange(P, dtype=np.uint32), F)
    up_ports = torch.from_numpy(np.tile(np.arange(F, dtype=np.int32), P)).to(dev)
    dn_psn = np.arange(P, dtype=np.uint32)
    dn_ports = torch.full((P,), F, dtype=torch.int32, device=dev)
    opof = lambda p: np.where(p % 4 == 0, 0x06, np.where(p % 4 == 3, 0x08, 0x07)).astype(np.uint8)
    rounds = [(frames_for(up_psn + base, opof(up_psn)), frames_for(dn_psn + base, opof(dn_psn))) for base in (0, P)]
    sw = inccl.GpuSwitch(F, 2 * P, nonroot=True, flags=inccl.SW_RECYCLE)
    tmpl = np.zeros(F + 1, inccl.FRAME_TEMPLATE_DTYPE)
    tmpl["qp"], tmpl["src_port"], tmpl["dst_port"] = 0x11, 4791, 4791
    tmpl_dev = torch.from_numpy(tmpl.view(np.uint8).copy()).to(dev)
    st = torch.cuda.Stream(device=dev)
    n_up = F * P
    out = torch.empty((n_up * (F + 1), stride), dtype=torch.uint8, device=dev)
    out_len = torch.empty(n_up * (F + 1), dtype=torch.int32, device=dev)
    action = torch.empty(n_up, dtype=torch.int32, device=dev)
    psn_out = torch.empty(n_up, dtype=torch.int32, device=dev)
    turn = [0]
    seen = {}

    def one(check=False):
        up, dn = rounds[turn[0] % 2]
        turn[0] += 1
        sw.batch(up, up_ports, tmpl_dev, stream=st.cuda_stream, out=out, out_len=out_len, action=action, psn=psn_out)
        if check:
            torch.cuda.synchronize()
            seen["up"] = action.cpu().numpy().copy(), out_len.cpu().numpy().reshape(n_up, F + 1).copy()
        sw.batch(dn, dn_ports, tmpl_dev, stream=st.cuda_stream, out=out[: P * (F + 1)], out_len=out_len[: P * (F + 1)],
                 action=action[:P], psn=psn_out[:P])
        if check:
            torch.cuda.synchronize()
            seen["dn"] = action[:P].cpu().numpy().copy(), out_len[: P * (F + 1)].cpu().numpy().reshape(P, F + 1).copy()

    one(check=True)
    a, ln = seen["up"]
    fwd = a == inccl.SW_FORWARD
    ok = int(fwd.sum()) == P and bool((a[~fwd] == inccl.SW_ABSORBED).all())
    ok = ok and bool((ln[fwd, F] > 0).all() and (ln[fwd, :F] == 0).all() and (ln[~fwd] == 0).all())
    a, ln = seen["dn"]
    ok = ok and bool((a == inccl.SW_DOWN).all() and (ln[:, :F] > 0).all() and (ln[:, F] == 0).all())
    ms = kernel_time_ms(one, st, iters)
    sw.destroy()
    frames = n_up + P
    return {"what": "non-root inccl_switch_batch x 2 per round: the children's frames up (FORWARD to the parent), "
                    "the parent's results down (DOWN to every child); INCCL_SW_RECYCLE",
            "fan_in": F, "psns": P, "frames": frames, "us_per_round": round(ms * 1e3, 2),
            "payload_GBs": round(frames * 1024 / (ms * 1e-3) / 1e9, 1), "frames_per_s": round(frames / (ms * 1e-3)),
            "every_psn_forwards_and_takes_its_result_once": ok, "timing": "HIP events on the batches' stream, eager calls"}


SIZES_BYTES = (4 << 10, 64 << 10, 1 << 20, 4 << 20, 64 << 20, 256 << 20, 1 << 30)


def host_us_per_call(fn, iters: int) -> float:
    """Host wall time per call of `fn` over `iters` back-to-back calls (one
    synchronisation at the end): what a caller of a stream-ordered API sees."""
    import torch
    for _ in range(max(3, iters // 10)):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def n1_sizes(dev, R: int, k: int, sizes=SIZES_BYTES) -> list:
    """north_star's bucket sizes at N = 1 (4/64/256/1024 MiB) and the small-bucket
    regime below them (4 KiB = one reference message, api.h:39; 64 KiB; 1 MiB):
    the fused kernel on R resident buckets of each size.  Per size:

      eager_us     inccl.reduce_f32 from Python, host time per call over
                   back-to-back calls: what a caller of the plain API sees
      prepared_us  the same bucket through a prepared op (inccl_op_run: the
                   arguments bound once, one ctypes argument per call)
      graph1_us    a hipGraph holding one call, replayed per call
      graph20_us   a hipGraph holding 20 calls, host time per call over its
                   back-to-back replays (as the N > 1 sweep's graph_us,
                   graph_replay_us): the launch cost a captured step pays
      kernel_us    a hipGraph holding `per` calls, per call: the device rate of
                   back-to-back kernels (HIP events on the replay stream)
      GBps_buckets R * bucket bytes / eager_us (the call); GBps_buckets_prepared
                   likewise; hbm_frac from kernel_us against 8 TB/s"""
    import torch

    from container_inc_amd import inccl
    rows = []
    st = torch.cuda.Stream(device=dev)
    for b in sizes:
        n = b // 4
        gen = torch.Generator(device=dev)
        gen.manual_seed(1000)
        xs = [torch.randn(n, generator=gen, device=dev) for _ in range(R)]
        out = torch.empty(n, device=dev)
        torch.cuda.synchronize()
        iters = int(max(20, min(3000, (8 << 30) // (b * R + b))))
        h = st.cuda_stream
        call = lambda: inccl.reduce_f32(xs, k, out=out, stream=h)  # noqa: E731
        eager = host_us_per_call(call, iters)
        op = inccl.prepare_reduce_f32(xs, k, out=out, stream=h)
        prepared = host_us_per_call(op, iters)
        op.destroy()
        per = max(10, min(100, iters // 4))
        res = {}
        for tag, cnt in (("g1", 1), ("g20", 20), ("dev", per)):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                for _ in range(cnt):
                    call()
            reps = max(4, iters // cnt)
            with torch.cuda.stream(st):   # replay() launches on the current stream
                g.replay()
                if tag != "dev":
                    res[tag] = host_us_per_call(g.replay, reps) / cnt
                else:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(reps):
                        g.replay()
                    e1.record(st)
                    torch.cuda.synchronize()
                    res[tag] = e0.elapsed_time(e1) * 1e3 / (reps * cnt)
            del g
        kernel_us = res["dev"]
        alg = (R + 1) * 4 * n
        rows.append({"bucket_bytes": b, "bucket_mib": round(b / (1 << 20), 6),
                     "eager_us": round(eager, 2), "prepared_us": round(prepared, 2),
                     "graph1_us": round(res["g1"], 2), "graph20_us": round(res["g20"], 2),
                     "kernel_us": round(kernel_us, 2),
                     "GBps_buckets": round(R * b / (eager * 1e-6) / 1e9, 1),
                     "GBps_buckets_prepared": round(R * b / (prepared * 1e-6) / 1e9, 1),
                     "GBps_buckets_kernel": round(R * b / (kernel_us * 1e-6) / 1e9, 1),
                     "hbm_GBps": round(alg / (kernel_us * 1e-6) / 1e9, 1),
                     "hbm_frac": round(alg / (kernel_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)})
        del xs, out
    torch.cuda.empty_cache()
    return rows


def cold_run(dev, R: int, k: int, n: int, sets: int = 4) -> dict:
    """The fused kernel rotating through `sets` independent input/output sets
    (sets * (R+1) * 4n bytes, far beyond the 256 MiB Infinity Cache), so no launch
    finds its inputs left on die by the previous one: an HBM figure by construction."""
    import torch

    from container_inc_amd import inccl
    st = torch.cuda.Stream(device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2000)
    groups = [([torch.randn(n, generator=gen, device=dev) for _ in range(R)], torch.empty(n, device=dev))
              for _ in range(sets)]
    torch.cuda.synchronize()
    it = [0]

    def one():
        xs, out = groups[it[0] % sets]
        it[0] += 1
        inccl.reduce_f32(xs, k, out=out, stream=st.cuda_stream)

    ms = kernel_time_ms(one, st, 40)
    alg = (R + 1) * 4 * n
    del groups
    torch.cuda.empty_cache()
    return {"sets": sets, "working_set_MiB": sets * alg >> 20, "kernel_us": round(ms * 1e3, 2),
            "achieved": round(alg / (ms * 1e-3) / 1e9, 1),
            "frac": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


def r_variants(dev, k: int, n: int, rs=(1, 8)) -> list:
    """BASELINE config 2's other local-bucket counts (R in {1, 2, 8}; R = 2 is the
    headline): the fused kernel on R resident 256 MiB buckets, repeated launches
    and, beside them, two rotated sets (2 x (R+1) x 256 MiB, beyond the Infinity
    Cache)."""
    import torch

    from container_inc_amd import inccl
    rows = []
    st = torch.cuda.Stream(device=dev)
    for R in rs:
        gen = torch.Generator(device=dev)
        gen.manual_seed(3000 + R)
        groups = [([torch.randn(n, generator=gen, device=dev) for _ in range(R)], torch.empty(n, device=dev))
                  for _ in range(2)]
        torch.cuda.synchronize()
        hot = kernel_time_ms(lambda: inccl.reduce_f32(groups[0][0], k, out=groups[0][1], stream=st.cuda_stream),
                             st, 40)
        it = [0]

        def rotated():
            xs, out = groups[it[0] % 2]
            it[0] += 1
            inccl.reduce_f32(xs, k, out=out, stream=st.cuda_stream)

        cold = kernel_time_ms(rotated, st, 40)
        alg = (R + 1) * 4 * n
        rows.append({"R": R, "bucket_mib": n * 4 >> 20, "kernel_us": round(hot * 1e3, 2),
                     "hbm_frac": round(alg / (hot * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                     "rotated_kernel_us": round(cold * 1e3, 2),
                     "rotated_hbm_frac": round(alg / (cold * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
        del groups
        torch.cuda.empty_cache()
    return rows


def bf16_buckets(dev, R: int, k: int, mib: int = 256, fmt: str = "bf16") -> dict:
    """bfloat16 (fmt "bf16") or float16 ("f16") gradient buckets (inccl_reduce_bf16 /
    _f16 = k_stream16<BF16,BF16,R> / <F16,F16,R>): R resident `mib` MiB buckets,
    repeated and rotated through two sets.  Algorithmic bytes (R + 1) * 2 * n.
    Parity: tests/test_gpu_bf16.py, tests/test_gpu_f16.py."""
    import torch

    from container_inc_amd import inccl
    dtype, reduce = {"bf16": (torch.bfloat16, inccl.reduce_bf16), "f16": (torch.float16, inccl.reduce_f16)}[fmt]
    n = mib * (1 << 20) // 2
    st = torch.cuda.Stream(device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4000)
    groups = [([torch.randn(n, generator=gen, device=dev).to(dtype) for _ in range(R)],
               torch.empty(n, device=dev, dtype=dtype)) for _ in range(2)]
    torch.cuda.synchronize()
    hot = kernel_time_ms(lambda: reduce(groups[0][0], k, out=groups[0][1], stream=st.cuda_stream), st, 40)
    it = [0]

    def rotated():
        xs, out = groups[it[0] % 2]
        it[0] += 1
        reduce(xs, k, out=out, stream=st.cuda_stream)

    cold = kernel_time_ms(rotated, st, 40)
    alg = (R + 1) * 2 * n
    del groups
    torch.cuda.empty_cache()
    return {"R": R, "bucket_mib": mib, "elems": n, "kernel_us": round(hot * 1e3, 2),
            "GBps_buckets": round(R * 2 * n / (hot * 1e-3) / 1e9, 1),
            "hbm_frac": round(alg / (hot * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "rotated_kernel_us": round(cold * 1e3, 2),
            "rotated_hbm_frac": round(alg / (cold * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


def api_allreduce_write(comm, mib: int = 256, calls: int = 7) -> dict:
    """The reference's own entry point, inccl_allreduce_write (api.h:99, api.c:403-452),
    on a `mib` MiB host int32 message at world 1: GB/s of one rank's message, with
    src/dst registered (inccl_host_register, the ibv_reg_mr of api.c:170-176: direct
    DMA) and unregistered (pinned staging).  Every call's dst is checked (at world 1
    the sum is the message itself)."""
    import numpy as np
    n = mib << 18
    rng = np.random.default_rng(9)
    src = rng.integers(-(2 ** 31), 2 ** 31 - 1, n, dtype=np.int64, endpoint=True).astype(np.int32)
    dst = np.empty_like(src)
    res = {"message_mib": mib, "world": 1}
    for mode in ("unregistered", "registered"):
        if mode == "registered":
            comm.host_register(src)
            comm.host_register(dst)
        for _ in range(2):   # first calls: staging / workspaces grow, DMA mappings warm up
            comm.allreduce_write(src, n, dst)
        ok = bool(np.array_equal(dst, src))
        times = []
        for _ in range(calls):
            dst[:1] = 0
            t0 = time.perf_counter()
            comm.allreduce_write(src, n, dst)
            times.append(time.perf_counter() - t0)
            ok = ok and bool(dst[0] == src[0])
        ok = ok and bool(np.array_equal(dst, src))
        dt = sorted(times)[len(times) // 2]   # median: single calls vary on a fresh box (tools/api_write_probe.py)
        res[mode] = {"ms": round(dt * 1e3, 3), "GBps": round(n * 4 / dt / 1e9, 2),
                     "best_GBps": round(n * 4 / min(times) / 1e9, 2), "calls": calls, "correct": ok}
        if mode == "registered":
            comm.host_deregister(src)
            comm.host_deregister(dst)
    res["reference_cpu_GBps_per_core"] = 0.27   # SURVEY.md §6, the reference's compiled path incl. framing/ICRC
    return res


def host_e2e(comm, k: int, gib: int = 1, bucket_mib: int = 64, world: int = 1) -> dict:
    """BASELINE config 3: a `gib` GiB fp32 gradient in pinned host memory through
    inccl_allreduce_f32_host (bucket_mib buckets, H2D / reduce / D2H on three
    streams).  PCIe-inclusive; reported beside `value`, never as it.  At N > 1
    every rank runs it (the reduce is the engine's allreduce across ranks); the
    time is the max over ranks."""
    import torch
    import torch.distributed as dist
    n = (gib << 30) // 4
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, generator=gen, dtype=torch.float32).pin_memory()
    y = torch.empty(n, dtype=torch.float32).pin_memory()
    comm.allreduce_f32_host(x, y, scale_exp=k, bucket_bytes=bucket_mib << 20)   # warm
    reps = 4
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        comm.allreduce_f32_host(x, y, scale_exp=k, bucket_bytes=bucket_mib << 20)
    dt = agree([(time.perf_counter() - t0) / reps], world)[0]
    # this box's PCIe ceiling on the same pinned buffers: H2D alone, D2H alone,
    # and both at once on two streams (what the pipeline overlaps).  The streams
    # have the greatest priority, as the pipeline's copy streams do (api.c
    # copy_streams_ensure): normal-priority ones can serialise the two directions, which
    # would make this "ceiling" lower than the pipeline itself.
    dev = torch.device("cuda", torch.cuda.current_device())
    m = (bucket_mib << 20) // 4
    d_in, d_out = torch.empty(m, device=dev), torch.empty(m, device=dev)
    try:
        prio = torch.cuda.Stream.priority_range()[1]
    except Exception:  # noqa: BLE001
        prio = -1
    s1, s2 = torch.cuda.Stream(device=dev, priority=prio), torch.cuda.Stream(device=dev, priority=prio)

    def copies(h2d: bool, d2h: bool) -> float:
        torch.cuda.synchronize()
        t = time.perf_counter()
        for off in range(0, n, m):
            if h2d:
                with torch.cuda.stream(s1):
                    d_in.copy_(x[off:off + m], non_blocking=True)
            if d2h:
                with torch.cuda.stream(s2):
                    y[off:off + m].copy_(d_out, non_blocking=True)
        torch.cuda.synchronize()
        return (gib << 30) / (time.perf_counter() - t) / 1e9

    copies(True, True)   # warm
    h2d, d2h, both = copies(True, False), copies(False, True), copies(True, True)
    del x, y, d_in, d_out
    return {"gradient_GiB": gib, "bucket_MiB": bucket_mib, "streams": 3, "ms": round(dt * 1e3, 2),
            "GBps": round((gib << 30) / dt / 1e9, 2),
            "pcie_GBps_both_directions": round(2 * (gib << 30) / dt / 1e9, 2),
            "copy_only_GBps": {"h2d": round(h2d, 2), "d2h": round(d2h, 2), "h2d_and_d2h_concurrent": round(both, 2),
                               "stream_priority": prio},
            "frac_of_concurrent_copy": round((gib << 30) / dt / 1e9 / both, 4),
            "what": "pinned host fp32 -> H2D -> fused quantise+sum+dequantise -> D2H, wall clock" if world == 1 else
                    f"pinned host fp32 on each of {world} ranks -> H2D -> the engine's allreduce -> D2H, wall clock, "
                    "max over ranks"}


def numerics_vs_exact(dev, n: int) -> list:
    """Error of the engine's result against the exact sum (fp64 of the fp32
    inputs) on config-2 data (N(0,1), seeds 1000+r), per (R, scale):
    max abs error, max relative error, and the fraction of lanes whose relative
    error exceeds north_star's 1e-6.  The engine is bit-exact vs its own spec
    (the oracle); this is the spec's distance from the true sum."""
    import torch

    from container_inc_amd import inccl
    rows = []
    for R in (2, 8):
        gen = torch.Generator(device=dev)
        xs = []
        for r in range(R):
            gen.manual_seed(1000 + r)
            xs.append(torch.randn(n, generator=gen, device=dev))
        exact = torch.zeros(n, dtype=torch.float64, device=dev)
        for x in xs:
            exact += x.double()
        fp32_naive = xs[0].clone()
        for x in xs[1:]:
            fp32_naive += x
        absx = exact.abs()
        nz = absx > 0
        for k in (25, "auto"):
            if k == "auto":
                word = torch.zeros(4, dtype=torch.int32, device=dev)
                out = inccl.reduce_f32_auto(xs, word=word)
                amax = float(word[:1].view(torch.float32).item())
                kk = inccl.choose_scale(amax, R)
            else:
                out = inccl.reduce_f32(xs, k)
                kk = k
            torch.cuda.synchronize()
            err = (out.double() - exact).abs()
            rel = torch.where(nz, err / absx.clamp_min(1e-300), torch.zeros_like(err))
            nerr = (fp32_naive.double() - exact).abs()
            nrel = torch.where(nz, nerr / absx.clamp_min(1e-300), torch.zeros_like(nerr))
            # the spec's own bound per lane: R quantisation errors of at most
            # 2^-(k+1) each, plus the fp32 rounding of the result (half an ulp)
            bound = R * 2.0 ** -(kk + 1) + out.double().abs() * 2.0 ** -24
            rows.append({"R": R, "scale_exp": kk, "auto": k == "auto", "lanes": n,
                         "max_abs_err": float(err.max().item()),
                         "quant_bound_abs": R * 2.0 ** -(kk + 1),
                         "lanes_beyond_spec_bound": int((err > bound * (1 + 1e-12)).sum().item()),
                         "max_rel_err": float(rel.max().item()),
                         "frac_rel_gt_1e-6": float((rel > 1e-6).double().mean().item()),
                         "frac_rel_gt_1e-6_fp32_naive_sum": float((nrel > 1e-6).double().mean().item())})
            del out, err, rel, nerr, nrel
        del xs, exact, fp32_naive, absx, nz
    torch.cuda.empty_cache()
    return rows


def load_traffic(workload: str):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3
    PMC summary (profiles/pmc_traffic.json) and the round it was recorded in,
    or (None, None)."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        d = json.load(open(path)).get(workload, {})
        return d.get("hbm_bytes_per_launch"), d.get("round")
    except Exception:
        return None, None


def main():
    a = parse()
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        # nothing has touched the GPU yet: the ranks are separate fresh processes
        sys.exit(self_launch(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        sys.exit(f"bench: WORLD_SIZE={world} but --gpus={a.gpus}: launch with --nproc-per-node equal to --gpus, "
                 "or omit WORLD_SIZE and let bench.py start the ranks")
    watchdog = Watchdog(float(os.environ.get("INCCL_BENCH_BUDGET", "480")), rank)
    if rank == 0:
        KEEPER[0] = LineKeeper()   # before anything touches the GPU

    import torch
    import torch.distributed as dist

    import container_inc_amd
    from container_inc_amd import inccl
    from container_inc_amd._lib import runtime_libs
    from container_inc_amd.plan import chunk_plan

    if os.environ.get("INCCL_BENCH_WATCHDOG"):   # debugging aid: dump every thread's stack when stuck
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["INCCL_BENCH_WATCHDOG"]), repeat=True)
    # rehearsal hook: every rank on device 0 (a one-GPU box running N>1 over the
    # p2p engine; RCCL refuses two ranks on one GPU).  Each rank then opens two
    # hardware queues, not HIP's default four (set before this process's first
    # HIP call): eight processes x four queues oversubscribe the GPU's queue
    # slots, and the scheduler time-slices the ranks -- the 8-rank rehearsal
    # step took 23.2 ms with four and 2.26 ms with two (DESIGN.md "Mesh
    # reduce-scatter route", liveness).  Never on the driver's one-process-per-
    # GPU runs.  ($INCCL_BENCH_REHEARSAL_HW_QUEUES: another count.)
    if os.environ.get("INCCL_BENCH_SAME_DEVICE") == "1":
        local_rank = 0
        if world > 1:
            os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("INCCL_BENCH_REHEARSAL_HW_QUEUES", "2")
    os.environ.setdefault("INCCL_BOOT_TIMEOUT", "120")
    # an ll / mesh candidate whose peer never arrives costs 2 s, not 5
    os.environ.setdefault("INCCL_LL_TIMEOUT_MS", "2000")
    if a.engine in ("p2p", "mesh", "meshw"):
        os.environ["INCCL_ENGINE"] = a.engine   # no eager RCCL communicator
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    container_inc_amd.load()
    if a.grid_cap:
        inccl.set_tuning(a.grid_cap, True)

    R, k = a.local_buckets, a.scale_exp
    n = a.bucket_mib * (1 << 20) // 4
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + rank)
    srcs = [torch.randn(n, generator=gen, device=dev, dtype=torch.float32) for _ in range(R)]
    out = torch.empty(n, device=dev, dtype=torch.float32)
    torch.cuda.synchronize()   # inputs made on torch's stream; the library runs on its own

    master = os.environ.get("MASTER_ADDR", "127.0.0.1")
    port = int(os.environ.get("MASTER_PORT", "29500")) + 17
    grp = inccl.inccl_group_create(world, rank, master, port=port, device=local_rank)
    if grp is None:
        raise SystemExit("inccl_group_create failed: " + container_inc_amd.load().inccl_last_error().decode())
    comm = inccl.inccl_communicator_create(grp, 0)
    stream = torch.cuda.Stream(device=dev)

    def barrier():
        if world > 1:
            dist.barrier()

    # N>1: pick the exchange engine / chunking during warmup (untimed).  Every
    # candidate runs alternating input sets A, B, A and must reproduce the
    # reference engine's results bit for bit (integer sums are exact) and the
    # oracle on a lane sample; any failure or mismatch on any rank drops that
    # candidate on all ranks.  The first candidate that passes on every rank is
    # the reference.
    #
    # Two phases, so that an engine never run across separate GPUs cannot cost
    # the line: phase 1 tunes the RCCL collectives (rccl, ar, a2a) and measures
    # a complete, verified headline with the fastest; only then does phase 2
    # tune this library's IPC engines (p2p, mesh, meshw).  A phase-2 engine that
    # faults or hangs leaves the phase-1 headline to the line keeper / watchdog.
    # If a phase-2 engine tunes faster, it is measured the same way and the
    # faster of the two measured headlines is the line (both are reported).
    tuning = []
    refs = [None]
    phases = [[]]
    srcs_b = None
    if world > 1:
        gen_b = torch.Generator(device=dev)
        gen_b.manual_seed(5000 + rank)
        srcs_b = [torch.randn(n, generator=gen_b, device=dev, dtype=torch.float32) for _ in range(R)]
        torch.cuda.synchronize()
        cands = []
        if a.engine in ("auto", "rccl"):
            cands += [("rccl", c, {}) for c in ([a.chunks] if a.chunks else [1, 4])]
        if a.engine in ("auto", "ar"):
            cands.append(("ar", 1, {}))
        if a.engine in ("auto", "a2a"):
            cands.append(("a2a", 1, {}))
        if a.engine in ("auto", "p2p"):
            cands.append(("p2p", 1, {}))
        for eng in ("mesh", "meshw"):
            if a.engine in ("auto", eng):
                cands += [(eng, 1, {}), (eng, 1, {"INCCL_MESH_LAG": "32"})]
        # rehearsal hook: which engines count as phase 1 (one-GPU rehearsals have no RCCL)
        safe = set((os.environ.get("INCCL_BENCH_SAFE_ENGINES") or "rccl,ar,a2a").split(","))
        phases = [[c for c in cands if c[0] in safe], [c for c in cands if c[0] not in safe]]
        tune_lanes = oracle_lanes(n, world, max(ch for _, ch, _ in cands), 1 << 16)

    def tune(cand_list, phase: int):
        """Warmup-time candidates of one phase: verified, then timed over
        TUNE_CALLS calls; returns (ms, engine, chunks, env) of the fastest."""
        best = None
        for eng, ch, env in cand_list:
            set_stage(f"engine tuning (phase {phase}): {eng} chunks={ch} {env or ''}")
            ok, dt, same, got, err = 1, float("inf"), False, None, None
            os.environ.update(env)
            try:
                comm.set_engine(eng)
                got, same = run_verified(comm, eng, ch, (srcs, srcs_b), out, k, stream, refs[0])
                for _ in range(TUNE_CALLS // 2):   # untimed: buffers just (re)allocated for this engine
                    comm.allreduce_f32(srcs, out=out, scale_exp=k, chunks=ch, stream=stream.cuda_stream)
                torch.cuda.synchronize()
                barrier()
                t0 = time.perf_counter()
                for _ in range(TUNE_CALLS):
                    comm.allreduce_f32(srcs, out=out, scale_exp=k, chunks=ch, stream=stream.cuda_stream)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / TUNE_CALLS
            except Exception as e:  # noqa: BLE001
                print(f"rank {rank}: engine {eng} chunks {ch} {env} failed: {e}", file=sys.stderr, flush=True)
                ok, err = 0, str(e)[:400]
            stages = None
            if a.full and agree([0.0 if ok else 1.0], world)[0] == 0.0:   # every rank probes, or none does
                try:
                    stages = stage_probe(comm, srcs, out, k, ch, stream, world)
                except Exception as e:  # noqa: BLE001
                    stages = {"error": str(e)[:200]}
            for key in env:
                os.environ.pop(key, None)
            v = agree([dt if ok else float("inf"), 0.0 if ok else 1.0, 0.0 if same else 1.0], world)
            good = v[1] == 0.0 and v[2] == 0.0
            par = None
            if v[1] == 0.0:
                # the candidate's result on input set A against the oracle: an
                # engine that is only self-consistent never becomes the reference
                par = oracle_check(srcs, got[0], tune_lanes, k, rank, world)
                good = good and agree([float(par["mismatches"] or 0) if rank == 0 else 0.0], world)[0] == 0.0
            if good and refs[0] is None:
                refs[0] = (got[0], got[1])
            if rank == 0:
                print(f"tune {eng} chunks={ch} {env or ''}: ok={v[1] == 0.0} identical={v[2] == 0.0} "
                      f"oracle_mismatches={par and par['mismatches']} ms={v[0] * 1e3:.3f}", file=sys.stderr,
                      flush=True)
            tuning.append({"engine": eng, "chunks": ch, "env": env or None, "phase": phase, "ok": v[1] == 0.0,
                           "bit_identical": v[1] == 0.0 and v[2] == 0.0, "verified": good,
                           "oracle_mismatches": par["mismatches"] if par else None,
                           "ms": round(v[0] * 1e3, 3) if v[1] == 0.0 else None,
                           "stages_us": stages,
                           # rank 0's error text (RCCL's own reason, ncclGetLastError, included)
                           **({"error": err} if err else {})})
            if good and (best is None or v[0] < best[0]):
                best = (v[0], eng, ch, env)
            del got
        return best

    def measure(eng: str, ch: int, env: dict) -> dict:
        """The headline measurement of one engine: settle, W warmup steps, K
        timed steps between barriers (max over ranks), the timed output and four
        alternating calls against the reference engine, and the oracle check."""
        if world > 1:
            comm.set_engine(eng)
        os.environ.update(env)

        def step():
            comm.allreduce_f32(srcs, out=out, scale_exp=k, chunks=ch, stream=stream.cuda_stream)

        # settle: untimed steps in groups of 10 until --settle-seconds have passed
        # (the same count on every rank), so that the timed steps see steady state
        # rather than the first passes over freshly allocated buckets
        set_stage(f"settle/warmup/timed steps of engine {eng if world > 1 else 'fused'}")
        settle_steps, t_settle = 0, time.perf_counter()
        while True:
            for _ in range(10):
                step()
            settle_steps += 10
            torch.cuda.synchronize()
            if agree([1.0 if time.perf_counter() - t_settle >= a.settle_seconds else 0.0], world)[0] > 0.0:
                break
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()

        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(a.steps):
            step()
        ev1.record(stream)
        torch.cuda.synchronize()
        barrier()
        wall = time.perf_counter() - t0
        dev_ms = ev0.elapsed_time(ev1)
        wall = agree([wall], world)[0]
        # --dump-outputs: what the last timed step left in `out` (every rank
        # holds the same allreduce result; rank 0 writes it), taken before
        # anything below runs another step
        dump = None
        if a.dump_outputs and rank == 0:
            sel = dump_lanes(n)
            dump = (out if sel is None else out.index_select(0, torch.from_numpy(sel).to(dev))).cpu().numpy()
        if not a.full:   # the headline alone: no verification, parity or stage runs
            for key in env:
                os.environ.pop(key, None)
            return {"engine": eng if world > 1 else "fused", "chunks": ch, "env": env,
                    "ms_per_step": wall * 1e3 / a.steps, "settle_steps": settle_steps, "dev_ms": dev_ms,
                    "verified": None, "parity": None, "stages": None, "dump": dump}
        # the timed steps' output against the reference engine's (N>1): the last
        # timed step's output, then four more steps alternating the two input
        # sets, each against the reference engine's results
        verified = None
        if refs[0] is not None:
            set_stage(f"verification of the timed engine {eng}")
            bad = 0 if torch.equal(out, refs[0][0]) else 1
            for i in range(4):
                comm.allreduce_f32(srcs_b if i % 2 == 0 else srcs, out=out, scale_exp=k, chunks=ch,
                                   stream=stream.cuda_stream)
                torch.cuda.synchronize()
                bad += 0 if torch.equal(out, refs[0][(i + 1) % 2]) else 1
            verified = agree([float(bad)], world)[0] == 0.0
        # the timed path's result against the oracle on a lane sample: 2^20
        # strided lanes plus both sides of every shard / chunk boundary, every
        # rank's inputs gathered to rank 0 (one more step first: `out` then holds
        # srcs' result)
        set_stage(f"oracle parity check of the timed engine {eng if world > 1 else 'fused'}")
        step()
        torch.cuda.synchronize()
        parity = oracle_check(srcs, out, oracle_lanes(n, world, ch, 1 << 20), k, rank, world)
        stages = None
        if world > 1:   # after the timed steps: where a step's time goes, per stage
            set_stage(f"stage timing of the timed engine {eng}")
            stages = stage_probe(comm, srcs, out, k, ch, stream, world)
        for key in env:
            os.environ.pop(key, None)
        return {"engine": eng if world > 1 else "fused", "chunks": ch, "env": env, "ms_per_step": wall * 1e3 / a.steps,
                "settle_steps": settle_steps, "dev_ms": dev_ms, "verified": verified, "parity": parity,
                "stages": stages, "dump": dump}

    # dominant kernel alone: fused (N=1) or quant + local sum (N>1), HIP events
    # on its stream; timed once, right after the first headline measurement
    kinfo = {}

    def dominant_kernel():
        set_stage("dominant-kernel timing")
        kstream = torch.cuda.Stream(device=dev)
        qbuf = torch.empty(n, device=dev, dtype=torch.int32) if world > 1 else None

        def kernel():
            if world == 1:
                inccl.reduce_f32(srcs, k, out=out, stream=kstream.cuda_stream)
            else:
                inccl.quant_sum(srcs, k, out=qbuf, stream=kstream.cuda_stream)

        k_ms = kernel_time_ms(kernel, kstream, max(a.steps, 20))
        del qbuf
        alg_bytes = (R + 1) * 4 * n
        achieved = alg_bytes / (k_ms * 1e-3) / 1e9
        kname = "k_stream_vec<F32,F32,R>" if world == 1 else "k_stream_vec<F32,Q32,R>"
        traffic, traffic_round = load_traffic(kname + f" R={R} n={n}")
        hbm = {
            "kernel": kname,
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": traffic,
            "traffic_source": ("profiles/pmc_traffic.json: separate rocprofv3 --pmc FETCH_SIZE (x2, gfx950) and "
                               f"WRITE_SIZE passes over this kernel and size, recorded in round {traffic_round} "
                               "(not re-measured in this run)")
            if traffic is not None else None,
            "alg_bytes_per_launch": alg_bytes,
            "kernel_ms": round(k_ms, 5),
        }
        if world == 1:
            # the same kernel rotating through 4 input/output sets (3 GiB, far past
            # the 256 MiB Infinity Cache): `frac` re-reads the same buffers every
            # launch, `frac_cold` cannot find them on die
            set_stage("cold (rotated-set) kernel timing")
            cold = cold_run(dev, R, k, n)
            hbm["frac_cold"] = cold["frac"]
            hbm["achieved_cold"] = cold["achieved"]
            hbm["kernel_ms_cold"] = round(cold["kernel_us"] * 1e-3, 5)
            kinfo["cold"] = cold
        kinfo["hbm"] = hbm

    per_rank = f"R={R} resident {a.bucket_mib} MiB fp32 buckets per rank: "

    def build_res(m: dict) -> dict:
        """The JSON line of one headline measurement."""
        ms_per_step, chunks = m["ms_per_step"], m["chunks"]
        workload = (f"fused quantise+sum+dequantise of R={R} resident {a.bucket_mib} MiB fp32 buckets, 1 GPU"
                    if world == 1 else per_rank + {
                        "rccl": f"quant+local sum -> RCCL reduce-scatter int32 -> dequant shard -> RCCL all-gather "
                                f"fp32, {chunks} pipelined chunks",
                        "ar": "quant+local sum -> RCCL all-reduce int32 in place -> dequant",
                        "a2a": "quant+local sum -> RCCL all-to-all of int32 shards -> fused sum+dequant (HIP) -> RCCL "
                               "all-gather fp32",
                        "p2p": "quant+local sum -> p2p pull of every peer's shard over xGMI with fused sum+dequant -> "
                               "p2p gather of every result shard",
                        "mesh": "one persistent HIP kernel: per-chunk quant+local sum pushed into the owner's inbox "
                                "over xGMI -> owner's sum+dequant on arrival flags -> pull of every result chunk",
                        "meshw": "one persistent HIP kernel: per-chunk quant+local sum pushed into the owner's inbox "
                                 "over xGMI -> owner's sum+dequant on arrival flags, result chunk pushed into every "
                                 "rank's inbox (all xGMI transfers are writes) -> local copy into dst",
                    }.get(m["engine"], m["engine"]))
        value = world * R * n * 4 / (ms_per_step * 1e-3) / 1e9
        res = {
            "metric": METRIC,
            "value": round(value, 2),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "settle_steps": m["settle_steps"],
            "device_ms_per_step_rank0": round(m["dev_ms"] / a.steps, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int32",
            "data": "synthetic N(0,1) fp32 buckets, torch.Generator seed 1000+rank",
            "config": {
                "workload": workload,
                "bucket_mib": a.bucket_mib,
                "local_buckets": R,
                "scale_exp": k,
                "numerics": f"fp32 in/out; quantised to int32 fixed point 2^-{k}; int32 wrap-around sum (exact)",
                "parallelism": f"dp{world}",
                "chunks": chunks,
                "engine": m["engine"],
                "engine_env": (m["env"] or None) if world > 1 else None,
                "same_device_rehearsal": ({"GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES")}
                                          if os.environ.get("INCCL_BENCH_SAME_DEVICE") == "1" and world > 1 else None),
                "engine_tuning": tuning or None,
                "shard_elems": chunk_plan(n, world, chunks)[0][2] if world > 1 else n,
            },
            # N = 1: the fused kernel's HBM roofline.  N > 1: the step is bound by
            # the xGMI links, so `roofline` is the link fraction of the whole step
            # and the dominant HBM kernel's figure moves to `roofline_hbm_kernel`.
            "roofline": kinfo.get("hbm") if world == 1 else xgmi_roofline(world, n * 4, ms_per_step * 1e-3),
            "cpu_baseline": None,
            "parity_vs_oracle": m["parity"],
            # the HIP / HSA / RCCL copies this rank is bound to (DESIGN.md "Runtimes")
            "runtime": runtime_libs(),
        }
        res["full"] = a.full
        if not a.full:
            # a plain run measures the headline alone: the keys that take runs
            # or checks of their own (--full) are not in its line
            for key in ("roofline", "cpu_baseline", "parity_vs_oracle"):
                del res[key]
            return res
        if world == 1:
            res["roofline_cold"] = kinfo["cold"]
        if world > 1:
            res["roofline_hbm_kernel"] = kinfo["hbm"]
            # per-stage microseconds of one step of the headline engine (HIP events
            # around each stage, untimed calls after the timed ones; stage_probe)
            res["stages_us"] = m["stages"]
            res["verified_vs_reference_engine"] = m["verified"]
            # nccl-tests convention (BASELINE config 4): algbw = one rank's bucket
            # bytes / step time; busbw = algbw * 2(W-1)/W, the per-GPU link traffic
            # of RS + AG
            algbw = n * 4 / (ms_per_step * 1e-3) / 1e9
            res["collective"] = {"algbw_GBps": round(algbw, 2),
                                 "busbw_GBps": round(algbw * 2 * (world - 1) / world, 2), "bytes_per_rank": n * 4}
        return res

    # The one JSON line, printed once: by the main thread at the end, or by the
    # watchdog (with the stage it was stuck in, exit code 3) if the run overruns
    # its budget, or by the line keeper if rank 0 dies -- from the first headline
    # measurement on, that line carries a measured headline (RESULT[0]).
    emit_lock, emitted = threading.Lock(), [False]

    def emit():
        with emit_lock:
            if emitted[0]:
                return False
            emitted[0] = True
        res = RESULT[0]
        res["elapsed_s"] = round(time.monotonic() - T_START, 1)
        if rank == 0:
            line = json.dumps(dict(res))   # a snapshot: the watchdog may emit while the main thread works
            print(line, flush=True)
            if KEEPER[0] is not None:
                KEEPER[0].update(printed=True)
            if a.json_out:
                with open(a.json_out, "w") as f:
                    f.write(line + "\n")
        return True

    def on_overrun(msg):
        RESULT[0]["error"] = msg + "; headline measured and kept, later keys partial"
        emit()

    def publish(res: dict, stage: str) -> None:
        """From now on every way the run can end prints `res`."""
        res["phase_s"] = PHASES
        if a.full and world > 1 and not a.no_sweep:
            res["sweep"] = SWEEP_ROWS
        RESULT[0] = res
        watchdog.on_fire = on_overrun
        set_stage(stage)

    measured = []   # (measurement, line) per headline measurement, in order
    PHASES["startup"] = round(time.monotonic() - T_START, 1)
    # time budgets from process start (agreed over ranks): the size sweeps start
    # no size -- and no engine of a size -- past sweep_soft, so that the bf16,
    # f16, reduce_scatter and host_e2e keys, which start until extra_soft, are
    # reached inside the watchdog's budget (INCCL_BENCH_BUDGET, 480 s) even when
    # every call is slow (the one-GPU N-rank rehearsal)
    sweep_soft = float(os.environ.get("INCCL_BENCH_SWEEP_SOFT", "180"))
    extra_soft = float(os.environ.get("INCCL_BENCH_EXTRA_SOFT", "400"))
    sweep_refs = {}   # bucket bytes -> the sweep's reference engine (pass 1), for pass 2

    def sweep_pass(name, want):
        """One pass of the size sweep; an exception (the same on every rank:
        the collectives are symmetric) is recorded in the line instead of
        costing the headline."""
        with Phase(name):
            try:
                size_sweep(comm, dev, R, k, rank, world, sweep_soft, SWEEP_ROWS, want=want, ref_of=sweep_refs)
            except Exception as e:  # noqa: BLE001
                print(f"rank {rank}: {name} failed: {e!r}", file=sys.stderr, flush=True)
                RESULT[0][name + "_error"] = repr(e)

    if world == 1:
        with Phase("headline"):
            m = measure("fused", 1, {})
            if a.full:
                dominant_kernel()
        measured.append((m, build_res(m)))
        publish(measured[-1][1], "headline measured")
    else:
        # Order, for a first run on a real node: the RCCL headline, then the
        # RCCL rows of the size sweep, and only then this library's IPC
        # engines (tuning, a possible faster headline, their sweep rows), bf16
        # and host_e2e -- whatever hangs or overruns later leaves the RCCL
        # headline and sweep in the line (watchdog / line keeper)
        with Phase("tune_rccl"):
            best1 = tune(phases[0], 1)
        if best1 is not None:
            with Phase("headline_rccl"):
                m = measure(best1[1], best1[2], best1[3])
                if a.full:
                    dominant_kernel()
            measured.append((m, build_res(m)))
            publish(measured[-1][1], f"headline measured on {m['engine']}; RCCL sweep next")
            if a.full and not a.no_sweep:
                for key in best1[3]:   # the sweep runs every engine with its defaults
                    os.environ.pop(key, None)
                sweep_pass("sweep_rccl", lambda eng: eng == "rccl")
        if os.environ.get("INCCL_BENCH_TEST_DIE") == "phase2" and rank == 0:   # test hook: rank 0 dies in phase 2
            import signal
            os.kill(os.getpid(), signal.SIGKILL)
        with Phase("tune_ipc"):
            best2 = tune(phases[1], 2)
        phase2_error = None
        if best2 is not None and (best1 is None or best2[0] < best1[0]):
            try:
                with Phase("headline_ipc"):
                    m = measure(best2[1], best2[2], best2[3])
            except Exception as e:  # noqa: BLE001 -- an engine error is the same on every rank
                if not measured:
                    raise
                phase2_error = f"{best2[1]}: {e!r}"
                print(f"rank {rank}: phase-2 headline on {phase2_error} failed; phase 1's stands", file=sys.stderr,
                      flush=True)
                for key in best2[3]:
                    os.environ.pop(key, None)
            else:
                if a.full and not kinfo:
                    dominant_kernel()
                line = build_res(m)
                # a phase-2 headline replaces phase 1's only if it was verified like it
                ok = m["verified"] is not False and ((m["parity"] or {}).get("mismatches") or 0) == 0
                if agree([0.0 if ok else 1.0], world)[0] == 0.0:
                    measured.append((m, line))
        if not measured:
            raise SystemExit("no exchange engine produced verified results on every rank")
        # the faster measured headline is the line; every measured one is listed
        best = min(measured, key=lambda x: x[0]["ms_per_step"])
        best[1]["config"]["engine_tuning"] = tuning or None
        best[1]["headline_candidates"] = [
            {"engine": mm["engine"], "chunks": mm["chunks"], "env": mm["env"] or None,
             "ms_per_step": round(mm["ms_per_step"], 4), "value": ln["value"],
             "verified_vs_reference_engine": mm["verified"],
             "oracle_mismatches": (mm["parity"] or {}).get("mismatches")}
            for mm, ln in measured]
        if phase2_error:
            best[1]["phase2_error"] = phase2_error
        for key in ("sweep_rccl_error",):   # carried over from the phase-1 line
            if key in measured[0][1] and key not in best[1]:
                best[1][key] = measured[0][1][key]
        publish(best[1], "headline measured")
        comm.set_engine(best[0]["engine"])
        os.environ.update(best[0]["env"])
    res = RESULT[0]
    chosen = ("fused", 1, {}) if world == 1 else (best[0]["engine"], best[0]["chunks"], dict(best[0]["env"]))
    if a.dump_outputs and rank == 0:
        # the headline measurement's last timed step, as its caller received it
        set_stage("writing --dump-outputs")
        with Phase("dump_outputs"):
            write_outputs(a.dump_outputs, {"out": (measured[0] if world == 1 else best)[0]["dump"]})
        set_stage("headline measured")
    if os.environ.get("INCCL_BENCH_TEST_DIE") == "1" and rank == 0:   # test hook: rank 0 dies after the headline
        import signal
        os.kill(os.getpid(), signal.SIGKILL)
    if a.full and world > 1 and not a.no_sweep:
        for key in chosen[2]:   # the sweep runs every engine with its defaults
            os.environ.pop(key, None)
        # The rest of the sweep and the bf16 key drive engines never before run
        # across separate GPUs; a size is only started while the run is inside
        # the soft budget, and a collective that hangs is ended by the watchdog
        # (headline line + partial sweep, rc 3).
        if os.environ.get("INCCL_BENCH_TEST_HANG") == "1" and rank == 0:   # test hook: a stuck rank 0
            set_stage("INCCL_BENCH_TEST_HANG sleep on rank 0")
            time.sleep(1e9)
        sweep_pass("sweep_other", lambda eng: eng != "rccl")
        with Phase("bf16"):
            if agree([time.monotonic() - T_START], world)[0] <= extra_soft:
                try:
                    res["bf16"] = bf16_engines(comm, dev, R, rank, world)
                except Exception as e:  # noqa: BLE001
                    print(f"rank {rank}: bf16 key failed: {e!r}", file=sys.stderr, flush=True)
                    res["bf16"] = {"error": repr(e)}
            else:
                res["bf16"] = {"skipped": f"run past {extra_soft:.0f} s from process start"}
        with Phase("f16"):
            if agree([time.monotonic() - T_START], world)[0] <= extra_soft:
                try:
                    res["f16"] = bf16_engines(comm, dev, R, rank, world, fmt="f16")
                except Exception as e:  # noqa: BLE001
                    print(f"rank {rank}: f16 key failed: {e!r}", file=sys.stderr, flush=True)
                    res["f16"] = {"error": repr(e)}
            else:
                res["f16"] = {"skipped": f"run past {extra_soft:.0f} s from process start"}
        with Phase("reduce_scatter"):
            if agree([time.monotonic() - T_START], world)[0] <= extra_soft:
                try:
                    # the mesh engine's row is its persistent kernel's own route (default on)
                    res["reduce_scatter"] = reduce_scatter_engines(comm, dev, R, rank, world,
                                                                   engines=("rccl", "p2p", "mesh"))
                    for small in (1 / 16, 1.0):   # 64 KiB and 1 MiB buckets: the ll engine's one kernel too
                        res["reduce_scatter"] += reduce_scatter_engines(comm, dev, R, rank, world, small,
                                                                        ("rccl", "p2p", "ll"))
                except Exception as e:  # noqa: BLE001
                    print(f"rank {rank}: reduce_scatter key failed: {e!r}", file=sys.stderr, flush=True)
                    res["reduce_scatter"] = {"error": repr(e)}
            else:
                res["reduce_scatter"] = {"skipped": f"run past {extra_soft:.0f} s from process start"}
        comm.set_engine(chosen[0])
        # north_star: the path starts and ends in host memory -- the end-to-end
        # rate with pinned H2D / D2H, at this N too
        with Phase("host_e2e"):
            if agree([time.monotonic() - T_START], world)[0] <= extra_soft:
                set_stage("host_e2e at N > 1")
                try:
                    res["host_e2e"] = host_e2e(comm, k, world=world)
                except Exception as e:  # noqa: BLE001
                    print(f"rank {rank}: host_e2e failed: {e!r}", file=sys.stderr, flush=True)
                    res["host_e2e"] = {"error": repr(e)}
            else:
                res["host_e2e"] = {"skipped": f"run past {extra_soft:.0f} s from process start"}
    def extra(key, fn):
        """An N = 1 extra key (one process, no collectives): a failure is recorded
        in the key instead of costing the headline line."""
        set_stage(f"extra key {key}")
        with Phase(key):
            try:
                res[key] = fn()
            except Exception as e:  # noqa: BLE001
                print(f"bench: extra key {key} failed: {e!r}", file=sys.stderr, flush=True)
                res[key] = {"error": repr(e)}

    if a.full and world == 1 and not a.no_extras:
        extra("host_e2e", lambda: host_e2e(comm, k))
        extra("api_allreduce_write", lambda: api_allreduce_write(comm))
        extra("sizes", lambda: n1_sizes(dev, R, k))
        extra("r_variants", lambda: r_variants(dev, k, n))
        extra("numerics_vs_exact", lambda: numerics_vs_exact(dev, n))
        extra("bf16", lambda: bf16_buckets(dev, R, k))
        extra("f16", lambda: bf16_buckets(dev, R, k, fmt="f16"))
        extra("switch_batch", lambda: switch_batch(dev))
        extra("switch_batch_acks", lambda: switch_batch(dev, acks=True))
        extra("switch_nonroot_round", lambda: switch_nonroot_round(dev))
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        extra("cpu_baseline", lambda: cpu_baseline(n, R, k, a.cpu_seconds))
        extra("cpu_baseline_allcores", lambda: cpu_baseline_allcores(n, R, k, min(a.cpu_seconds, 5.0)))
        extra("cpu_reference_pipeline", lambda: cpu_reference_pipeline(min(a.cpu_seconds, 5.0)))
    emit()
    watchdog.cancel()
    set_stage("teardown")
    comm.destroy()
    grp.destroy()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--line-keeper":
        line_keeper_main(sys.argv[2])
    else:
        main()
