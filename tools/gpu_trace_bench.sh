#!/bin/bash
# the driver's N=1 bench command (with --full: this script reads the roofline keys), then a plain
# run under rocprofv3 --kernel-trace with per-launch analysis.  Output: $INCCL_OUT_DIR (bench_out/).
cd "$GRAFT_REPO_ROOT" || exit 3
export O=${INCCL_OUT_DIR:-bench_out}
mkdir -p "$O"
export TMPDIR=/tmp
timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline --json-out "$O/bench_driverflags.json" > "$O/bench_driverflags.log" 2>&1 || { tail "$O/bench_driverflags.log"; exit 4; }
python3 -c "import json, os; d=json.load(open(os.environ['O'] + '/bench_driverflags.json')); print('driver flags:', d['value'], d['ms_per_step'], d['settle_steps'], d['roofline']['kernel_ms'], d['roofline']['frac'], d['roofline_cold']['frac'])"
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$O/trace" -o run -- python3 bench.py --steps 50 --warmup 10 --json-out "$O/bench_traced.json" > "$O/trace.log" 2>&1 || { tail "$O/trace.log"; exit 5; }
python3 - <<'P'
import csv, json, os
O = os.environ["O"]
rows = [r for r in csv.DictReader(open(O + "/trace/run_kernel_trace.csv")) if "k_stream_vec" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
print("launches", len(rows))
print(" ".join(f"{x:.0f}" for x in d))
b = json.load(open(O + "/bench_traced.json"))
s = b["settle_steps"]
timed = d[s + 10: s + 60]
print("timed steps: mean", round(sum(timed) / len(timed), 2), "bench ms_per_step", b["ms_per_step"])
P
