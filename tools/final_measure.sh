#!/bin/bash
# Round-end measurement on the GPU box: default bench line, task times (fp32 / bf16 mode), Cylinder, the 20-step rollout,
# Sod, and the per-configuration rocprofv3 passes (tools/profile_round.sh).  Outputs under <outdir>; copy what is to be
# judged into profiles/ (tools/make_pmc_json.py for the traffic JSON).
#   tools/final_measure.sh <outdir>
OUT=$(mkdir -p "${1:?usage: tools/final_measure.sh <outdir>}" && cd "$1" && pwd)
python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err"
bash tools/task_times.sh > "$OUT/task_times.txt" 2>&1
python bench.py --task cylinder --batch 200 --no-extras --no-cpu-baseline --steps 30 --warmup 5 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.read()); print('cylinder b=200 fp32', d['ms_per_step'], 'ms', d['value'], 'samples/s')" >> "$OUT/task_times.txt"
python bench.py --task vorticity --batch 20 --rollout 20 --no-extras --no-cpu-baseline --steps 10 --warmup 2 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.read()); print('vorticity rollout-20 b=20 fp32', d['ms_per_step'], 'ms/optimiser step', d.get('peak_memory_GB'), 'GB peak')" >> "$OUT/task_times.txt"
python bench.py --task sod --batch 8 --no-extras --no-cpu-baseline --steps 200 --warmup 20 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.read()); print('sod b=8 fp32', d['ms_per_step'], 'ms')" >> "$OUT/task_times.txt"
# (per-configuration rocprofv3 passes: run tools/profile_round.sh <outdir> separately)
cat "$OUT/task_times.txt"; tail -c 1500 "$OUT/bench_default.json"
