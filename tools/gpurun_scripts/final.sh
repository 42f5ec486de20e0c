#!/bin/bash
# Round-end validation on one MI355X: GPU suite, contract bench (plain and --full), smoke, one-rank RCCL bench, rocprofv3 kernel trace of the bench.
#   usage: final.sh OUT_DIR      -> OUT_DIR/*
# Every GPU step runs under a time limit of its own, and the first one that fails ends the script: nothing more is started on that GPU.
R=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "${1:?usage: final.sh OUT_DIR}" && OUT=$(cd "$1" && pwd) || exit 2
cd "$R" || exit 2
rm -f "$OUT/tolerances.txt"
step() { timeout -k 10 "$@" || { echo "final.sh: \`$*\` ended with $?: stopping here" >&2; exit 1; }; }
WF_TOL_LOG=$OUT/tolerances.txt step 2400 python -m pytest tests -m gpu -q -x > "$OUT/pytest_gpu_full.log" 2>&1
grep -E "passed|failed|rror|^FAILED|^tests/" "$OUT/pytest_gpu_full.log" | tail -12 > "$OUT/pytest_gpu.log"
step 300 python bench.py --gpus 1 --steps 20 --warmup 5 > "$OUT/bench_plain.json" 2> "$OUT/bench_plain.err"   # the driver's own command: the headline window alone
step 600 python bench.py --gpus 1 --steps 20 --warmup 5 --full > "$OUT/bench.json" 2> "$OUT/bench.err"   # ... with cpu_baseline, the `also` windows of configs 3 / 4, the box calibration
step 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
WF_FORCE_COMM=1 RANK=0 LOCAL_RANK=0 WORLD_SIZE=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29517 step 300 python bench.py --gpus 1 > "$OUT/bench_rccl1.json" 2> "$OUT/bench_rccl1.err"
cd /tmp && export TMPDIR=/tmp
step 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -- python3 "$R/bench.py" > "$OUT/bench_prof.json" 2> "$OUT/bench_prof.err"
cd "$R"
find "$OUT/prof" -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} "$OUT/kernel_stats.csv"
rm -rf "$OUT/prof"
tail -3 "$OUT/pytest_gpu.log"; head -c 700 "$OUT/bench.json"; echo; tail -2 "$OUT/smoke.log"; head -c 300 "$OUT/bench_rccl1.json"
