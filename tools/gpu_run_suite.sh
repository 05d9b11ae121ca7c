#!/bin/bash
# full GPU suite + bench --full in a given mode:  bash tools/gpu_run_suite.sh [mma] [tag]   (logs under $OUT_DIR, default out/)
MMA=${1:-bf16x3}; TAG=${2:-x}
O=${OUT_DIR:-out}; mkdir -p "$O"
timeout 900 python -m pytest tests -m gpu -q 2>&1 | grep -E "passed|failed|Error|mismatch|gradient" | cut -c1-2500 | tee "$O/tests_$TAG.log"
timeout 120 python tools/bench_gemm.py --mma $MMA 2>&1 | tail -1
timeout 600 python bench.py --full --steps 5 --warmup 2 --mma $MMA --cpu-sample-frames 2 2>&1 | tail -1 | tee "$O/bench_$TAG.log" | cut -c1-400
