#!/bin/bash
# Timing of refvsr_score_regions beside refvsr_score_frames, the float64 host path and a whole evaluate() call -> profiles/score_regions_timing.txt
# (command 1), then the kernel durations from a trace in a run of its own (command 2).  Every GPU step under its own time limit; a failing step ends the script.
# Output directory: $OUT_DIR (default build/score_regions, which git ignores).
set -o pipefail
OUT="${OUT_DIR:-build/score_regions}"
mkdir -p "$OUT"
timeout -k 10 400 python tools/bench_score_regions.py --reps 3 --out "$OUT/score_regions_timing.txt" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o regions -- python tools/bench_score_regions.py --skip evaluate,host --out "$OUT/score_regions_trace_leg.txt"
