#!/bin/bash
# The HD leg of tools/bench_eval_metrics.py (refvsr_score_frames_down at 1080 x 1920 <- 4320 x 7680: device events, the fused scorer against
# refvsr_score_frames on torch's GPU F.interpolate of the same 8K frames, evaluate() on RefVSR_small_MFID_8K with --metrics host and device)
# -> profiles/score_down_timing.txt.  One GPU step under its own time limit.
# Output directory: $OUT_DIR (default build/score_down, which git ignores).
set -o pipefail
OUT="${OUT_DIR:-build/score_down}"
mkdir -p "$OUT"
timeout -k 10 900 python tools/bench_eval_metrics.py --skip kernel,evaluate --reps 2 --hd_frames 5 --out "$OUT/score_down_timing.txt"
