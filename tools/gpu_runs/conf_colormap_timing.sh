#!/bin/bash
# Timing of refvsr_conf_colormap (16 maps per call at 270 x 480 and 1080 x 1920) -> profiles/conf_colormap.txt (command 1), then the two kernels'
# durations from a trace in a run of its own (command 2).  Every GPU step under its own time limit; a failing step ends the script.
# Output directory: $OUT_DIR (default build/conf_colormap, which git ignores).
set -o pipefail
OUT="${OUT_DIR:-build/conf_colormap}"
mkdir -p "$OUT"
timeout -k 10 240 python tools/bench_conf_colormap.py --out "$OUT/conf_colormap.txt" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o colormap -- python tools/bench_conf_colormap.py --out "$OUT/conf_colormap_trace_leg.txt"
