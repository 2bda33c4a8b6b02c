#!/bin/bash
# Where videorun's wall time goes (tools/bench_videorun_io.py) -> profiles/videorun_stream_timing.txt: whole-run wall seconds per frame
# of --io sync, --io stream and --io stream --out /dev/null on a 544 x 960 pair in /dev/shm, then the same at --io_depth 1.  Every GPU
# step under its own time limit; a failing step ends the script.  Output directory: $OUT_DIR (default build/videorun_stream, which git
# ignores).
set -o pipefail
OUT="${OUT_DIR:-build/videorun_stream}"
mkdir -p "$OUT"
timeout -k 10 400 python tools/bench_videorun_io.py --frames 64 --passes 3 --out "$OUT/depth2.txt" &&
timeout -k 10 400 python tools/bench_videorun_io.py --frames 64 --passes 3 --io_depth 1 --out "$OUT/depth1.txt" &&
cat "$OUT/depth2.txt" "$OUT/depth1.txt" > "$OUT/videorun_stream_timing.txt"
