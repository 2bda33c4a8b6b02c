#!/bin/bash
# Y'CbCr 4:2:0 input frames -> profiles/gpu_yuv_in_report.txt and profiles/yuv_in_timing.txt.
#   1: tests/test_gpu_yuv_in.py, verbose, with the slowest tests listed;
#   2: tools/bench_yuv_in.py -- refvsr_yuv420_to_rgb alone beside refvsr_ingest_u8 (rotated through more than the Infinity Cache, and
#      hot), then forward_group with input_yuv = 'nv12' against uint8 channels-last input, resident and copied from pinned host memory;
#   3: the default path against the PARENT commit: both trees run the same bench.py command (input_yuv = None) in alternating passes
#      of this one call, parent first and last (tools/bench_yuv.py --ab writes the summary).
# PARENT: a built checkout of the parent commit (default build/parent: `mkdir -p build/parent && git archive HEAD~1 | tar -x -C
# build/parent && make -C build/parent/refvsr_amd/csrc`).  Every GPU step under its own time limit; a failing step ends the script.  Output directory: $OUT_DIR (default build/yuv_in_timing,
# which git ignores).
set -o pipefail
HERE="$(pwd)"
PARENT="${PARENT:-build/parent}"
OUT="${OUT_DIR:-build/yuv_in_timing}"
mkdir -p "$OUT"
OUT="$(cd "$OUT" && pwd)"
timeout -k 10 300 python -m pytest tests/test_gpu_yuv_in.py -m gpu -v --durations=20 -p no:cacheprovider > "$OUT/gpu_yuv_in_report.txt" 2>&1 \
    || { tail -40 "$OUT/gpu_yuv_in_report.txt"; exit 1; }
sed -i '/^rootdir: /d;/^cachedir: /d' "$OUT/gpu_yuv_in_report.txt"          # (the checkout's own path says nothing about the run)
tail -3 "$OUT/gpu_yuv_in_report.txt"
timeout -k 10 420 python tools/bench_yuv_in.py --out "$OUT/yuv_in_timing.txt" > "$OUT/bench_yuv_in.log" 2>&1 || { tail -30 "$OUT/bench_yuv_in.log"; exit 1; }
BENCH="bench.py --gpus 1 --steps 20 --warmup 5 --no-other-configs --no-kernels --no-live-pmc --no-cpu-baseline"
n=0
run() {  # tree directory, tree name
    n=$((n + 1))
    (cd "$1" && timeout -k 10 240 python $BENCH --full-json "$OUT/$2_full_$n.json" > "$OUT/$2_$n.json" 2> "$OUT/$2_$n.err") || { tail -5 "$OUT/$2_$n.err"; return 1; }
}
run "$PARENT" parent && run "$HERE" new && run "$PARENT" parent && run "$HERE" new && run "$PARENT" parent || exit 1
python tools/bench_yuv.py --ab "$OUT" --out "$OUT/yuv_in_timing.txt"
cat "$OUT/yuv_in_timing.txt"
