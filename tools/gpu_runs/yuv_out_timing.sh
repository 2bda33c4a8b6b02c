#!/bin/bash
# Y'CbCr 4:2:0 result frames -> profiles/yuv_out_timing.txt.
#   1 + 2: tools/bench_yuv.py -- refvsr_result_to_yuv420 alone against refvsr_convert_result_hwc (rotated through more than the
#          Infinity Cache, and hot), then forward_group with result_yuv = 'nv12' against None, on the device and with the copy to
#          pinned host memory;
#   3:     the default path against the PARENT commit: both trees run the same bench.py command (result_yuv = None) in alternating
#          passes of this one call, parent first and last.
# PARENT: a built checkout of the parent commit (default build/parent: `git worktree add build/parent HEAD~1 && make -C
# build/parent/refvsr_amd/csrc`).  Every GPU step under its own time limit; a failing step ends the script.  Output directory:
# $OUT_DIR (default build/yuv_out_timing, which git ignores).
set -o pipefail
HERE="$(pwd)"
PARENT="${PARENT:-build/parent}"
OUT="${OUT_DIR:-build/yuv_out_timing}"
PASSES="${PASSES:-2}"
mkdir -p "$OUT"
OUT="$(cd "$OUT" && pwd)"
BENCH="bench.py --gpus 1 --steps 20 --warmup 5 --no-other-configs --no-kernels --no-live-pmc --no-cpu-baseline"
timeout -k 10 420 python tools/bench_yuv.py --out "$OUT/yuv_out_timing.txt" > "$OUT/bench_yuv.log" 2>&1 || { tail -20 "$OUT/bench_yuv.log"; exit 1; }
n=0
run() {  # tree directory, tree name
    n=$((n + 1))
    (cd "$1" && timeout -k 10 240 python $BENCH --full-json "$OUT/$2_full_$n.json" > "$OUT/$2_$n.json" 2> "$OUT/$2_$n.err") || { tail -5 "$OUT/$2_$n.err"; return 1; }
}
for i in $(seq "$PASSES"); do
    run "$PARENT" parent && run "$HERE" new || exit 1
done
run "$PARENT" parent || exit 1
python tools/bench_yuv.py --ab "$OUT" --out "$OUT/yuv_out_timing.txt"
cat "$OUT/yuv_out_timing.txt"
