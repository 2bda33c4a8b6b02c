#!/bin/bash
# 4:2:2, 4:4:4 and left-sited frames -> profiles/gpu_yuv_chroma_report.txt and profiles/yuv_chroma_timing.txt.
#   1: tests/test_gpu_yuv_chroma.py, verbose, with the slowest tests listed;
#   2: tools/bench_yuv_chroma.py -- every new kernel alone, both ways, at 1080p and 8K next to the 4:2:0 / centre kernel of the same
#      repeats (rotated through more than the Infinity Cache, and hot); the unchanged 4:2:0 / centre launches of the PARENT's library
#      against this tree's in alternating passes of one process; forward_group with result_yuv = 'i444p10' against None;
#   3: the default path against the PARENT commit: both trees run the same bench.py command (no yuv field set) in alternating passes of
#      this one call, parent first and last (tools/bench_yuv.py --ab writes the summary).
# PARENT: a built checkout of the parent commit (default build/parent: `mkdir -p build/parent && git archive HEAD~1 | tar -x -C
# build/parent && make -C build/parent/refvsr_amd/csrc`).  Every GPU step under its own time limit; a failing step ends the script.
# Output directory: $OUT_DIR (default build/yuv_chroma_timing, which git ignores).  STEPS (default 123) chooses the steps.
set -o pipefail
HERE="$(pwd)"
PARENT="${PARENT:-build/parent}"
OUT="${OUT_DIR:-build/yuv_chroma_timing}"
STEPS="${STEPS:-123}"
mkdir -p "$OUT"
OUT="$(cd "$OUT" && pwd)"
if [[ "$STEPS" == *1* ]]; then
    timeout -k 10 300 python -m pytest tests/test_gpu_yuv_chroma.py -m gpu -v --durations=20 -p no:cacheprovider > "$OUT/gpu_yuv_chroma_report.txt" 2>&1 \
        || { tail -40 "$OUT/gpu_yuv_chroma_report.txt"; exit 1; }
    sed -i '/^rootdir: /d;/^cachedir: /d' "$OUT/gpu_yuv_chroma_report.txt"      # (the checkout's own path says nothing about the run)
    tail -3 "$OUT/gpu_yuv_chroma_report.txt"
fi
if [[ "$STEPS" == *2* ]]; then
    timeout -k 10 420 python tools/bench_yuv_chroma.py --parent "$PARENT/refvsr_amd/librefvsr_hip.so" --out "$OUT/yuv_chroma_timing.txt" \
        > "$OUT/bench_yuv_chroma.log" 2>&1 || { tail -30 "$OUT/bench_yuv_chroma.log"; exit 1; }
    cat "$OUT/yuv_chroma_timing.txt"
fi
if [[ "$STEPS" == *3* ]]; then
    BENCH="bench.py --gpus 1 --steps 20 --warmup 5 --no-other-configs --no-kernels --no-live-pmc --no-cpu-baseline"
    n=0
    run() {  # tree directory, tree name
        n=$((n + 1))
        (cd "$1" && timeout -k 10 240 python $BENCH --full-json "$OUT/$2_full_$n.json" > "$OUT/$2_$n.json" 2> "$OUT/$2_$n.err") || { tail -5 "$OUT/$2_$n.err"; return 1; }
    }
    run "$PARENT" parent && run "$HERE" new && run "$PARENT" parent && run "$HERE" new && run "$PARENT" parent || exit 1
    python tools/bench_yuv.py --ab "$OUT" --out "$OUT/yuv_chroma_timing.txt"
    tail -8 "$OUT/yuv_chroma_timing.txt"
fi
