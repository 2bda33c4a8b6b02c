#!/bin/bash
# Cost of the weight check (config.weight_check = 'auto') against the PARENT commit -> profiles/weight_check_ab.txt.
# PARENT: a built checkout of the parent commit (default build/parent: `git worktree add build/parent HEAD~1 && make -C
# build/parent/refvsr_amd/csrc`).  Both trees run the same bench command on the same seeded inputs in alternating passes of this one
# call (parent first and last: the parent's own passes give the parent-vs-parent spread), then the fingerprint kernels are timed per
# parameter set, once with device events and once under a kernel trace in a run of its own.  Every GPU step under its own time
# limit; a failing step ends the script.  Output directory: $OUT_DIR (default build/weight_check_ab, which git ignores).
set -o pipefail
HERE="$(pwd)"
PARENT="${PARENT:-build/parent}"
OUT="${OUT_DIR:-build/weight_check_ab}"
PASSES="${PASSES:-3}"
mkdir -p "$OUT"
OUT="$(cd "$OUT" && pwd)"
BENCH="bench.py --gpus 1 --steps 20 --warmup 5 --full --no-other-configs --no-kernels --no-live-pmc --no-cpu-baseline --no-wavefront"
n=0
run() {  # tree directory, tree name
    n=$((n + 1))
    (cd "$1" && timeout -k 10 300 python $BENCH --full-json "$OUT/$2_full_$n.json" > "$OUT/$2_$n.json" 2> "$OUT/$2_$n.err") || { tail -5 "$OUT/$2_$n.err"; return 1; }
}
for i in $(seq "$PASSES"); do
    run "$PARENT" parent && run "$HERE" new || exit 1
done
run "$PARENT" parent || exit 1
timeout -k 10 240 python tools/bench_param_fingerprint.py --out "$OUT/weight_check_kernel.txt" > "$OUT/kernel_bench.log" 2>&1 || { tail -5 "$OUT/kernel_bench.log"; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o fingerprint -- python tools/bench_param_fingerprint.py --out "$OUT/weight_check_kernel_trace_leg.txt" > "$OUT/kernel_trace.log" 2>&1 || { tail -5 "$OUT/kernel_trace.log"; exit 1; }
python tools/weight_check_ab.py "$OUT" --trace "$OUT/prof" --kernel-report "$OUT/weight_check_kernel.txt" | tee "$OUT/weight_check_ab.txt"
