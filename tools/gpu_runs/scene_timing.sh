#!/bin/bash
# Scene cuts -> profiles/gpu_scene_report.txt and profiles/scene_timing.txt.
#   1: tests/test_gpu_scene.py, verbose, with the slowest tests listed;
#   2: tools/bench_scene.py --only 1 -- refvsr_luma_sad alone, 5 pairs per call, rotated through more than the Infinity Cache, and hot;
#   3: tools/bench_scene.py --only 2 -- videorun's seconds per frame on a cut-free 64-frame 270 x 480 file: the PARENT commit's command,
#      this tree without options, this tree with --scene_cut 0.1, alternating passes, every pass a fresh process.
# Before it, on any machine (no GPU needed): `python tools/bench_scene.py --make-file build/scene_timing`, and PARENT, a built checkout
# of the parent commit (default build/parent: `mkdir -p build/parent && git archive HEAD~1 | tar -x -C build/parent && make -C
# build/parent/refvsr_amd/csrc`).  Every GPU step under its own time limit; a failing step ends the script.  Output directory:
# $OUT_DIR (default build/scene_timing, which git ignores).
set -o pipefail
PARENT="${PARENT:-build/parent}"
OUT="${OUT_DIR:-build/scene_timing}"
mkdir -p "$OUT"
OUT="$(cd "$OUT" && pwd)"
timeout -k 10 300 python -m pytest tests/test_gpu_scene.py -m gpu -v --durations=15 -p no:cacheprovider > "$OUT/gpu_scene_report.txt" 2>&1 \
    || { tail -40 "$OUT/gpu_scene_report.txt"; exit 1; }
sed -i '/^rootdir: /d;/^cachedir: /d' "$OUT/gpu_scene_report.txt"            # (the checkout's own path says nothing about the run)
tail -3 "$OUT/gpu_scene_report.txt"
timeout -k 10 240 python tools/bench_scene.py --only 1 --out "$OUT/scene_kernel.txt" > "$OUT/scene_kernel.log" 2>&1 || { tail -30 "$OUT/scene_kernel.log"; exit 1; }
timeout -k 10 900 python tools/bench_scene.py --only 2 --files build/scene_timing --parent "$PARENT" --out "$OUT/scene_videorun.txt" > "$OUT/scene_videorun.log" 2>&1 \
    || { tail -30 "$OUT/scene_videorun.log"; exit 1; }
cat "$OUT/scene_kernel.txt" "$OUT/scene_videorun.txt" > "$OUT/scene_timing.txt"
cat "$OUT/scene_timing.txt"
