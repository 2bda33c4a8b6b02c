"""Summary of the weight-check A/B (tools/gpu_runs/weight_check_ab.sh): the parent tree and this tree ran `bench.py --gpus 1 --steps 20
--warmup 5 --full` in alternating passes of ONE call; every pass left its stdout line in <dir>/<tree>_<pass>.json.  Per leg (the
headline group mode, one_frame_per_call, dropin_surface): every pass's value, the median per tree, the parent-vs-parent spread
(min / median of the parent's passes), new / parent, and the verdict against the bar -- new >= 0.99 x the parent's median, or inside
the parent's own spread where that is wider.  With --trace DIR: the fingerprint kernels' durations per grid size from the
rocprofv3 kernel trace found under DIR.

    python tools/weight_check_ab.py DIR [--trace DIR] [--kernel-report FILE] > profiles/weight_check_ab.txt
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

LEGS = (('group mode (value)', lambda r: r), ('one_frame_per_call', lambda r: r.get('one_frame_per_call') or {}),
        ('dropin_surface', lambda r: r.get('dropin_surface') or {}))


def last_json_line(path):
    rec = None
    for ln in open(path):
        ln = ln.strip()
        if ln.startswith('{'):
            try:
                rec = json.loads(ln)
            except ValueError:
                pass
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('dir')
    ap.add_argument('--trace', default=None)
    ap.add_argument('--kernel-report', default=None)
    a = ap.parse_args()
    runs = {'parent': [], 'new': []}
    order = []
    passes = []
    for path in glob.glob(os.path.join(a.dir, '*.json')):
        m = re.match(r'^(parent|new)_(\d+)\.json$', os.path.basename(path))
        if m:
            passes.append((int(m.group(2)), m.group(1), path))
    for _, tree, path in sorted(passes):
        rec = last_json_line(path)
        if rec:
            runs[tree].append(rec)
            order.append(tree)
    print('# weight-check A/B: bench.py --gpus 1 --steps 20 --warmup 5 --full (other legs switched off), one GPU call, passes in the order')
    print('# %s; frames/s, each value = the median of the pass\'s 5 timed repeats' % ' '.join(order))
    ok_all = bool(runs['parent'] and runs['new'])
    for leg, pick in LEGS:
        vals = {t: [pick(r).get('value') for r in rs if pick(r).get('value')] for t, rs in runs.items()}
        if not vals['parent'] or not vals['new']:
            print('%-22s not measured' % leg)
            ok_all = False
            continue
        mp, mn = statistics.median(vals['parent']), statistics.median(vals['new'])
        spread = min(vals['parent']) / mp
        bar = min(0.99, spread)
        ok = mn >= bar * mp
        ok_all = ok_all and ok
        print('%-22s parent %s median %.2f (min / median %.4f) | new %s median %.2f | new / parent %.4f | bar %.4f -> %s'
              % (leg, ['%.2f' % v for v in vals['parent']], mp, spread, ['%.2f' % v for v in vals['new']], mn, mn / mp, bar,
                 'within' if ok else 'MISSED'))
    print('# verdict: %s' % ('every leg within the bar' if ok_all else 'NOT every leg within the bar'))
    if a.kernel_report and os.path.exists(a.kernel_report):
        print('#\n# tools/bench_param_fingerprint.py (device events, host clocks):')
        sys.stdout.write(open(a.kernel_report).read())
    if a.trace:
        files = glob.glob(os.path.join(a.trace, '**', '*kernel_trace.csv'), recursive=True)
        print('#\n# rocprofv3 --kernel-trace --stats -- python tools/bench_param_fingerprint.py: kernel durations per grid size (a run of its own)')
        if not files:
            print('kernel trace: not measured')
        per = {}
        for f in files:
            for row in csv.DictReader(open(f)):
                name = row.get('Kernel_Name', '')
                if 'fp_chunk_kernel' in name or 'fp_finish_kernel' in name:
                    key = ('fp_chunk_kernel' if 'fp_chunk' in name else 'fp_finish_kernel', int(row.get('Grid_Size_X') or row.get('Grid_Size') or 0))
                    per.setdefault(key, []).append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e3)
        for (name, grid), us in sorted(per.items()):
            print('%-18s grid %8d threads: %5d launches, median %.2f us, min %.2f, max %.2f' % (name, grid, len(us), statistics.median(us), min(us), max(us)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
