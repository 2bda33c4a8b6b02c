#!/usr/bin/env python3
"""Digest of every kernel source's device assembly: one `sha256  lines  file` row per csrc/*.hip.

Runs `make asm` of refvsr_amd/csrc (the objects' own flags plus --cuda-device-only -S) into a
temporary directory and hashes each .s without the lines that hold `__hip_cuid`, the per-compile
unique id.  Two trees whose rows agree run the same device code.  Needs hipcc, no GPU.

  python tools/device_asm_digest.py [-j N] [REPO_ROOT]
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile


def digest(root, jobs):
    csrc = os.path.join(root, 'refvsr_amd', 'csrc')
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call(['make', '-C', csrc, '-j%d' % jobs, 'asm', 'ASMDIR=' + tmp],
                              stdout=sys.stderr)
        for name in sorted(os.listdir(tmp)):
            with open(os.path.join(tmp, name), 'rb') as f:
                lines = [l for l in f if b'__hip_cuid' not in l]
            rows.append((hashlib.sha256(b''.join(lines)).hexdigest(), len(lines),
                         'csrc/' + name[:-2] + '.hip'))
    return rows


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('root', nargs='?',
                    default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('-j', type=int, default=8)
    a = ap.parse_args()
    for sha, n, name in digest(a.root, a.j):
        print('%s  %6d  %s' % (sha, n, name))
