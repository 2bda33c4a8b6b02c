#!/usr/bin/env python3
"""Kernel by kernel: the resources and the instruction stream of one tree's device assembly against another's.

  python tools/kernel_resource_table.py PARENT_ASM_DIR NEW_ASM_DIR yuv yuv_in [--rename OLD=NEW ...]

Both directories come from `make -C refvsr_amd/csrc asm ASMDIR=...` (tools/device_asm_digest.py has the flags' story).  One row per
kernel of the named sources: .vgpr_count, .sgpr_count, .private_segment_fixed_size (scratch), .group_segment_fixed_size (LDS) and the
instruction count of both trees, the VGPR allocation granules (of 8), and whether the instruction streams are equal up to symbol and
label names.  Kernels are matched by their demangled names after --rename, a kernel of the parent that has fewer template arguments
than its match is padded with --pad (the arguments the merged template added).  Needs c++filt (binutils; CXXFILT names another), no GPU."""
import argparse
import os
import re
import subprocess
import sys

CXXFILT = os.environ.get('CXXFILT', 'c++filt')
FIELDS = ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')


def kernels(path):
    """{mangled name: (fields dict, [normalised instruction lines])} of one .s file."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r'^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:', text, flags=re.M | re.S):
        name, body = m.group(1), m.group(2)
        ins = []
        for line in body.split('\n'):
            line = line.split(';')[0].strip()
            if not line or line.startswith('.') and not line.startswith('.LBB') or line.endswith(':') and not line.startswith('.LBB'):
                continue
            line = re.sub(r'\.LBB\d+_(\d+)', r'.LBB_\1', line)
            ins.append(re.sub(r'\b_Z\w+', 'SYM', line))
        out[name] = [None, ins]
    for m in re.finditer(r'^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)', text, flags=re.M | re.S):
        blk = m.group(0)
        name = re.search(r'^\s+\.name:\s+(\S+)', blk, flags=re.M).group(1)
        if name in out:
            out[name][0] = dict((f, int(re.search(r'^\s+%s:\s+(\d+)' % re.escape(f), blk, flags=re.M).group(1))) for f in FIELDS)
    return out


def demangle(names):
    # (DF16_, _Float16, is newer than binutils' c++filt: it goes in as Dh, 'half')
    res = subprocess.run([CXXFILT], input='\n'.join(n.replace('DF16_', 'Dh') for n in names), capture_output=True, text=True, check=True).stdout.split('\n')
    return dict(zip(names, (re.sub(r'^void |\(.*$', '', r).replace('half', '_Float16') for r in res)))


def key_of(name, renames, pad):
    base, args = re.match(r'(\w+)<(.*)>$', name).groups() if '<' in name else (name, '')
    args = [a.strip().replace('(unsigned char)', '') for a in args.split(',')] if args else []
    if base in renames:
        base, args = renames[base], args + (pad.get(base) or [])
    return '%s<%s>' % (base, ', '.join(args))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('parent')
    ap.add_argument('new')
    ap.add_argument('sources', nargs='+', help='source names without .hip')
    ap.add_argument('--rename', action='append', default=[], help='OLD=NEW kernel template name')
    ap.add_argument('--pad', action='append', default=[], help="OLD=ARG,ARG: template arguments appended to a renamed parent kernel's")
    a = ap.parse_args()
    renames = dict(r.split('=') for r in a.rename)
    pad = dict((k, v.split(',')) for k, v in (p.split('=') for p in a.pad))
    bad = 0
    for src in a.sources:
        sides = []
        for d in (a.parent, a.new):
            ks = kernels(os.path.join(d, src + '.s'))
            dm = demangle(sorted(ks))
            sides.append(dict((key_of(dm[n], renames, pad), ks[n]) for n in ks))
        old, new = sides
        print('== %s.hip: %d kernels in the parent, %d here' % (src, len(old), len(new)))
        print('%-62s %-23s %-23s %s' % ('kernel (the name here)', 'parent v/s/scratch/lds/ins', 'here v/s/scratch/lds/ins', 'granules  stream'))
        for k in sorted(set(old) | set(new)):
            o, n = old.get(k), new.get(k)
            cell = lambda e: '-' if e is None else '%d/%d/%d/%d/%d' % (tuple(e[0][f] for f in FIELDS) + (len(e[1]),))
            note = 'only one side'
            if o and n:
                go, gn = -(-o[0]['.vgpr_count'] // 8), -(-n[0]['.vgpr_count'] // 8)
                note = '%2d -> %2d  %s' % (go, gn, 'equal' if o[1] == n[1] else 'DIFFERENT')
                bad += gn > go or n[0]['.private_segment_fixed_size'] > 0
            else:
                bad += 1
            print('%-62s %-23s %-23s %s' % (k, cell(o), cell(n), note))
    print('rows with scratch, more VGPR granules than the parent, or no partner: %d' % bad)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
